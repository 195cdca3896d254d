"""The HIP scan kernels (per-query JIT and precompiled interpreter) against the plain oracles of
tests/scan_oracles.py -- never against ops/reference.py, whose calendar arithmetic is the same
algorithm and which also fills the kernels' time lookup table.

Where each opcode is asserted in this file (every test but test_jit_staging runs for jit and interp):

=====================================================  =========================================
T_SECOND T_MINUTE T_HOUR T_DAY T_MONTH T_YEAR           test_time_formats (absolute patterns),
                                                        test_granularities
T_MOY T_DOM T_DOW T_HOD T_MOH T_SOM T_DOY               test_time_formats, test_jit_staging
T_MS T_WEEK T_QUARTER T_PERIOD                          test_granularities (none / week /
                                                        quarter, P3M / fifteen_minute, duration,
                                                        PT6H)
T_QOY                                                   test_quarter_of_year
E_COL E_CONST E_ADD E_SUB E_MUL E_DIV E_NEG E_ABS       test_expressions (E_MIN / E_MAX also
E_MIN E_MAX E_FLOOR E_CEIL E_SQRT E_LOG E_EXP E_MOD     test_min_max_ignore_nan)
E_PMOD E_POW E_LUT
F_EXPR over every operation                             test_expression_filters
F_FLT_RANGE F_INT_RANGE F_IN_SET F_ID_RANGE F_BITMAP    test_range_filters, test_padding_rows
F_NOT
A_MIN_I A_MAX_I A_SUM_I A_MIN_F A_MAX_F A_SUM_F         test_min_max_sum
A_SUM_X                                                 test_exact_decimal_sum
=====================================================  =========================================

cal_minutes, epoch_ms and secs_wide run the device calendar arithmetic (``time_field_t`` /
``time_field``); secs_lut takes the JIT's lookup table.
"""
import numpy as np
import pytest

import scan_oracles as O
from spark_druid_olap_amd.engine.executor import Engine
from spark_druid_olap_amd.ops import desc as D

pytestmark = pytest.mark.gpu

TIME_CASES = [(s, z) for s in O.TIME_SHARDS for z, _ in O.ZONES]


@pytest.fixture(scope="module", params=["jit", "interp"], autouse=True)
def kernel_path(request):
    from spark_druid_olap_amd.engine import device_exec as DE

    old = DE.USE_JIT
    DE.USE_JIT = request.param == "jit"
    yield request.param
    DE.USE_JIT = old


@pytest.fixture(scope="module")
def eng():
    return Engine(use_native=True)


_GPU = {}


def gpu_shard(name):
    if name not in _GPU:
        _GPU[name] = O.shard(name).to("cuda")
    return _GPU[name]


def _run(prog, mode=None):
    from spark_druid_olap_amd.engine.device_exec import PreparedScan

    return PreparedScan(prog, mode=mode).run()


@pytest.mark.parametrize("kind", list(O.FORMAT_GROUPS))
@pytest.mark.parametrize("name,zone", TIME_CASES)
def test_time_formats(eng, name, zone, kind):
    O.check_formats(eng, gpu_shard(name), zone, O.FORMAT_GROUPS[kind])


@pytest.mark.parametrize("name,zone", TIME_CASES)
def test_granularities(eng, name, zone):
    O.check_granularities(eng, gpu_shard(name), zone)


@pytest.mark.parametrize("name,zone", TIME_CASES)
def test_quarter_of_year(name, zone):
    O.quarter_of_year_counts(gpu_shard(name), dict(O.ZONES)[zone], _run)


@pytest.mark.parametrize("kernel_path", ["jit"], indirect=True)  # the interpreter has one staging path
@pytest.mark.parametrize("stage", ["lds", "reg"])
@pytest.mark.parametrize("name", O.TIME_SHARDS)
def test_jit_staging(eng, kernel_path, name, stage):
    """Both column staging paths of the JIT (LDS-DMA planes, VGPR loads) feed the time key."""
    assert kernel_path == "jit"
    from spark_druid_olap_amd.engine import device_exec as DE

    old = DE.JIT_STAGE
    DE.JIT_STAGE = stage
    try:
        O.check_formats(eng, gpu_shard(name), O.ZONES[0][0], groups=[["MM", "dd", "e", "HH"], ["D"]])
        O.check_granularities(eng, gpu_shard(name), O.ZONES[1][0], names=["week"])
    finally:
        DE.JIT_STAGE = old


def test_expressions(eng):
    O.check_expressions(eng, gpu_shard("values"))


def test_min_max_ignore_nan(eng):
    """E_MIN / E_MAX with one NaN operand return the other operand (scan_desc.h)."""
    sh = gpu_shard("values")
    a, b = sh.cols["f64"], sh.cols["y"]
    one = np.isnan(a) ^ np.isnan(b)
    got = O.rows_of_expr(eng, sh, {k: (["f64", "y"], O.EXPR_JS[k].format(a="a", b="b")) for k in ("min", "max")})
    other = np.where(np.isnan(a), b, a)
    for k in ("min", "max"):
        O.assert_float_rows(got[k][one], other[one], 0, k)
        assert np.isnan(got[k][np.isnan(a) & np.isnan(b)]).all()


def test_expression_depth_four(eng):
    """An expression using all four stack registers of the device VM."""
    sh = gpu_shard("values")
    got = O.rows_of_expr(eng, sh, {"v": (["f64", "y"], "b * (a - (b / a))")})["v"]
    a, b = sh.cols["f64"], sh.cols["y"]
    with np.errstate(all="ignore"):
        O.assert_float_rows(got, b * (a - (b / a)), 0, "depth 4")


def test_expression_filters(eng):
    O.check_expression_filters(eng, gpu_shard("values"))


def test_range_filters(eng):
    O.check_range_filters(eng, gpu_shard("values"))


@pytest.mark.parametrize("mode", [D.M_DENSE_LDS, D.M_DENSE_GLOBAL, D.M_HASH])
def test_padding_rows(mode):
    O.check_padding(gpu_shard("values"), lambda prog: _run(prog, mode))


def test_min_max_sum(eng):
    O.check_minmaxsum(eng, gpu_shard("values"))


def test_exact_decimal_sum(eng):
    O.check_exact_decimal_sum(eng, gpu_shard("values"))
