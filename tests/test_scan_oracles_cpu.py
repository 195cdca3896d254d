"""The reference executor (``Engine(use_native=False)``) and the host decoders against the plain
oracles of tests/scan_oracles.py: time fields at calendar edges, expression VM, filters, padding.

Where each opcode is asserted in this file:

=====================================================  =========================================
T_SECOND T_MINUTE T_HOUR T_DAY T_MONTH T_YEAR           test_reference_time_formats (absolute
                                                        patterns), test_reference_granularities
T_MOY T_DOM T_DOW T_HOD T_MOH T_SOM T_DOY               test_reference_time_formats,
                                                        test_day_of_year_labels,
                                                        test_extract_labels
T_MS T_WEEK T_QUARTER T_PERIOD                          test_reference_granularities
                                                        (none / week / quarter, P3M /
                                                        fifteen_minute, duration, PT6H)
T_QOY                                                   test_reference_quarter_of_year
E_COL E_CONST E_ADD E_SUB E_MUL E_DIV E_NEG E_ABS       test_reference_expressions
E_MIN E_MAX E_FLOOR E_CEIL E_SQRT E_LOG E_EXP E_MOD     (E_MIN / E_MAX also
E_PMOD E_POW E_LUT                                      test_min_max_ignore_nan)
F_EXPR over every operation                             test_reference_expression_filters
F_FLT_RANGE F_INT_RANGE F_IN_SET F_ID_RANGE F_BITMAP    test_reference_range_filters,
F_NOT                                                   test_reference_padding_rows
A_MIN_I A_MAX_I A_SUM_I A_MIN_F A_MAX_F A_SUM_F         test_reference_min_max_sum
A_SUM_X                                                 test_reference_exact_decimal_sum
=====================================================  =========================================
"""
import ast
import os

import numpy as np
import pytest

import scan_oracles as O
from spark_druid_olap_amd.engine.executor import Engine
from spark_druid_olap_amd.engine.lower import Lowerer, LoweringError, tz_offset_ms
from spark_druid_olap_amd.ops.reference import run_reference
from spark_druid_olap_amd.query import spec as S

TIME_CASES = [(s, z) for s in O.TIME_SHARDS for z, _ in O.ZONES]


@pytest.fixture(scope="module")
def eng():
    return Engine(use_native=False)


def test_oracles_are_independent():
    """scan_oracles.py imports none of the engine's own calendar code at module level or inside
    its oracle functions."""
    tree = ast.parse(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "scan_oracles.py")).read())
    banned = ("ops.reference", "query.intervals", "query.joda")
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):
            mod = node.module or ""
            assert not mod.endswith(banned), mod
            if mod.endswith("query.granularity"):  # only the Granularity spec class, to build queries
                assert [a.name for a in node.names] == ["Granularity"]
            if mod.endswith(".query") or mod.endswith(".ops"):
                assert not {a.name for a in node.names} & {"reference", "intervals", "joda", "granularity"}


def test_shards_have_the_intended_shape():
    from spark_druid_olap_amd.query import joda
    from spark_druid_olap_amd.query.granularity import Granularity
    from spark_druid_olap_amd.segment.datasource import CHUNK_ROWS, padded_len

    assert set(joda._EXACT) == set(O.FORMATS) and joda.T_QOY == O.T_QOY
    for zone, tz_ms in O.ZONES:
        assert tz_offset_ms(zone) == tz_ms
    sizes = {"cal_minutes": 3264, "epoch_ms": O.N, "secs_wide": O.N, "secs_lut": O.N, "values": O.N}
    for name, n in sizes.items():
        sh = O.shard(name)
        assert sh.ds.num_rows == n == sh.n and n % CHUNK_ROWS and padded_len(n) > n
        assert n % 64 or name == "cal_minutes"  # (3 264 rows end on a word boundary, inside a chunk)
        kc = Lowerer(sh.ds).granularity_key(Granularity.parse("hour"), [])
        # only secs_lut (and the one-day values shard) may take the precomputed table
        assert (kc.tlut is not None) == (name in ("secs_lut", "values")), name
    c = O.shard("values").cols
    for col in ("u8", "i16", "i32", "i64", "dec", "f64", "f32", "grp", "row", "dnum"):
        assert (c[col] == 0).any(), col  # a zero-filled padding row would match real predicates
    assert np.isnan(c["f64"]).sum() >= 2 and np.isinf(c["f32"]).any()


@pytest.mark.parametrize("kind", list(O.FORMAT_GROUPS))
@pytest.mark.parametrize("name,zone", TIME_CASES)
def test_reference_time_formats(eng, name, zone, kind):
    O.check_formats(eng, O.shard(name), zone, O.FORMAT_GROUPS[kind])


@pytest.mark.parametrize("name,zone", TIME_CASES)
def test_reference_granularities(eng, name, zone):
    O.check_granularities(eng, O.shard(name), zone)


@pytest.mark.parametrize("name,zone", TIME_CASES)
def test_reference_quarter_of_year(name, zone):
    O.quarter_of_year_counts(O.shard(name), dict(O.ZONES)[zone], run_reference)


def _labels(eng, sh, fmt, zone=None):
    q = S.GroupByQuerySpec(sh.ds.name, [S.ExtractionDimensionSpec("__time", "t", S.TimeFormatExtractionFunctionSpec(fmt, zone))],
                           aggregations=[S.FunctionAggregationSpec("count", "c")], intervals=O.INTERVAL)
    r = eng.execute(q, sh.ds)
    return {str(t): int(c) for t, c in zip(r.data["t"], r.data["c"])}, r.num_rows


def test_day_of_year_labels(eng):
    """Day 366 is its own group labelled "366" (it used to be formatted inside a non-leap year
    and came back as a second "1")."""
    sh = O.shard("cal_minutes")
    got, nrows = _labels(eng, sh, "D")
    want = O.counts(O.format_labels(sh.ms, "D"))
    assert nrows == len(got) == 366
    assert "366" in got and got["366"] == want["366"] > 0
    assert got["1"] == want["1"] and got["1"] != got["366"]
    assert got == want
    got3, _ = _labels(eng, sh, "DDD")
    assert got3 == O.counts(O.format_labels(sh.ms, "DDD")) and "366" in got3 and "001" in got3


def test_extract_labels(eng):
    """The other field extracts are formatted from a representative instant too: the last days of
    the month, every month and every weekday keep their own label."""
    sh = O.shard("cal_minutes")
    for fmt, must in (("dd", ["29", "30", "31"]), ("d", ["29", "30", "31"]), ("MM", ["02", "12"]), ("MMMM", ["February"]),
                      ("e", ["1", "7"]), ("EEEE", ["Monday", "Sunday"]), ("HH", ["00", "23"]), ("mm", ["59"])):
        got, nrows = _labels(eng, sh, fmt)
        assert nrows == len(got)
        assert got == O.counts(O.format_labels(sh.ms, fmt)), fmt
        assert all(m in got for m in must), (fmt, sorted(got))


def _depth_agg(expr):
    return S.JavascriptAggregationSpec("v", ["f64", "y"], "function(current, a, b) { return Math.max(current, %s); }" % expr,
                                       "function(x, y) { return Math.max(x, y); }", "function() { return -Infinity; }")


def test_expression_depth(eng):
    """The device VM has four stack registers: an expression needing five is declined, one needing
    exactly four lowers and evaluates correctly."""
    sh = O.shard("values")
    four = "b * (a - (b / a))"  # pushes b, a, b, a before the first operation
    with pytest.raises(LoweringError):
        Lowerer(sh.ds).lower_aggregate(O.INTERVAL, None, [S.DefaultDimensionSpec("row")], None,
                                       [_depth_agg("a + (%s)" % four)])
    Lowerer(sh.ds).lower_aggregate(O.INTERVAL, None, [S.DefaultDimensionSpec("row")], None, [_depth_agg(four)])
    got = O.rows_of_expr(eng, sh, {"v": (["f64", "y"], four)})["v"]
    a, b = sh.cols["f64"], sh.cols["y"]
    with np.errstate(all="ignore"):
        O.assert_float_rows(got, b * (a - (b / a)), 0, "depth 4")


def test_reference_expressions(eng):
    O.check_expressions(eng, O.shard("values"))


def test_min_max_ignore_nan(eng):
    """E_MIN / E_MAX with one NaN operand return the other operand (scan_desc.h)."""
    sh = O.shard("values")
    a, b = sh.cols["f64"], sh.cols["y"]
    one = np.isnan(a) ^ np.isnan(b)
    assert one.sum() >= 10
    got = O.rows_of_expr(eng, sh, {k: (["f64", "y"], O.EXPR_JS[k].format(a="a", b="b")) for k in ("min", "max")})
    other = np.where(np.isnan(a), b, a)
    for k in ("min", "max"):
        O.assert_float_rows(got[k][one], other[one], 0, k)
        assert np.isnan(got[k][np.isnan(a) & np.isnan(b)]).all()


def test_nested_evaluator_min_max_ignore_nan():
    """The outer-query evaluator of the same expression ASTs (engine/nested.py) follows the rule."""
    import types

    import torch

    from spark_druid_olap_amd.engine.nested import _torch_eval
    from spark_druid_olap_amd.query.jsfunc import parse_expr

    sh = O.shard("values")
    a, b = sh.cols["f64"], sh.cols["y"]
    cols = {k: types.SimpleNamespace(num=None, decode=None, as_float=lambda v=v: torch.from_numpy(v))
            for k, v in (("a", a), ("b", b))}
    for k in ("min", "max"):
        got = _torch_eval(parse_expr(O.EXPR_JS[k].format(a="a", b="b")), {}, cols).numpy()
        z = (a == 0) & (b == 0)
        want = O.expr_expected(k, a, b)
        O.assert_float_rows(np.where(z, np.abs(got), got), np.where(z, np.abs(want), want), 0, "nested " + k)


def test_reference_expression_filters(eng):
    O.check_expression_filters(eng, O.shard("values"))


def test_reference_range_filters(eng):
    O.check_range_filters(eng, O.shard("values"))


def test_reference_padding_rows():
    O.check_padding(O.shard("values"), run_reference)


def test_reference_min_max_sum(eng):
    O.check_minmaxsum(eng, O.shard("values"))


def test_reference_exact_decimal_sum(eng):
    O.check_exact_decimal_sum(eng, O.shard("values"))
