"""Variance / stddev on the device (ops/csrc/moments.hip through PreparedMoments) against exact
``fractions.Fraction`` arithmetic over the host columns.

Bounds.  Integer / decimal columns: 4 ulp (relative 4 * 2^-52) of the correctly rounded exact value
-- one rounding each for the numerator, the denominator, their quotient, the division by a
decimal's 10^(2 scale) and the square root.  Double column (values 1e6 + N(0,1), kappa = mean /
sigma = 1e6): relative 1e-9 -- the corrected two-pass bound n u + n^2 kappa^2 u^2 is about 3e-12 at
n = 1.2e4, the uncentred formula would err by kappa^2 u = 1e-4; ``np.var`` must meet the same bound
on the same groups."""
import decimal
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from spark_druid_olap_amd.engine import device_exec
from spark_druid_olap_amd.engine.columns import materialize
from spark_druid_olap_amd.engine.executor import Engine
from spark_druid_olap_amd.query import spec as S
from spark_druid_olap_amd.segment.datasource import make_datasource
from spark_druid_olap_amd.segment.dictionary import Dictionary

pytestmark = pytest.mark.gpu

N = 3 * 4096 + 37  # three chunk regions and a ragged fourth
DAY = 86400000
IV = ["2019-01-01/2021-01-01"]
FLT = S.SelectorFilterSpec("flt", "flt_00000")
ULP4 = 4 * 2.0 ** -52
# group shape -> (dimensions, tier of an integer column, tier of a double column's first pass)
# (g1200: one LDS table; g5k: 3-4 key slices of one; g40k: global atomics -- but a double column's
# count-and-sum states are 12 B, so its first pass still runs sliced and only its second is global)
SHAPES = {"g7": (["g7"], "few", "few"), "g1200": (["g1200"], "lds", "lds"), "g5k": (["g5k"], "lds", "lds"),
          "g40k": (["g5k", "g8"], "global", "lds")}
SCALE = {"dec": 2}


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(5)
    keep = rng.random(N) < 0.5
    g7 = rng.choice(np.arange(4, 7), size=N, p=[0.7, 0.25, 0.05])
    g7[100], g7[[200, 9000]] = 0, 1            # one group of 1 row, one of 2
    g7[rng.choice(np.arange(300, 8000), 40, replace=False)] = 2   # every row carries one value (below)
    g7[rng.choice(np.arange(8001, 8999), 30, replace=False)] = 3  # every row filtered out
    keep[[100, 200, 9000]] = True
    keep[g7 == 3] = False
    ids = {"flt": np.where(keep, 0, 1), "g7": g7, "g1200": rng.permutation(N) % 1200,
           "g5k": rng.permutation(N) % 5000, "g8": rng.integers(0, 8, N)}
    dicts, dim_ids = {}, {}
    for k, v in ids.items():
        names = np.asarray([f"{k}_{i:05d}" for i in range(int(v.max()) + 1)], dtype=object)
        dicts[k], codes = Dictionary.build(names[v])
        dim_ids[k] = torch.from_numpy(np.asarray(codes, dtype=np.int64))
        ids[k] = names[v]
    cols = {"q": rng.integers(0, 100, N).astype(np.int16),                                    # two digits
            "big": (rng.choice([-1, 1], N) * (3_000_000_000 + rng.integers(0, 1000, N))),     # sum x^2 > 2^64
            "near": 10 ** 12 + rng.integers(0, 3, N),                                         # x^2 > 2^64, var < 1
            "dec": rng.integers(-50_000, 50_000, N).astype(np.int32),                         # cents
            "x": 1e6 + rng.standard_normal(N)}
    for c, v in (("q", 7), ("big", -3_000_000_005), ("near", 10 ** 12 + 1), ("dec", 1234)):
        cols[c][g7 == 2] = v
    kinds = {"q": "long", "big": "long", "near": "long", "dec": "decimal", "x": "double"}
    days = torch.from_numpy(18262 + (np.arange(N) * 70) // N)
    ds = make_datasource("mom", N, days, DAY, dim_ids, dicts, {k: torch.from_numpy(v) for k, v in cols.items()},
                         kinds, SCALE)
    return ds.to("cuda"), dict(ids, **cols), keep


def _exact(xs, ddof, scale=0):
    """The variance of ``xs`` (ints or doubles, taken exactly) as a Fraction; None where n <= ddof."""
    n = len(xs)
    if n <= ddof:
        return None
    fx = [Fraction(x) for x in xs]
    s1, s2 = sum(fx), sum(x * x for x in fx)
    return (n * s2 - s1 * s1) / (n * (n - ddof)) / Fraction(10) ** (2 * scale)


def _sqrt(fr):
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        return float((decimal.Decimal(fr.numerator) / decimal.Decimal(fr.denominator)).sqrt())


def _groups(host, keep, dims, col):
    out = {}
    for *k, v in zip(*(host[d][keep].tolist() for d in dims), host[col][keep].tolist()):
        out.setdefault(tuple(k), []).append(v)
    return out


def _run(ds, dims, aggs, post=(), having=None):
    q = S.GroupByQuerySpec("mom", [S.DefaultDimensionSpec(d) for d in dims], filter=FLT, aggregations=aggs,
                           postAggregations=list(post), having=having, intervals=IV)
    pq = Engine().prepare(q, ds)
    r = pq.run()
    mp = pq.__dict__.get("_moments_prep")
    assert isinstance(mp, device_exec.PreparedMoments)  # the HIP moment sums answered, not torch
    keys = list(zip(*(materialize(r.data[d]).tolist() for d in dims)))
    return mp, r, keys


def _check(keys, got, want, bound):
    assert len(keys) == len(want) and set(keys) == set(want)
    for k, g in zip(keys, np.asarray(got, dtype=np.float64).tolist()):
        w = want[k]
        if w is None:
            assert math.isnan(g), (k, g)
        else:
            assert g >= 0.0 and abs(g - w) <= bound * abs(w), (k, g, w, abs(g - w) / abs(w) if w else g)


@pytest.mark.parametrize("col", ["q", "big", "near", "dec"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_integer_variance_and_stddev_are_exact(data, shape, col):
    ds, host, keep = data
    dims, tier, _ = SHAPES[shape]
    aggs = [S.VarianceAggregationSpec("vs", col), S.VarianceAggregationSpec("vp", col, "population")]
    mp, r, keys = _run(ds, dims, aggs, [S.StddevPostAggregationSpec("sd", "vs")])
    assert mp.rw == 3 and mp.tiers == [tier]
    groups = _groups(host, keep, dims, col)
    for name, ddof in (("vs", 1), ("vp", 0)):
        ex = {k: _exact(v, ddof, SCALE.get(col, 0)) for k, v in groups.items()}
        _check(keys, r.data[name], {k: None if e is None else float(e) for k, e in ex.items()}, ULP4)
        if ddof:
            _check(keys, r.data["sd"], {k: None if e is None else _sqrt(e) for k, e in ex.items()}, ULP4)
    if shape == "g7":
        vs, vp = (dict(zip(keys, np.asarray(r.data[c]).tolist())) for c in ("vs", "vp"))
        one, two, flat = (("g7_00000",), ("g7_00001",), ("g7_00002",))
        assert math.isnan(vs[one]) and vp[one] == 0.0 and not math.isnan(vs[two]) and vs[flat] == 0.0 and vp[flat] == 0.0
        assert ("g7_00003",) not in vs


@pytest.mark.parametrize("shape", list(SHAPES))
def test_double_variance_two_pass(data, shape):
    ds, host, keep = data
    dims, _, tier = SHAPES[shape]
    aggs = [S.VarianceAggregationSpec("vs", "x"), S.VarianceAggregationSpec("vp", "x", "population")]
    mp, r, keys = _run(ds, dims, aggs)
    assert mp.tiers == [tier]
    groups = _groups(host, keep, dims, "x")
    for name, ddof in (("vs", 1), ("vp", 0)):
        want = {k: None if len(v) <= ddof else float(_exact(v, ddof)) for k, v in groups.items()}
        _check(keys, r.data[name], want, 1e-9)
        ref = [np.var(np.asarray(groups[k]), ddof=ddof) if want[k] is not None else np.nan for k in keys]
        _check(keys, ref, want, 1e-9)  # (the bound is attainable: the reference formula meets it)


def test_having_reads_the_variance(data):
    ds, host, keep = data
    want = {k: float(_exact(v, 1)) for k, v in _groups(host, keep, ["g7"], "q").items() if len(v) > 1}
    c = sorted(want.values())[len(want) // 2]
    aggs = [S.VarianceAggregationSpec("v", "q"), S.VarianceAggregationSpec("w", "dec", "population"),
            S.FunctionAggregationSpec("count", "n")]
    mp, r, keys = _run(ds, ["g7"], aggs, having=S.ComparisonHavingSpec("greaterThan", "v", c))
    assert mp.rw == 5  # one record: the group key and two value words per column
    assert set(keys) == {k for k, w in want.items() if w > c} and 0 < len(keys) < len(want)
    _check(keys, r.data["v"], {k: want[k] for k in keys}, ULP4)
