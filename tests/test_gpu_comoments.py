"""Covariance / correlation on the device (ops/csrc/comoments.hip through PreparedComoments) against
exact ``fractions.Fraction`` arithmetic over the host columns.

Bounds.  Integer / decimal pairs: 4 ulp (relative 4 * 2^-52) of the exact value -- a covariance
rounds its numerator, its denominator, their quotient and the decimal scale; a correlation three
numerators, their product, the square root and the quotient (at most 4.5 units of 2^-53) plus the
oracle's own half ulp.  Pairs with a double column (x = 1e6 + N(0,1), kappa = mean / sigma = 1e6):
|got - exact| <= 1e-11 sigma_x sigma_y (the group's own population sigmas) for a covariance and
<= 1e-11 for a correlation -- the corrected two-pass bound n u + (n u kappa)^2 is about 1.1e-12 at
the largest group (n ~ 6e3) for any summation order, the tolerance ten times that; numpy's centred
two-pass must meet the same bound on the same groups.

Every case runs with the correlation (the pair's state keeps the squares: 9 / 15 / 5 words) and
with the covariances alone (5 / 7 / 3 words: other paddings, LDS capacities and slice counts).

Key spaces: the 15-word state of a wide-integer correlation fits 564 groups in an LDS table, so
g1200 already takes three key slices and g5k nine, while the 5-word state (1,820 a table) holds
g1200 in one table and g5k in three; g5k x g8 (40,000) is beyond 16 tables of every integer state
(16 x 1,820 at most), while a double pair's first pass (20-byte states) still runs sliced there."""
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
# group shape -> (dimensions, tier of an integer pair, tier of a double pair's first pass)
SHAPES = {"g7": (["g7"], "few", "few"), "g1200": (["g1200"], "lds", "lds"), "g5k": (["g5k"], "lds", "lds"),
          "g40k": (["g5k", "g8"], "global", "lds")}
SCALE = {"dec": 2}
INT_PAIRS = [("a", "b"), ("big", "near"), ("a", "big"), ("dec", "a")]
DBL_PAIRS = [("x", "y"), ("a", "x")]
ONE, TWO, FLAT, GONE = (("g7_%05d" % i,) for i in range(4))


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(7)
    keep = rng.random(N) < 0.5
    g7 = rng.choice(np.arange(4, 7), size=N, p=[0.7, 0.25, 0.05])
    g7[100], g7[[200, 9000]] = 0, 1            # one group of 1 row, one of 2
    g7[rng.choice(np.arange(300, 8000), 40, replace=False)] = 2   # every row carries one pair (below)
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
    e = rng.standard_normal(N)
    cols = {"a": rng.integers(-100, 100, N).astype(np.int16), "b": rng.integers(-300, 300, N).astype(np.int16),
            "big": (rng.choice([-1, 1], N) * (3_000_000_000 + rng.integers(0, 1000, N))),  # four digits, both signs
            "near": 10 ** 12 + rng.integers(0, 3, N),                                      # covariance < 1
            "dec": rng.integers(-50_000, 50_000, N).astype(np.int32),                      # cents
            "x": 1e6 + e, "y": 2e6 + 0.5 * e + rng.standard_normal(N)}                     # rho ~ 0.45
    # the constant group (doubles with short mantissas: their sums and means are exact), and the two
    # rows of the 2-row group, which differ in every column by little (so +-1 is exact for integers)
    for c, flat, two in (("a", 7, (3, 10)), ("b", -3, (5, -2)), ("big", -3_000_000_005, (3 * 10 ** 9 + 1, 3 * 10 ** 9 + 7)),
                         ("near", 10 ** 12 + 1, (10 ** 12, 10 ** 12 + 2)), ("dec", 1234, (-100, 250)),
                         ("x", 1000000.5, (1e6 - 1.0, 1e6 + 2.0)), ("y", 2000000.25, (2e6 + 3.0, 2e6 - 1.0))):
        cols[c][g7 == 2] = flat
        cols[c][[200, 9000]] = two
    kinds = dict.fromkeys(cols, "long")
    kinds.update(dec="decimal", x="double", y="double")
    days = torch.from_numpy(18262 + (np.arange(N) * 70) // N)
    ds = make_datasource("como", N, days, DAY, dim_ids, dicts, {k: torch.from_numpy(v) for k, v in cols.items()},
                         kinds, SCALE)
    return ds.to("cuda"), dict(ids, **cols), keep


def _exact(host, keep, dims, cx, cy):
    """Per group key (n, A = n Sxy - Sx Sy, Vx, Vy) of the kept rows as exact Fractions, decimals
    in their units."""
    rows = {}
    for *k, x, y in zip(*(host[c][keep].tolist() for c in (*dims, cx, cy))):
        rows.setdefault(tuple(k), []).append((Fraction(x) / 10 ** SCALE.get(cx, 0), Fraction(y) / 10 ** SCALE.get(cy, 0)))
    out = {}
    for k, v in rows.items():
        n, sx, sy = len(v), sum(x for x, _ in v), sum(y for _, y in v)
        out[k] = (n, n * sum(x * y for x, y in v) - sx * sy, n * sum(x * x for x, _ in v) - sx * sx,
                  n * sum(y * y for _, y in v) - sy * sy)
    return out


def _want(ex, name):
    """The exact value of aggregator ``name`` as a float (None: undefined) and sigma_x sigma_y."""
    n, a, vx, vy = ex
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        root = (decimal.Decimal((vx * vy).numerator) / decimal.Decimal((vx * vy).denominator)).sqrt()
        if name == "r":
            ok = n >= 2 and vx and vy
            return float(decimal.Decimal(a.numerator) / decimal.Decimal(a.denominator) / root) if ok else None, 1.0
    ddof = 1 if name == "cs" else 0
    return None if n <= ddof else float(a / (n * (n - ddof))), float(root) / (n * n)


def _run(ds, dims, aggs, having=None):
    q = S.GroupByQuerySpec("como", [S.DefaultDimensionSpec(d) for d in dims], filter=FLT, aggregations=aggs,
                           having=having, intervals=IV)
    pq = Engine().prepare(q, ds)
    r = pq.run()
    cp = pq.__dict__.get("_comoments_prep")
    assert isinstance(cp, device_exec.PreparedComoments)  # the HIP co-moment sums answered, not torch
    assert r.stats["comoments_device"] == cp.tiers          # ... and the result says so
    keys = list(zip(*(materialize(r.data[d]).tolist() for d in dims)))
    return cp, r, keys


def _aggs(cx, cy, corr):
    """Both covariances, with the correlation (the pair's state then keeps the squares) or without."""
    cov = [S.CovarianceAggregationSpec("cs", cx, cy), S.CovarianceAggregationSpec("cp", cx, cy, "population")]
    return cov + [S.CorrelationAggregationSpec("r", cx, cy)] if corr else cov


def _check(keys, got, ex, name, rel, abs_):
    """``got`` within rel |exact| + abs_ sigma_x sigma_y of the exact value, NaN where undefined."""
    assert len(keys) == len(ex) and set(keys) == set(ex)
    for k, g in zip(keys, np.asarray(got, dtype=np.float64).tolist()):
        w, s = _want(ex[k], name)
        if w is None:
            assert math.isnan(g), (name, k, g)
        else:
            assert abs(g - w) <= rel * abs(w) + abs_ * s, (name, k, g, w, abs(g - w))


def _fixed(keys, r, corr):
    v = {n: dict(zip(keys, np.asarray(r.data[n]).tolist())) for n in ("cs", "cp") + (("r",) if corr else ())}
    assert math.isnan(v["cs"][ONE]) and v["cp"][ONE] == 0.0 and not math.isnan(v["cs"][TWO])
    assert v["cs"][FLAT] == 0.0 and v["cp"][FLAT] == 0.0 and GONE not in v["cs"]
    if corr:
        assert math.isnan(v["r"][ONE]) and abs(v["r"][TWO]) == 1.0 and math.isnan(v["r"][FLAT])
        assert all(math.isnan(x) or abs(x) <= 1.0 for x in v["r"].values())  # (the engine's own values: clamped)


@pytest.fixture(scope="module")
def exact(data):
    """The Fraction oracle per (dimensions, pair), computed once for the cases that share it."""
    _, host, keep = data
    memo = {}

    def get(dims, pair):
        if (*dims, *pair) not in memo:
            memo[(*dims, *pair)] = _exact(host, keep, dims, *pair)
        return memo[(*dims, *pair)]

    return get


@pytest.mark.parametrize("corr", [True, False], ids=["corr", "cov-only"])
@pytest.mark.parametrize("pair", INT_PAIRS, ids="-".join)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_integer_pairs_are_exact(data, exact, shape, pair, corr):
    ds, host, keep = data
    dims, tier, _ = SHAPES[shape]
    cp, r, keys = _run(ds, dims, _aggs(*pair, corr))
    assert cp.rw == 5 and cp.tiers == [tier] and [p[2] for p in cp.passes.values()] == [corr]
    for name in ("cs", "cp", "r")[:3 if corr else 2]:
        _check(keys, r.data[name], exact(dims, pair), name, ULP4, 0.0)
    if shape == "g7":
        _fixed(keys, r, corr)


@pytest.mark.parametrize("corr", [True, False], ids=["corr", "cov-only"])
@pytest.mark.parametrize("pair", DBL_PAIRS, ids="-".join)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pairs_with_a_double_column_two_pass(data, exact, shape, pair, corr):
    ds, host, keep = data
    dims, _, tier = SHAPES[shape]
    cp, r, keys = _run(ds, dims, _aggs(*pair, corr))
    assert cp.tiers == [tier] and [p[2] for p in cp.passes.values()] == [corr]
    ex = exact(dims, pair)
    groups = {}
    for *k, x, y in zip(*(host[c][keep].tolist() for c in (*dims, *pair))):
        groups.setdefault(tuple(k), []).append((x, y))
    for name, ddof in (("cs", 1), ("cp", 0), ("r", None))[:3 if corr else 2]:
        _check(keys, r.data[name], ex, name, 0.0, 1e-11)
        ref = []  # (the bound is attainable: numpy's centred two-pass meets it)
        for k in keys:
            x, y = np.asarray(groups[k], dtype=np.float64).T
            dx, dy = x - x.mean(), y - y.mean()
            with np.errstate(invalid="ignore", divide="ignore"):
                ref.append((dx * dy).sum() / np.sqrt((dx * dx).sum() * (dy * dy).sum()) if ddof is None
                           else (dx * dy).sum() / (len(x) - ddof))
        _check(keys, ref, ex, name, 0.0, 1e-11)
    if shape == "g7":
        _fixed(keys, r, corr)  # (the 2-row group's sums have two addends: +-1 is exact for doubles too)


def test_pair_is_accumulated_once_and_having_reads_the_correlation(data, exact):
    ds = data[0]
    ex = exact(["g7"], ("a", "b"))
    want = {k: _want(e, "r")[0] for k, e in ex.items() if _want(e, "r")[0] is not None}
    vals = sorted(want.values())
    c = (vals[len(vals) // 2 - 1] + vals[len(vals) // 2]) / 2  # (between two groups: no survivor hangs on an ulp)
    aggs = [S.CorrelationAggregationSpec("r", "a", "b"), S.CovarianceAggregationSpec("cp", "b", "a", "population"),
            S.FunctionAggregationSpec("count", "n")]
    cp, r, keys = _run(ds, ["g7"], aggs, having=S.ComparisonHavingSpec("greaterThan", "r", c))
    assert cp.rw == 5 and len(cp.passes) == 1 and cp.tiers == ["few"]  # one producer pass, one accumulation
    assert set(keys) == {k for k, w in want.items() if w > c} and 0 < len(keys) < len(want)
    _check(keys, r.data["r"], {k: ex[k] for k in keys}, "r", ULP4, 0.0)
    _check(keys, r.data["cp"], {k: ex[k] for k in keys}, "cp", ULP4, 0.0)
