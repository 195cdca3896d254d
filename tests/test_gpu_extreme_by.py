"""max_by / min_by on the device (ops/csrc/extreme.hip through PreparedExtremes) against a plain loop
over the host columns: the payload of the kept row at max / min of (y, row index).  The answer is
unique, so every comparison is exact equality.

Every query asks for all four payload types (int16, int64, double, decimal) over one ordering column
and one or both directions: they must share one accumulation.  Ordering columns: int16 in +-100
(dense ties: the tie rule decides most groups), a decimal stored as int32 and ``__time`` (about 70
distinct days) take the packed pass; int64 of both signs beyond 2^32 and doubles of both signs the two
wide passes.

Key spaces: 7 groups (few), 1,200 (one LDS table), 5,000 (one table of one-word states, two key
slices of two-word states: 4,096 a table) and 5,000 x 8 (beyond 4 slices of either: global)."""
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
SHAPES = {"g7": (["g7"], "few"), "g1200": (["g1200"], "lds"), "g5k": (["g5k"], "lds"), "g40k": (["g5k", "g8"], "global")}
ORDERINGS = ["y16", "ydec", "y64", "yd", "__time"]
PAYLOADS = ["p16", "p64", "pd", "pdec"]
SCALE = {"ydec": 2, "pdec": 2}
DIRS = {"max": [True], "min": [False], "both": [True, False]}
ONE, TIED, GONE = (("g7_%05d" % i,) for i in (0, 2, 3))


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(11)
    keep = rng.random(N) < 0.5
    g7 = rng.choice(np.arange(4, 7), size=N, p=[0.7, 0.25, 0.05])
    g7[100] = 0                                                   # a group of one row
    g7[rng.choice(np.arange(300, 8000), 40, replace=False)] = 2   # every row ties on y
    g7[rng.choice(np.arange(8001, 8999), 30, replace=False)] = 3  # every row filtered out
    keep[100] = True
    keep[g7 == 3] = False
    ids = {"flt": np.where(keep, 0, 1), "g7": g7, "g1200": rng.permutation(N) % 1200,
           "g5k": rng.permutation(N) % 5000, "g8": rng.integers(0, 8, N)}
    dicts, dim_ids = {}, {}
    for k, v in ids.items():
        names = np.asarray([f"{k}_{i:05d}" for i in range(int(v.max()) + 1)], dtype=object)
        dicts[k], codes = Dictionary.build(names[v])
        dim_ids[k] = torch.from_numpy(np.asarray(codes, dtype=np.int64))
        ids[k] = names[v]
    sign = rng.choice([-1, 1], N)
    cols = {"y16": rng.integers(-100, 101, N).astype(np.int16),
            "ydec": rng.integers(-50_000, 50_000, N).astype(np.int32),
            "y64": sign * ((1 << 33) + rng.integers(0, 50, N)),   # ties in the value, not in the low word alone
            "yd": np.round(rng.standard_normal(N), 1) * 1e3 + 0.5,  # both signs, ties, no -0.0
            "p16": rng.integers(-30000, 30000, N).astype(np.int16), "p64": sign * ((1 << 40) + np.arange(N)),
            "pd": rng.standard_normal(N), "pdec": rng.integers(-10 ** 6, 10 ** 6, N).astype(np.int32)}
    for c, v in (("y16", 7), ("ydec", -1234), ("y64", -(1 << 33) - 5), ("yd", -2.5)):
        cols[c][g7 == 2] = v
    kinds = dict.fromkeys(cols, "long")
    kinds.update(ydec="decimal", pdec="decimal", yd="double", pd="double")
    days = (np.arange(N) * 70) // N + 18262
    ds = make_datasource("ext", N, torch.from_numpy(days), DAY, dim_ids, dicts,
                         {k: torch.from_numpy(v) for k, v in cols.items()}, kinds, SCALE)
    return ds.to("cuda"), dict(ids, __time=days, **cols), keep


@pytest.fixture(scope="module")
def oracle(data):
    """(dimensions, ordering column, is max) -> {group key: row index at the extreme of (y, i)},
    computed once for the cases that share it."""
    _, host, keep = data
    memo = {}

    def get(dims, by, is_max):
        if (*dims, by, is_max) not in memo:
            best = {}
            for i in np.flatnonzero(keep).tolist():
                k, cand = tuple(host[d][i] for d in dims), (host[by][i].item(), i)
                if k not in best or (cand > best[k] if is_max else cand < best[k]):
                    best[k] = cand
            memo[(*dims, by, is_max)] = {k: i for k, (_, i) in best.items()}
        return memo[(*dims, by, is_max)]

    return get


def _run(ds, dims, aggs, having=None):
    q = S.GroupByQuerySpec("ext", [S.DefaultDimensionSpec(d) for d in dims], filter=FLT, aggregations=aggs,
                           having=having, intervals=IV)
    pq = Engine().prepare(q, ds)
    r = pq.run()
    ep = pq.__dict__.get("_extremes_prep")
    assert isinstance(ep, device_exec.PreparedExtremes)  # the HIP extremes answered, not torch
    assert r.stats["extremes_device"] == ep.tiers          # ... and the result says so
    return ep, r, list(zip(*(materialize(r.data[d]).tolist() for d in dims)))


def _payload(host, x, i):
    v = host[x][i].item()
    return v / 10 ** SCALE[x] if x in SCALE else v


def _check(host, keys, r, name, x, rows):
    assert len(keys) == len(rows) and set(keys) == set(rows)
    got = np.asarray(r.data[name])
    assert got.dtype == (np.int64 if x in ("p16", "p64") else np.float64)
    assert got.tolist() == [_payload(host, x, rows[k]) for k in keys], name


@pytest.mark.parametrize("dirs", list(DIRS))
@pytest.mark.parametrize("by", ORDERINGS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_payload_at_the_extreme_is_exact(data, oracle, shape, by, dirs):
    ds, host, keep = data
    dims, tier = SHAPES[shape]
    cls = {True: S.MaxByAggregationSpec, False: S.MinByAggregationSpec}
    aggs = [cls[mx](f"{x}_{int(mx)}", x, by) for mx in DIRS[dirs] for x in PAYLOADS]
    ep, r, keys = _run(ds, dims, aggs)
    packed = by in ("y16", "ydec", "__time")
    assert ep.rw == (2 if by == "__time" else 4) and ep.tiers == [tier]  # one accumulation for all payloads
    assert list(ep.passes.values()) == [(0 if by == "__time" else 2, packed, {"max": 1, "min": 2, "both": 3}[dirs])]
    for mx in DIRS[dirs]:
        rows = oracle(dims, by, mx)
        for x in PAYLOADS:
            _check(host, keys, r, f"{x}_{int(mx)}", x, rows)
        if shape == "g7":
            tied = [i for i in np.flatnonzero(keep).tolist() if host["g7"][i] == TIED[0]]
            assert rows[ONE] == 100 and GONE not in rows and len(tied) > 5
            if by != "__time":  # (all of the group's rows tie: the last wins a max_by, the first a min_by)
                assert rows[TIED] == (tied[-1] if mx else tied[0])


def test_orderings_share_the_producer_and_having_reads_the_column(data, oracle):
    ds, host, _ = data
    rows = oracle(["g7"], "y16", True)
    vals = sorted(host["p16"][i].item() for i in rows.values())
    c = (vals[len(vals) // 2 - 1] + vals[len(vals) // 2]) / 2
    aggs = [S.MaxByAggregationSpec("a", "p16", "y16"), S.MaxByAggregationSpec("b", "pdec", "y16"),
            S.MinByAggregationSpec("c", "pd", "y16"), S.MinByAggregationSpec("d", "p64", "yd"),
            S.FunctionAggregationSpec("count", "n")]
    ep, r, keys = _run(ds, ["g7"], aggs, having=S.ComparisonHavingSpec("greaterThan", "a", c))
    # one producer pass over both ordering columns, one accumulation for the three aggregators over y16
    assert ep.rw == 6 and ep.passes == {"y16": (2, True, 3), "yd": (4, False, 2)} and ep.tiers == ["few", "few"]
    assert set(keys) == {k for k, i in rows.items() if host["p16"][i] > c} and 0 < len(keys) < len(rows)
    for name, x, by, mx in (("a", "p16", "y16", True), ("b", "pdec", "y16", True), ("c", "pd", "y16", False),
                            ("d", "p64", "yd", False)):
        want = oracle(["g7"], by, mx)
        _check(host, keys, r, name, x, {k: want[k] for k in keys})
