"""Fixed-bucket histograms on the device (ops/csrc/histogram.hip through PreparedHistogram) against a
plain loop over the host columns with Fraction edges.  The counts are integers, so every comparison
is exact equality.

Columns: int16 in +-100, a decimal stored as int32 (scale 2), int64 of both signs beyond 2^32 and a
double of both signs with ties, -0.0, 0.0, NaNs of both signs and values exactly on edges, on lo and
on hi.  One group holds one row, one has every row filtered out, one holds outliers only.

Counter spaces: 7 groups x 7 counters (replicated 64 times) and x 1,024 (twice, the deepest search),
1,200 x 7 (one LDS table) and x 64 (256 groups a table: 5 key slices), 40,000 x 7 (global atomics)."""
import bisect
from fractions import Fraction

import numpy as np
import pytest
import torch

from spark_druid_olap_amd.engine import device_exec
from spark_druid_olap_amd.engine.columns import materialize
from spark_druid_olap_amd.engine.executor import Engine
from spark_druid_olap_amd.ops import buckets
from spark_druid_olap_amd.query import spec as S
from spark_druid_olap_amd.segment.datasource import make_datasource
from spark_druid_olap_amd.segment.dictionary import Dictionary

pytestmark = pytest.mark.gpu

N = 3 * 4096 + 37  # three chunk regions and a ragged fourth
DAY = 86400000
IV = ["2019-01-01/2021-01-01"]
FLT = S.SelectorFilterSpec("flt", "flt_00000")
H = S.FixedBucketsHistogramAggregationSpec
SHAPES = {"g7_b5": (["g7"], 5, "rep"), "g7_b1022": (["g7"], 1022, "rep"), "g1200_b5": (["g1200"], 5, "lds"),
          "g1200_b62": (["g1200"], 62, "lds"), "g40k_b5": (["g5k", "g8"], 5, "global")}
LIMITS = {"x16": (-50, 50), "xdec": (-250.5, 250.5), "x64": (-(1 << 33) - 20, (1 << 33) + 30), "xd": (-1, 1.5)}
SCALE = {"xdec": 2}
ONE, OUT, GONE = (("g7_%05d" % i,) for i in (0, 2, 3))


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(13)
    keep = rng.random(N) < 0.5
    g7 = rng.choice(np.arange(4, 7), size=N, p=[0.7, 0.25, 0.05])
    g7[100] = 0                                                   # a group of one row
    g7[rng.choice(np.arange(300, 8000), 40, replace=False)] = 2   # every row an outlier
    g7[rng.choice(np.arange(8001, 8999), 30, replace=False)] = 3  # every row filtered out
    keep[[5, 6, 100]] = True  # (rows 5 and 6: the NaNs)
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
    xd = np.round(rng.standard_normal(N), 1)  # ties; -1.0, -0.5, 0.5, 1.0, 1.5 lie on edges, lo and hi
    xd[xd == 0.0] = rng.choice([-0.0, 0.0], int((xd == 0.0).sum()))
    xd[[5, 6]] = np.asarray([0x7FF8000000000000, 0xFFF8000000000000], dtype=np.uint64).view(np.float64)
    cols = {"x16": rng.integers(-100, 101, N).astype(np.int16),
            "xdec": rng.integers(-50_000, 50_000, N).astype(np.int32),
            "x64": sign * ((1 << 33) + rng.integers(0, 50, N)), "xd": xd}
    for c, v in (("x16", 50), ("xdec", 25050), ("x64", (1 << 33) + 30), ("xd", 9.0)):
        cols[c][g7 == 2] = v  # (at hi or beyond: "above")
    kinds = {"x16": "long", "xdec": "decimal", "x64": "long", "xd": "double"}
    days = (np.arange(N) * 70) // N + 18262
    ds = make_datasource("fbh", N, torch.from_numpy(days), DAY, dim_ids, dicts,
                         {k: torch.from_numpy(v) for k, v in cols.items()}, kinds, SCALE)
    return ds.to("cuda"), dict(ids, **cols), keep


@pytest.fixture(scope="module")
def oracle(data):
    """(dimensions, column, edges) -> {group key: [below, c_0 .. c_{B-1}, above]} over the kept rows,
    computed once for the cases that share it."""
    _, host, keep = data
    memo = {}

    def get(dims, col, edges):
        key = (*dims, col, tuple(edges))
        if key not in memo:
            out = {}
            for i in np.flatnonzero(keep).tolist():
                v = host[col][i].item()
                if v != v:
                    slot = len(edges)  # NaN: above
                else:
                    slot = bisect.bisect_right(edges, Fraction(v) / 10 ** SCALE.get(col, 0))  # edges <= the value
                out.setdefault(tuple(host[d][i] for d in dims), [0] * (len(edges) + 1))[slot] += 1
            memo[key] = out
        return memo[key]

    return get


def _run(ds, dims, aggs):
    q = S.GroupByQuerySpec("fbh", [S.DefaultDimensionSpec(d) for d in dims], filter=FLT, aggregations=aggs, intervals=IV)
    pq = Engine().prepare(q, ds)
    r = pq.run()
    ep = pq.__dict__.get("_histogram_prep")
    assert isinstance(ep, device_exec.PreparedHistogram)  # the HIP bucket counts answered, not torch
    assert r.stats["histogram_device"] == ep.tiers          # ... and the result says so
    return ep, r, list(zip(*(materialize(r.data[d]).tolist() for d in dims)))


def _check(keys, r, name, want, mode="ignore"):
    assert len(keys) == len(want) and set(keys) == set(want)
    got = np.asarray(r.data[name])
    assert got.dtype == np.int64
    assert got.tolist() == buckets.apply_mode(np.asarray([want[k] for k in keys]), mode).tolist(), name


@pytest.mark.parametrize("mode", ["ignore", "overflow"])
@pytest.mark.parametrize("col", list(LIMITS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_counts_are_exact(data, oracle, shape, col, mode):
    ds, _, _ = data
    dims, B, tier = SHAPES[shape]
    lo, hi = LIMITS[col]
    ep, r, keys = _run(ds, dims, [H("h", col, B, lo, hi, mode)])
    assert ep.rw == 3 and ep.tiers == [tier]
    want = oracle(dims, col, buckets.bucket_edges(lo, hi, B))
    _check(keys, r, "h", want, mode)
    if dims == ["g7"]:
        assert sum(want[ONE]) == 1 and GONE not in want and want[OUT][-1] == sum(want[OUT]) > 5


def test_histograms_share_the_producer_and_equal_thresholds_an_accumulation(data, oracle):
    ds, _, _ = data
    aggs = [H("a", "x16", 5, -50, 50), H("b", "xd", 5, -1, 1.5), H("c", "x16", breaks=[-50, -30, -10, 10, 30, 50]),
            H("d", "x16", 5, -50, 50, "overflow"), S.FunctionAggregationSpec("count", "n", "count")]
    ep, r, keys = _run(ds, ["g7"], aggs)
    assert ep.rw == 5 and len(ep.passes) == 2 and ep.tiers == ["rep", "rep"]  # one pass, two accumulations
    x16, xd = (oracle(["g7"], c, buckets.bucket_edges(*LIMITS[c], 5)) for c in ("x16", "xd"))
    for name, want, mode in (("a", x16, "ignore"), ("b", xd, "ignore"), ("c", x16, "ignore"), ("d", x16, "overflow")):
        _check(keys, r, name, want, mode)
        assert np.asarray(r.data[name]).sum(axis=1).tolist() == np.asarray(r.data["n"]).tolist()
