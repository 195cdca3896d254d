"""Exact COUNT(DISTINCT) on the device (ops/csrc/distinct.hip through PreparedDistinct) against
plain Python sets over the host columns."""
import numpy as np
import pytest
import torch

from spark_druid_olap_amd.engine import device_exec
from spark_druid_olap_amd.engine.columns import materialize
from spark_druid_olap_amd.engine.executor import Engine
from spark_druid_olap_amd.models import tpch
from spark_druid_olap_amd.query import spec as S
from spark_druid_olap_amd.segment.datasource import make_datasource
from spark_druid_olap_amd.segment.dictionary import Dictionary
from spark_druid_olap_amd.session import Session

pytestmark = pytest.mark.gpu

N = 3 * 4096 + 37  # three chunk regions and a ragged fourth
DAY = 86400000
IV = ["2019-01-01/2021-01-01"]
FLT = S.SelectorFilterSpec("flt", "a")


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(11)
    keep = rng.random(N) < 0.5
    g7 = rng.choice(np.arange(4, 7), size=N, p=[0.7, 0.25, 0.05])
    g7[100], g7[[200, 9000]] = 0, 1            # one group of 1 row, one of 2
    g7[rng.choice(np.arange(300, 8000), 40, replace=False)] = 2   # every row carries one value (below)
    g7[rng.choice(np.arange(8001, 8999), 30, replace=False)] = 3  # every row filtered out
    keep[[100, 200, 9000]] = True
    keep[g7 == 3] = False
    ids = {"flt": np.where(keep, 0, 1), "g7": g7, "g5k": rng.permutation(N) % 5000,
           "c33": rng.permutation(N) % 33, "c5k": rng.permutation(N) % 5000, "cnull": rng.integers(0, 12, N)}
    for c in ("c33", "c5k", "cnull"):
        ids[c][g7 == 2] = 7
    names = {"flt": ["a", "b"], "g7": [f"k{i}" for i in range(7)], "g5k": [f"v{i:04d}" for i in range(5000)],
             "c33": [f"c{i:02d}" for i in range(33)], "c5k": [f"d{i:04d}" for i in range(5000)],
             "cnull": [""] + [f"n{i:02d}" for i in range(11)]}
    dicts, dim_ids = {}, {}
    for k, v in ids.items():
        dicts[k], codes = Dictionary.build(np.asarray(names[k], dtype=object)[v])
        dim_ids[k] = torch.from_numpy(np.asarray(codes, dtype=np.int64))
    assert len(dicts["c33"]) == 33 and len(dicts["c5k"]) == 5000  # (a word boundary; 157 words a row)
    days = torch.from_numpy(18262 + (np.arange(N) * 70) // N)
    v = rng.integers(0, 100, N)
    ds = make_datasource("dc", N, days, DAY, dim_ids, dicts, {"v": torch.from_numpy(v)}, {"v": "long"}, {})
    host = dict({k: np.asarray(names[k], dtype=object)[x] for k, x in ids.items()}, v=v)
    return ds.to("cuda"), host, keep


def _want(host, sel, dim, col):
    """{group: distinct non-null values of ``col``} over the rows ``sel``, by Python sets."""
    out = {}
    for g, c in zip(host[dim][sel].tolist() if dim else [None] * int(sel.sum()), host[col][sel].tolist()):
        out.setdefault(g, set()).add(c)
    return {g: len(v - {""}) for g, v in out.items()}


def _run(ds, dim, aggs, having=None):
    q = S.GroupByQuerySpec("dc", [S.DefaultDimensionSpec(dim)] if dim else [], filter=FLT, aggregations=aggs,
                           having=having, intervals=IV)
    pq = Engine().prepare(q, ds)
    r = pq.run()
    dp = pq.__dict__.get("_distinct_prep")
    assert isinstance(dp, device_exec.PreparedDistinct)  # the HIP bitsets answered, not torch
    keys = materialize(r.data[dim]).tolist() if dim else [None]
    return dp, r, keys


@pytest.mark.parametrize("force_global", [False, True])
@pytest.mark.parametrize("col", ["c33", "c5k", "cnull"])
@pytest.mark.parametrize("dim", [None, "g7", "g5k"])
def test_distinct_counts_match_sets(data, monkeypatch, dim, col, force_global):
    ds, host, keep = data
    monkeypatch.setattr(device_exec, "DISTINCT_FORCE_GLOBAL", force_global)
    dp, r, keys = _run(ds, dim, [S.DistinctCountAggregationSpec("d", col)])
    words = (len(set(host[dim])) if dim else 1) * -(-len(set(host[col])) // 32)
    tier = "global" if force_global or words > 16384 else "lds"
    assert dp.tiers == [tier] and r.stats["distinct_count_device"] == tier
    got = np.asarray(r.data["d"])
    assert got.dtype == np.int64 and dict(zip(keys, got.tolist())) == _want(host, keep, dim, col)


def test_two_distincts_share_one_producer_pass(data):
    ds, host, keep = data
    dp, r, keys = _run(ds, "g7", [S.DistinctCountAggregationSpec("a", "c33"), S.FunctionAggregationSpec("count", "n"),
                                  S.DistinctCountAggregationSpec("b", "cnull"),
                                  S.FunctionAggregationSpec("longSum", "s", "v")])
    assert dp.rw == 3  # one record: the group key and one id word per counted column
    for name, col in (("a", "c33"), ("b", "cnull")):
        assert dict(zip(keys, np.asarray(r.data[name]).tolist())) == _want(host, keep, "g7", col)
    assert dict(zip(keys, np.asarray(r.data["n"]).tolist())) == \
        {g: int((host["g7"][keep] == g).sum()) for g in set(host["g7"][keep])}
    assert int(np.asarray(r.data["s"]).sum()) == int(host["v"][keep].sum())


def test_filtered_distinct_and_having(data):
    ds, host, keep = data
    inner = S.SelectorFilterSpec("cnull", "n03")
    aggs = [S.DistinctCountAggregationSpec("d", "c33"),
            S.FilteredAggregationSpec(S.NotFilterSpec(inner), S.DistinctCountAggregationSpec("f", "c5k"))]
    _, r, keys = _run(ds, "g7", aggs, S.ComparisonHavingSpec("greaterThan", "d", 1))
    want_d = {g: n for g, n in _want(host, keep, "g7", "c33").items() if n > 1}
    want_f = _want(host, keep & (host["cnull"] != "n03"), "g7", "c5k")
    assert dict(zip(keys, np.asarray(r.data["d"]).tolist())) == want_d
    assert dict(zip(keys, np.asarray(r.data["f"]).tolist())) == {g: want_f.get(g, 0) for g in want_d}


def test_sql_count_distinct_is_one_pushed_query():
    f = tpch.generate_flat(0.002, "cpu")
    df, t = tpch.to_pandas(f), "orderLineItemPartSupplier"
    s = Session(engine=Engine(use_native=True), conf={"spark.sparklinedata.druid.distinctCount.pushdown": "all"})
    s.register_datasource(tpch.to_datasource(f, profile="bench").to("cuda"))
    s.register_table(t + "Base", df, schema=tpch.FLAT_SCHEMA)
    s.sql(tpch.druid_ddl(with_column_mapping=False))
    d = s.sql(f"select l_returnflag, count(distinct l_shipmode), count(distinct p_brand), sum(l_quantity), count(*) "
              f"from {t} where l_linestatus = 'F' group by l_returnflag")
    specs = d.druid_query_specs()
    assert len(specs) == 1, d.explain()
    assert sum(isinstance(a, S.DistinctCountAggregationSpec) for a in specs[0].aggregations) == 2
    sel = df[df.l_linestatus == "F"].groupby("l_returnflag")
    want = {k: (g.l_shipmode.nunique(), g.p_brand.nunique(), float(g.l_quantity.sum()), len(g)) for k, g in sel}
    assert {r[0]: (r[1], r[2], float(r[3]), r[4]) for r in d.collect()} == want
