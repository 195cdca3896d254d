"""The distinctCount aggregator off the GPU: JSON, the reference executor, and the SQL plan of a
CPU session (exact COUNT(DISTINCT) keeps its two-level rewrite there)."""
import numpy as np
import pytest

from spark_druid_olap_amd.engine.executor import Engine
from spark_druid_olap_amd.models import tpch
from spark_druid_olap_amd.query import spec as S
from spark_druid_olap_amd.session import Session

T = "orderLineItemPartSupplier"


@pytest.fixture(scope="module")
def flat():
    f = tpch.generate_flat(0.002, "cpu")
    return tpch.to_datasource(f, profile="bench"), tpch.to_pandas(f)


def test_distinct_count_json_round_trip():
    a = S.DistinctCountAggregationSpec("d", "l_shipmode")
    j = a.to_json()
    assert j["type"] == "distinctCount" and j["name"] == "d" and j["fieldName"] == "l_shipmode"
    assert S.from_json(j, "aggregation") == a


@pytest.mark.parametrize("dim", [None, "l_returnflag"])
def test_reference_executor_matches_sets(flat, dim):
    ds, df = flat
    aggs = [S.DistinctCountAggregationSpec("d", "p_brand"), S.FunctionAggregationSpec("count", "n"),
            S.FilteredAggregationSpec(S.SelectorFilterSpec("l_linestatus", "F"),
                                      S.DistinctCountAggregationSpec("f", "l_shipmode"))]
    q = S.GroupByQuerySpec(ds.name, [S.DefaultDimensionSpec(dim)] if dim else [], aggregations=aggs,
                           filter=S.SelectorFilterSpec("l_shipmode", "AIR"), intervals=["1990-01-01/2000-01-01"])
    r = Engine(use_native=False).prepare(q, ds).run().to_pandas()
    air = df[df.l_shipmode == "AIR"]
    groups = list(air.groupby(dim)) if dim else [(None, air)]
    assert len(r) == len(groups)
    for k, g in groups:
        row = r[r[dim] == k].iloc[0] if dim else r.iloc[0]
        assert (row.d, row.n, row.f) == (len(set(g.p_brand)), len(g), len(set(g[g.l_linestatus == "F"].l_shipmode)))


def test_cpu_session_keeps_two_level_plan(flat):
    ds, df = flat
    s = Session(engine=Engine(use_native=False))
    s.register_datasource(ds)
    s.register_table(T + "Base", df, schema=tpch.FLAT_SCHEMA)
    s.sql(tpch.druid_ddl(with_column_mapping=False))
    d = s.sql(f"select l_returnflag, count(distinct l_shipmode), sum(l_quantity) from {T} group by l_returnflag")
    specs = d.druid_query_specs()
    assert len(specs) == 2, d.explain()  # the regular half and the (l_returnflag, l_shipmode) inner level
    assert not any(isinstance(a, S.DistinctCountAggregationSpec) for q in specs for a in q.aggregations)
    want = {k: g.l_shipmode.nunique() for k, g in df.groupby("l_returnflag")}
    assert {r[0]: r[1] for r in d.collect()} == want
