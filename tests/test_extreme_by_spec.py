"""The maxBy / minBy aggregators off the GPU: JSON, the lowering's refusals, and SQL max_by / min_by of
a CPU session as one pushed query (torch takes the same lexicographic extreme there) against the
same statement over the base table."""
import copy

import pytest

from spark_druid_olap_amd.engine.executor import Engine
from spark_druid_olap_amd.engine.lower import LoweringError
from spark_druid_olap_amd.models import tpch
from spark_druid_olap_amd.query import spec as S
from spark_druid_olap_amd.segment.datasource import MetricColumn
from spark_druid_olap_amd.session import Session
from spark_druid_olap_amd.sql.analyzer import AnalysisError

T = "orderLineItemPartSupplier"
IV = ["1990-01-01/2000-01-01"]
CLASSES = [S.MaxByAggregationSpec, S.MinByAggregationSpec]


@pytest.fixture(scope="module")
def session():
    f = tpch.generate_flat(0.002, "cpu")
    ds, df = tpch.to_datasource(f, profile="bench"), tpch.to_pandas(f)
    s = Session(engine=Engine(use_native=False))
    s.register_datasource(ds)
    s.register_table(T + "Base", df, schema=tpch.FLAT_SCHEMA)
    s.sql(tpch.druid_ddl(with_column_mapping=False))
    return s, ds, df


@pytest.mark.parametrize("cls", CLASSES)
def test_json_round_trip(cls):
    spec = cls("v", "l_extendedprice", "__time")
    j = spec.to_json()
    assert j["type"] == ("maxBy" if cls is S.MaxByAggregationSpec else "minBy") and j["jsonClass"] == cls.__name__
    assert (j["fieldName"], j["byFieldName"]) == ("l_extendedprice", "__time")
    assert S.from_json(j, "aggregation") == spec
    assert S.from_json({"type": j["type"], "name": "v", "fieldName": "l_extendedprice", "byFieldName": "__time"},
                       "aggregation") == spec


@pytest.mark.parametrize("cls", CLASSES)
def test_refusals(session, cls):
    _, ds, _ = session

    def lower(x, y, d, agg=None, **kw):
        q = S.GroupByQuerySpec(d.name, [], aggregations=[agg or cls("v", x, y)], intervals=IV)
        return Engine(use_native=False, **kw).prepare(q, d)

    dd = copy.copy(ds)
    m = ds.metrics["l_quantity"]
    dd.metrics = dict(ds.metrics, dbl=MetricColumn("dbl", "double", m.data.double()),
                      sk=MetricColumn("sk", "hll", m.data, sketch=object()))
    # (an integer max / min per group is bitwise reproducible: a double ordering column lowers in deterministic mode)
    pq = lower("l_quantity", "dbl", dd, deterministic=True)
    assert pq._full_prog.extremes == [("v", "l_quantity", "dbl", cls is S.MaxByAggregationSpec)]
    assert [a.out_type for a in pq._full_prog.aggs] == ["long"]
    assert [a.out_type for a in lower("l_extendedprice", "__time", dd)._full_prog.aggs] == ["double"]  # (a decimal)
    for x, y in (("sk", "l_quantity"), ("l_quantity", "sk")):
        with pytest.raises(LoweringError, match="sketch metric"):
            lower(x, y, dd)
    for x, y in (("l_quantity", "l_shipmode"), ("l_shipmode", "l_quantity"), ("__time", "l_quantity")):
        with pytest.raises(LoweringError, match="not a metric"):
            lower(x, y, dd)
    with pytest.raises(LoweringError, match="filtered"):
        lower("", "", dd, S.FilteredAggregationSpec(S.SelectorFilterSpec("l_shipmode", "AIR"),
                                                    cls("v", "l_quantity", "l_tax")))

    class TwoRanks:  # (only what lowering reads of a world: every rank would answer for its own shard)
        distributed, size, rank = True, 2, 0

    eng = Engine(use_native=False)
    eng.world = TwoRanks()
    with pytest.raises(LoweringError, match="across ranks"):
        eng.prepare(S.GroupByQuerySpec(dd.name, [], aggregations=[cls("v", "l_quantity", "l_tax")], intervals=IV), dd)


@pytest.mark.parametrize("fn", ["max_by", "min_by"])
def test_sql_is_one_pushed_query(session, fn):
    s, _, df = session
    q = f"select o_orderkey, {fn}(l_quantity, l_extendedprice), avg(l_quantity), count(*) " \
        "from %s where o_orderkey < 400 group by o_orderkey"
    d = s.sql(q % T)
    specs = d.druid_query_specs()
    assert len(specs) == 1, d.explain()
    cls = S.MaxByAggregationSpec if fn == "max_by" else S.MinByAggregationSpec
    assert sum(isinstance(a, cls) for a in specs[0].aggregations) == 1
    got, want = (sorted(x.collect()) for x in (d, s.sql(q % (T + "Base"))))
    assert len(got) == len(want) > 50
    # shard order is not the base table's: a group's value is one of the payloads at its extreme, and
    # THE payload where only one row holds the extreme (l_extendedprice: nearly every order)
    sub = df[df.o_orderkey < 400]
    ext = sub.groupby("o_orderkey").l_extendedprice.transform("max" if fn == "max_by" else "min")
    allowed = sub[sub.l_extendedprice == ext].groupby("o_orderkey").l_quantity.agg(set)
    single = 0
    for g, w in zip(got, want):
        assert g[0] == w[0] and g[2:] == w[2:]
        assert g[1] in allowed[g[0]], (g, w)
        if len(allowed[g[0]]) == 1:
            single += 1
            assert g[1] == w[1]
    assert single >= 0.8 * len(got)


def test_sql_time_ordering_global_and_errors(session):
    s, _, df = session
    q = "select l_returnflag, max_by(l_quantity, cast(l_shipdate as date)), min_by(l_quantity, cast(l_shipdate as date))" \
        " from %s group by l_returnflag"
    d = s.sql(q % T)
    (spec,) = d.druid_query_specs()
    assert sorted((a.type, a.byFieldName) for a in spec.aggregations) == [("maxBy", "__time"), ("minBy", "__time")]
    for flag, last, first in d.collect():
        sub = df[df.l_returnflag == flag]
        assert last in set(sub.l_quantity[sub.l_shipdate == sub.l_shipdate.max()])
        assert first in set(sub.l_quantity[sub.l_shipdate == sub.l_shipdate.min()])
    # a global min_by over the base table: the first row among those with the smallest quantity
    (v,), = s.sql(f"select min_by(l_extendedprice, l_quantity) from {T}Base").collect()
    assert v == df.l_extendedprice[df.l_quantity == df.l_quantity.min()].iloc[0]
    for bad in ("max_by(distinct l_quantity, l_tax)", "min_by(l_quantity)", "max_by(l_quantity, l_tax, l_tax)",
                "max_by(l_quantity, l_tax) over (partition by o_orderkey)"):
        with pytest.raises(AnalysisError):
            s.sql(f"select {bad} from {T}Base").collect()
