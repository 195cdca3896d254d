"""The skewness / kurtosis aggregators off the GPU: JSON, the lowering's refusals, and SQL skewness /
kurtosis of a CPU session as one pushed query (the float64 two-pass fallback answers there) against
the same statement over the base table."""
import copy
import math

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
SPECS = [S.SkewnessAggregationSpec, S.KurtosisAggregationSpec]


@pytest.fixture(scope="module")
def session():
    f = tpch.generate_flat(0.002, "cpu")
    ds, df = tpch.to_datasource(f, profile="bench"), tpch.to_pandas(f)
    s = Session(engine=Engine(use_native=False))
    s.register_datasource(ds)
    s.register_table(T + "Base", df, schema=tpch.FLAT_SCHEMA)
    s.sql(tpch.druid_ddl(with_column_mapping=False))
    return s, ds


@pytest.mark.parametrize("cls", SPECS)
def test_json_round_trip(cls):
    spec = cls("s", "l_quantity")
    j = spec.to_json()
    assert j["type"] == cls.__name__[:8].lower() and j["fieldName"] == "l_quantity" and "jsonClass" in j
    assert S.from_json(j, "aggregation") == spec


@pytest.mark.parametrize("cls", SPECS)
def test_refusals(session, cls):
    _, ds = session

    def lower(x, d, agg=None, **kw):
        q = S.GroupByQuerySpec(d.name, [], aggregations=[agg or cls("v", x)], intervals=IV)
        return Engine(use_native=False, **kw).prepare(q, d)

    dd = copy.copy(ds)
    m = ds.metrics["l_quantity"]
    wide = m.data.long().clone()
    wide[0] += 1 << 32  # (an integer range of 2^32 and more goes through doubles as well)
    dd.metrics = dict(ds.metrics, dbl=MetricColumn("dbl", "double", m.data.double()),
                      wide=MetricColumn("wide", "long", wide), sk=MetricColumn("sk", "hll", m.data, sketch=object()))
    for col in ("dbl", "wide"):
        lower(col, dd)
        with pytest.raises(LoweringError, match="not bitwise reproducible"):
            lower(col, dd, deterministic=True)
    lower("l_quantity", dd, deterministic=True)  # (integer sums are reproducible)
    with pytest.raises(LoweringError, match="sketch metric"):
        lower("sk", dd)
    with pytest.raises(LoweringError, match="not a metric"):
        lower("l_shipmode", dd)
    with pytest.raises(LoweringError, match="filtered"):
        lower("", dd, S.FilteredAggregationSpec(S.SelectorFilterSpec("l_shipmode", "AIR"), cls("v", "l_quantity")))

    class TwoRanks:  # (only what lowering reads of a world: every rank would answer for its own shard)
        distributed, size, rank = True, 2, 0

    eng = Engine(use_native=False)
    eng.world = TwoRanks()
    with pytest.raises(LoweringError, match="across ranks"):
        eng.prepare(S.GroupByQuerySpec(dd.name, [], aggregations=[cls("v", "l_quantity")], intervals=IV), dd)


def test_sql_is_one_pushed_query(session):
    s, _ = session
    q = "select o_orderkey, skewness(l_extendedprice), kurtosis(l_quantity), avg(l_quantity), count(*) " \
        "from %s where o_orderkey < 400 group by o_orderkey"
    d = s.sql(q % T)
    specs = d.druid_query_specs()
    assert len(specs) == 1, d.explain()
    assert sum(isinstance(a, tuple(SPECS)) for a in specs[0].aggregations) == 2
    got, want = (sorted(x.collect()) for x in (d, s.sql(q % (T + "Base"))))
    assert len(got) == len(want) > 50
    nulls = 0
    for g, w in zip(got, want):
        assert g[0] == w[0] and g[3:] == w[3:]
        nulls += g[1] is None
        # (both sides are float64 two-pass formulas over at most 7 rows)
        assert (g[1] is None and w[1] is None) or abs(g[1] - w[1]) <= 1e-9 * (1 + abs(w[1])), (g, w)
        assert (g[2] is None and w[2] is None) or math.isclose(g[2] + 3, w[2] + 3, rel_tol=1e-9), (g, w)
        assert g[4] > 1 or (g[1] is None and g[2] is None)  # one-row orders
    assert nulls > 0


def test_sql_global_distinct_and_window(session):
    s, _ = session
    (sk, ku, n), = s.sql(f"select skewness(l_extendedprice), kurtosis(l_quantity), count(*) from {T}Base").collect()
    assert sk > 0.0 and -1.3 < ku < -1.1 and n > 1000  # (a uniform quantity: excess kurtosis -1.2)
    for bad in ("skewness(distinct l_quantity)", "kurtosis(l_quantity, l_tax)", "skewness(l_shipmode)",
                "kurtosis(l_quantity) over (partition by o_orderkey)"):
        with pytest.raises(AnalysisError):
            s.sql(f"select {bad} from {T}Base").collect()
