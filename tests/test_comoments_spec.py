"""The covariance / correlation aggregators off the GPU: JSON, the lowering's refusals, and SQL
corr / covar_samp / covar_pop of a CPU session as one pushed query (the float64 two-pass fallback
answers there) against the same statement over the base table."""
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


@pytest.fixture(scope="module")
def session():
    f = tpch.generate_flat(0.002, "cpu")
    ds, df = tpch.to_datasource(f, profile="bench"), tpch.to_pandas(f)
    s = Session(engine=Engine(use_native=False))
    s.register_datasource(ds)
    s.register_table(T + "Base", df, schema=tpch.FLAT_SCHEMA)
    s.sql(tpch.druid_ddl(with_column_mapping=False))
    return s, ds


@pytest.mark.parametrize("spec", [S.CovarianceAggregationSpec("c", "l_quantity", "l_tax"),
                                  S.CovarianceAggregationSpec("c", "l_quantity", "l_tax", "population"),
                                  S.CorrelationAggregationSpec("c", "l_quantity", "l_tax")])
def test_json_round_trip(spec):
    j = spec.to_json()
    assert j["type"] in ("covariance", "correlation") and (j["fieldName"], j["fieldName2"]) == ("l_quantity", "l_tax")
    assert S.from_json(j, "aggregation") == spec
    d = S.from_json({"type": "covariance", "name": "c", "fieldName": "x", "fieldName2": "y"}, "aggregation")
    assert d.estimator == "sample"


@pytest.mark.parametrize("cls", [S.CovarianceAggregationSpec, S.CorrelationAggregationSpec])
def test_refusals(session, cls):
    _, ds = session

    def lower(x, y, d, agg=None, **kw):
        q = S.GroupByQuerySpec(d.name, [], aggregations=[agg or cls("v", x, y)], intervals=IV)
        return Engine(use_native=False, **kw).prepare(q, d)

    dd = copy.copy(ds)
    m = ds.metrics["l_quantity"]
    dd.metrics = dict(ds.metrics, dbl=MetricColumn("dbl", "double", m.data.double()),
                      sk=MetricColumn("sk", "hll", m.data, sketch=object()))
    lower("l_quantity", "dbl", dd)  # (a pair with a double column lowers ...)
    with pytest.raises(LoweringError, match="not bitwise reproducible"):
        lower("l_quantity", "dbl", dd, deterministic=True)  # ... but not in deterministic mode
    lower("l_quantity", "l_tax", dd, deterministic=True)  # (integer sums are reproducible)
    with pytest.raises(LoweringError, match="sketch metric"):
        lower("sk", "l_quantity", dd)
    with pytest.raises(LoweringError, match="not a metric"):
        lower("l_quantity", "l_shipmode", dd)
    with pytest.raises(LoweringError, match="filtered"):
        lower("", "", dd, S.FilteredAggregationSpec(S.SelectorFilterSpec("l_shipmode", "AIR"),
                                                    cls("v", "l_quantity", "l_tax")))

    class TwoRanks:  # (only what lowering reads of a world: every rank would answer for its own shard)
        distributed, size, rank = True, 2, 0

    eng = Engine(use_native=False)
    eng.world = TwoRanks()
    with pytest.raises(LoweringError, match="across ranks"):
        eng.prepare(S.GroupByQuerySpec(dd.name, [], aggregations=[cls("v", "l_quantity", "l_tax")], intervals=IV), dd)
    if cls is S.CovarianceAggregationSpec:
        with pytest.raises(LoweringError, match="unknown estimator"):
            lower("", "", dd, cls("v", "l_quantity", "l_tax", "biased"))


@pytest.mark.parametrize("fn", ["corr", "covar_samp", "covar_pop"])
def test_sql_is_one_pushed_query(session, fn):
    s, _ = session
    q = f"select o_orderkey, {fn}(l_quantity, l_extendedprice), avg(l_quantity), count(*) " \
        "from %s where o_orderkey < 400 group by o_orderkey"
    d = s.sql(q % T)
    specs = d.druid_query_specs()
    assert len(specs) == 1, d.explain()
    cls = S.CorrelationAggregationSpec if fn == "corr" else S.CovarianceAggregationSpec
    assert sum(isinstance(a, cls) for a in specs[0].aggregations) == 1
    got, want = (sorted(x.collect()) for x in (d, s.sql(q % (T + "Base"))))
    assert len(got) == len(want) > 50
    nulls = 0
    for g, w in zip(got, want):
        assert g[0] == w[0] and g[2:] == w[2:]
        nulls += g[1] is None
        # (both sides are float64 two-pass formulas over at most 7 rows: a few ulp apart)
        assert (g[1] is None and w[1] is None) or math.isclose(g[1], w[1], rel_tol=1e-12, abs_tol=0.0), (g, w)
        assert g[3] > 1 or (g[1] == 0.0 if fn == "covar_pop" else g[1] is None)  # one-row orders
    assert (nulls > 0) == (fn != "covar_pop")


def test_sql_global_distinct_and_window(session):
    s, _ = session
    (r, c, n), = s.sql(f"select corr(l_quantity, l_extendedprice), covar_pop(l_quantity, l_quantity), "
                       f"count(*) from {T}Base").collect()
    (v,), = s.sql(f"select var_pop(l_quantity) from {T}Base").collect()
    assert 0.0 < r < 1.0 and math.isclose(c, v, rel_tol=1e-12) and n > 1000
    for bad in ("corr(distinct l_quantity, l_tax)", "covar_samp(l_quantity)",
                "corr(l_quantity, l_tax) over (partition by o_orderkey)"):
        with pytest.raises(AnalysisError):
            s.sql(f"select {bad} from {T}Base").collect()
