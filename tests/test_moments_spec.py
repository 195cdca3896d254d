"""The variance aggregator and the stddev post-aggregator off the GPU: JSON, the lowering's
refusals, and the SQL variance family of a CPU session as one pushed query (the float64 two-pass
fallback answers there)."""
import math

import pytest

from spark_druid_olap_amd.engine.executor import Engine
from spark_druid_olap_amd.engine.lower import LoweringError
from spark_druid_olap_amd.models import tpch
from spark_druid_olap_amd.query import spec as S
from spark_druid_olap_amd.session import Session

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


@pytest.mark.parametrize("spec, kind", [(S.VarianceAggregationSpec("v", "l_quantity"), "aggregation"),
                                        (S.VarianceAggregationSpec("v", "l_quantity", "population"), "aggregation"),
                                        (S.StddevPostAggregationSpec("s", "v"), "postagg")])
def test_json_round_trip(spec, kind):
    j = spec.to_json()
    assert j["type"] == ("variance" if kind == "aggregation" else "stddev") and j["fieldName"] == spec.fieldName
    assert S.from_json(j, kind) == spec
    assert S.from_json({"type": "variance", "name": "v", "fieldName": "x"}, "aggregation").estimator == "sample"


def test_refusals(session):
    _, ds = session
    import copy

    from spark_druid_olap_amd.segment.datasource import MetricColumn

    def lower(col, d, **kw):
        q = S.GroupByQuerySpec(d.name, [], aggregations=[S.VarianceAggregationSpec("v", col)], intervals=IV)
        return Engine(use_native=False, **kw).prepare(q, d)

    dd = copy.copy(ds)
    m = ds.metrics["l_quantity"]
    dd.metrics = dict(ds.metrics, dbl=MetricColumn("dbl", "double", m.data.double()),
                      sk=MetricColumn("sk", "hll", m.data, sketch=object()))
    lower("dbl", dd)  # (a double metric lowers ...)
    with pytest.raises(LoweringError, match="not bitwise reproducible"):
        lower("dbl", dd, deterministic=True)  # ... but not in deterministic mode
    lower("l_quantity", dd, deterministic=True)  # (integer sums are reproducible)
    with pytest.raises(LoweringError, match="sketch metric"):
        lower("sk", dd)
    with pytest.raises(LoweringError, match="not a metric"):
        lower("l_shipmode", dd)


@pytest.mark.parametrize("fn", ["stddev", "stddev_samp", "stddev_pop", "variance", "var_samp", "var_pop"])
def test_sql_family_is_one_pushed_query(session, fn):
    s, _ = session
    q = f"select o_orderkey, {fn}(l_extendedprice), {fn}(l_quantity), avg(l_quantity), median(l_tax), count(*) " \
        "from %s where o_orderkey < 400 group by o_orderkey"
    d = s.sql(q % T)
    specs = d.druid_query_specs()
    assert len(specs) == 1, d.explain()
    assert sum(isinstance(a, S.VarianceAggregationSpec) for a in specs[0].aggregations) == 2
    got, want = (sorted(x.collect()) for x in (d, s.sql(q % (T + "Base"))))
    assert len(got) == len(want) > 50
    nulls = 0
    for g, w in zip(got, want):
        assert g[0] == w[0] and g[3:] == w[3:]
        for a, b in zip(g[1:3], w[1:3]):
            nulls += a is None
            # (both sides are float64 two-pass formulas over at most 7 rows: a few ulp apart)
            assert (a is None and b is None) or math.isclose(a, b, rel_tol=1e-12, abs_tol=0.0)
    # one-row orders: NULL under the sample estimators, 0 under the population ones
    assert (nulls > 0) == (not fn.endswith("_pop"))
