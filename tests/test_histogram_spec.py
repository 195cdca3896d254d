"""The fixedBucketsHistogram aggregator off the GPU: JSON, the thresholds against a Fraction loop, the
lowering's refusals, and SQL histogram() of a CPU session as one pushed query (torch counts against
the same thresholds there) against the same statement over the base table."""
import copy
import math
from fractions import Fraction

import numpy as np
import pytest

from spark_druid_olap_amd.engine.executor import Engine
from spark_druid_olap_amd.engine.lower import LoweringError
from spark_druid_olap_amd.models import tpch
from spark_druid_olap_amd.ops import buckets
from spark_druid_olap_amd.query import spec as S
from spark_druid_olap_amd.segment.datasource import MetricColumn
from spark_druid_olap_amd.session import Session
from spark_druid_olap_amd.sql.analyzer import AnalysisError

T = "orderLineItemPartSupplier"
IV = ["1990-01-01/2000-01-01"]
H = S.FixedBucketsHistogramAggregationSpec


@pytest.fixture(scope="module")
def session():
    f = tpch.generate_flat(0.002, "cpu")
    ds, df = tpch.to_datasource(f, profile="bench"), tpch.to_pandas(f)
    s = Session(engine=Engine(use_native=False))
    s.register_datasource(ds)
    s.register_table(T + "Base", df, schema=tpch.FLAT_SCHEMA)
    s.sql(tpch.druid_ddl(with_column_mapping=False))
    return s, ds, df


@pytest.mark.parametrize("spec", [H("h", "l_extendedprice", 20, 0, 100000.5, "overflow"),
                                  H("h", "l_quantity", breaks=[-1.5, 0, 7, 50])])
def test_json_round_trip(spec):
    j = spec.to_json()
    assert j["type"] == "fixedBucketsHistogram" and j["jsonClass"] == "FixedBucketsHistogramAggregationSpec"
    assert S.from_json(j, "aggregation") == spec
    plain = {k: v for k, v in j.items() if k not in ("jsonClass", "outlierHandlingMode")}
    assert S.from_json(plain, "aggregation") == spec.copy(outlierHandlingMode="ignore")


# (limits, stored values of a long column / values of a decimal(2) and a double column)
ZEROS = [-1.0, -0.01, -0.0, 0.0, 0.01, 1.0]
CASES = {
    "tenths": (dict(lower=0, upper=1, num_buckets=10), [-1, 0, 1, 2], [i / 100 for i in range(-5, 106)] + [0.1, 0.3, 0.7]),
    "edge_at_zero": (dict(breaks=[-1, 0, 1]), [-2, -1, 0, 1, 2], ZEROS),
    "narrow": (dict(lower=-1, upper=1, num_buckets=8), [-2, -1, 0, 1, 2], ZEROS + [0.25, 0.24, -0.25, -0.26, 0.99]),
    "at_limits": (dict(lower=-2.5, upper=7.5, num_buckets=4), [-3, -2, 7, 8], [-2.5, -2.51, 7.5, 7.49, 2.5, math.nan]),
}


@pytest.mark.parametrize("kind", ["long", "decimal", "double"])
@pytest.mark.parametrize("case", list(CASES))
def test_thresholds_against_a_fraction_loop(case, kind):
    kw, longs, reals = CASES[case]
    edges = buckets.bucket_edges(**kw)
    thr = buckets.bucket_thresholds(edges, kind, 2)
    assert thr.dtype == np.uint64 and len(thr) == len(edges) and np.all(thr[1:] >= thr[:-1])
    if kind == "double":
        stored = np.asarray(reals, dtype=np.float64)
        value = [None if math.isnan(v) else Fraction(v) for v in stored.tolist()]
    else:
        stored = np.asarray(longs if kind == "long" else [round(v * 100) for v in reals if v == v], dtype=np.int64)
        value = [Fraction(v, 1 if kind == "long" else 100) for v in stored.tolist()]
    want = [len(edges) if v is None else sum(e <= v for e in edges) for v in value]  # (NaN: above)
    assert buckets.slots(stored, thr, kind).tolist() == want
    if case == "narrow" and kind == "long":
        assert len(set(thr.tolist())) < len(thr)  # buckets narrower than 1: equal thresholds, empty buckets
    if case == "edge_at_zero" and kind == "double":
        assert want[2] == want[3] == 2  # -0.0 and +0.0 both reach the edge at zero


def test_overflow_mode_folds_the_outliers():
    c = np.asarray([[3, 1, 2, 4, 5], [0, 0, 0, 0, 7]])
    assert buckets.apply_mode(c, "overflow").tolist() == [[0, 4, 2, 9, 0], [0, 0, 0, 7, 0]]
    assert buckets.apply_mode(c, "ignore") is c


BAD = [(dict(numBuckets=5, lowerLimit=1, upperLimit=1), "lowerLimit < upperLimit"),
       (dict(numBuckets=0, lowerLimit=0, upperLimit=1), "numBuckets >= 1"),
       (dict(numBuckets=1023, lowerLimit=0, upperLimit=1), "at most 1022"),
       (dict(breaks=[0, 1, 1]), "strictly ascending"),
       (dict(breaks=[3]), "strictly ascending"),
       (dict(numBuckets=5, lowerLimit=0, upperLimit=1, outlierHandlingMode="clip"), "outlierHandlingMode"),
       (dict(numBuckets=5, lowerLimit=0, upperLimit=1, fieldName="sk"), "sketch metric"),
       (dict(numBuckets=5, lowerLimit=0, upperLimit=1, fieldName="l_shipmode"), "not a metric")]


@pytest.mark.parametrize("kw,msg", BAD, ids=[m for _, m in BAD])
def test_refusals(session, kw, msg):
    _, ds, _ = session
    dd = copy.copy(ds)
    dd.metrics = dict(ds.metrics, sk=MetricColumn("sk", "hll", ds.metrics["l_quantity"].data, sketch=object()))
    kw = dict({"fieldName": "l_quantity"}, **kw)
    with pytest.raises(LoweringError, match=msg):
        Engine(use_native=False).prepare(S.GroupByQuerySpec(dd.name, [], aggregations=[H("h", **kw)], intervals=IV), dd)


def test_refusals_of_context(session):
    _, ds, _ = session
    h = H("h", "l_quantity", 5, 0, 50)

    def prepare(eng, **kw):
        return eng.prepare(S.GroupByQuerySpec(ds.name, [], aggregations=kw.pop("aggs", [h]), intervals=IV, **kw), ds)

    assert prepare(Engine(use_native=False, deterministic=True))._full_prog.histograms[0][:2] == ("h", "l_quantity")
    with pytest.raises(LoweringError, match="filtered"):
        prepare(Engine(use_native=False), aggs=[S.FilteredAggregationSpec(S.SelectorFilterSpec("l_shipmode", "AIR"), h)])
    with pytest.raises(LoweringError, match="one count per bucket"):
        prepare(Engine(use_native=False), having=S.ComparisonHavingSpec("greaterThan", "h", 1))

    class TwoRanks:  # (only what lowering reads of a world: every rank would answer for its own shard)
        distributed, size, rank = True, 2, 0

    eng = Engine(use_native=False)
    eng.world = TwoRanks()
    with pytest.raises(LoweringError, match="across ranks"):
        prepare(eng)


def test_sql_is_one_pushed_query(session):
    s, _, df = session
    q = "select l_returnflag, histogram(l_extendedprice, 0, 100000, 20), count(*), " \
        "histogram(l_quantity, array(0, 10.5, 25, 50)) from %s group by l_returnflag"
    d = s.sql(q % T)
    specs = d.druid_query_specs()
    assert len(specs) == 1, d.explain()
    hs = [a for a in specs[0].aggregations if isinstance(a, H)]
    assert [(a.fieldName, a.numBuckets, a.breaks) for a in hs] == [("l_extendedprice", 20, None),
                                                                   ("l_quantity", None, [0, 10.5, 25, 50])]
    got, want = (sorted(x.collect()) for x in (d, s.sql(q % (T + "Base"))))
    assert got == want and len(got) == 3
    for flag, h, n, h2 in got:
        assert len(h) == 22 and sum(h) == n == sum(h2) == int((df.l_returnflag == flag).sum())
        sub = df.l_extendedprice[df.l_returnflag == flag]
        assert h[1:-1] == np.histogram(sub, 20, (0, 100000))[0].tolist()


@pytest.mark.parametrize("bad", ["histogram(distinct l_quantity, 0, 50, 5)", "histogram(l_quantity, 0, l_tax, 5)",
                                 "histogram(l_quantity, 0, 50, 2.5)", "histogram(l_quantity, 0, 50, 0)",
                                 "histogram(l_quantity, 50, 50, 5)", "histogram(l_quantity, array(1))",
                                 "histogram(l_quantity, array(1, 3, 2))", "histogram(l_quantity, 0, 50)",
                                 "histogram(l_quantity, 0, 50, 5) over (partition by o_orderkey)"])
def test_sql_analysis_errors(session, bad):
    s, _, _ = session
    with pytest.raises(AnalysisError):
        s.sql(f"select {bad} from {T}Base").collect()
