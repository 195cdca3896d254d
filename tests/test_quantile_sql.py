"""percentile / median / percentile_approx through SQL and the Druid query spec, against numpy."""
import math

import numpy as np
import pytest
import torch

from spark_druid_olap_amd.engine.executor import Engine
from spark_druid_olap_amd.engine.lower import LoweringError
from spark_druid_olap_amd.models import tpch
from spark_druid_olap_amd.query import spec as S
from spark_druid_olap_amd.session import Session
from spark_druid_olap_amd.sql.types import AnalysisError

T = "orderLineItemPartSupplier"
Q = ("select l_returnflag, median(l_quantity), percentile(l_extendedprice, array(0.1, 0.9)), "
     f"percentile_approx(l_discount, 0.95) from {T} where l_shipmode = 'AIR' group by l_returnflag")


@pytest.fixture(scope="module")
def flat():
    f = tpch.generate_flat(0.002, "cpu")
    return tpch.to_datasource(f, profile="bench"), tpch.to_pandas(f)


def _session(ds, df, native):
    s = Session(engine=Engine(use_native=native))
    s.register_datasource(ds)
    s.register_table(T + "Base", df, schema=tpch.FLAT_SCHEMA)
    s.sql(tpch.druid_ddl(with_column_mapping=False))
    return s


def _check(s, df, q=Q):
    d = s.sql(q)
    assert len(d.druid_queries()) == 1, d.explain()  # pushed, not a base-table scan
    rows = {r[0]: r[1:] for r in d.collect()}
    air = df[df.l_shipmode == "AIR"]
    assert set(rows) == set(air.l_returnflag)
    for flag, g in air.groupby("l_returnflag"):
        med, pr, ap = rows[flag]
        disc = np.sort(g.l_discount.to_numpy(dtype=np.float64))
        assert med == pytest.approx(np.quantile(g.l_quantity.to_numpy(dtype=np.float64), 0.5), rel=1e-12)
        assert list(pr) == pytest.approx(list(np.quantile(g.l_extendedprice.to_numpy(dtype=np.float64), [0.1, 0.9])),
                                         rel=1e-12)
        assert ap == disc[max(0, math.ceil(0.95 * len(disc)) - 1)]
    return rows


def test_percentiles_pushed_match_numpy(flat):
    ds, df = flat
    s = _session(ds, df, False)
    rows = _check(s, df)
    assert _check(s, df, Q.replace("percentile_approx(", "approx_percentile(")) == rows


@pytest.mark.gpu
def test_percentiles_pushed_match_numpy_gpu(flat):
    ds, df = flat
    _check(_session(ds.to("cuda"), df, True), df)


def test_quantiles_spec_json_round_trip():
    a = S.QuantilesAggregationSpec("p", "l_quantity", [0.25, 0.5], False)
    j = a.to_json()
    assert j["type"] == "quantiles" and j["fractions"] == [0.25, 0.5] and j["interpolate"] is False
    assert S.from_json(j, "aggregation") == a


def test_percentage_out_of_range_is_rejected(flat):
    s = _session(*flat, False)
    with pytest.raises(AnalysisError):
        s.sql(f"select percentile(l_quantity, 1.5) from {T}")


def test_quantiles_over_a_long_dimension():
    from spark_druid_olap_amd.segment.datasource import make_datasource
    from spark_druid_olap_amd.segment.dictionary import LONG, Dictionary

    rng = np.random.default_rng(3)
    v = rng.integers(-500, 500, 1000)
    dic, codes = Dictionary.build(v, LONG)
    ds = make_datasource("d", len(v), torch.from_numpy(18262 + np.arange(len(v)) // 100), 86400000,
                         {"v": torch.from_numpy(np.asarray(codes, dtype=np.int64))}, {"v": dic}, {}, {})
    q = S.GroupByQuerySpec("d", [], aggregations=[S.QuantilesAggregationSpec("p", "v", [0.1, 0.5, 1], True)],
                           intervals=["2019-01-01/2021-01-01"])
    r = Engine(use_native=False).execute(q, ds)
    np.testing.assert_allclose(r.data["p"][0], np.quantile(v.astype(np.float64), [0.1, 0.5, 1]), rtol=1e-12, atol=0)


def test_quantiles_refused_where_they_would_be_wrong(flat):
    ds, _ = flat
    agg = S.QuantilesAggregationSpec("p", "l_quantity", [0.5], True)
    dims = [S.DefaultDimensionSpec("l_returnflag")]
    iv = ["1992-01-01/1999-01-01"]
    eng = Engine(use_native=False)
    with pytest.raises(LoweringError, match="one value per fraction"):
        eng.prepare(S.GroupByQuerySpec("tpch", dims, aggregations=[agg], intervals=iv,
                                       having=S.ComparisonHavingSpec("greaterThan", "p", 1.0)), ds)

    class TwoRanks:  # (only what lowering reads of a world: every rank would select over its own shard)
        distributed, size, rank = True, 2, 0

    eng.world = TwoRanks()
    with pytest.raises(LoweringError, match="across ranks"):
        eng.prepare(S.GroupByQuerySpec("tpch", dims, aggregations=[agg], intervals=iv), ds)
