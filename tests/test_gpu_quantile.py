"""Exact per-group percentiles on the device (ops/csrc/quantile.hip through PreparedQuantile)
against plain numpy over the host columns."""
import math

import numpy as np
import pytest
import torch

from spark_druid_olap_amd.engine.columns import materialize
from spark_druid_olap_amd.engine.device_exec import PreparedQuantile
from spark_druid_olap_amd.engine.executor import Engine
from spark_druid_olap_amd.query import spec as S
from spark_druid_olap_amd.segment.datasource import make_datasource
from spark_druid_olap_amd.segment.dictionary import Dictionary

pytestmark = pytest.mark.gpu

N = 3 * 4096 + 37  # three chunk regions and a ragged fourth
FR = [0, 0.25, 0.5, 0.999, 1]
DAY = 86400000


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(7)
    keep = rng.random(N) < 0.5
    g7 = rng.choice(np.arange(4, 7), size=N, p=[0.7, 0.25, 0.05])
    g7[100], g7[[200, 9000]] = 0, 1            # one group of 1 row, one of 2
    g7[rng.choice(np.arange(300, 8000), 40, replace=False)] = 2   # constant values (below)
    g7[rng.choice(np.arange(8001, 8999), 30, replace=False)] = 3  # every row filtered out
    keep[[100, 200, 9000]] = True
    keep[g7 == 3] = False
    cols = {"q": rng.integers(1, 51, N), "price": rng.integers(0, 1 << 20, N),
            "wide": rng.integers(-(1 << 62), 1 << 62, N),
            "dbl": np.where(rng.random(N) < 0.05, 0.0, rng.choice([-1.0, 1.0], N) * 10.0 ** rng.uniform(-3, 12, N))}
    for c in cols.values():
        c[g7 == 2] = c[0]
    ids = {"flt": np.where(keep, 0, 1), "g7": g7, "g5k": rng.permutation(N) % 5000}
    names = {"flt": ["a", "b"], "g7": [f"k{i}" for i in range(7)], "g5k": [f"v{i:04d}" for i in range(5000)]}
    dicts, dim_ids = {}, {}
    for k, v in ids.items():
        dicts[k], codes = Dictionary.build(np.asarray(names[k], dtype=object)[v])
        dim_ids[k] = torch.from_numpy(np.asarray(codes, dtype=np.int64))
    days = torch.from_numpy(18262 + (np.arange(N) * 70) // N)  # 2020-01-01 .. early March
    ds = make_datasource("qt", N, days, DAY, dim_ids, dicts, {k: torch.from_numpy(v) for k, v in cols.items()},
                         {"q": "long", "price": "decimal", "wide": "long", "dbl": "double"}, {"price": 2})
    host = dict(cols, price=cols["price"] / 100.0)
    return ds.to("cuda"), host, keep, {k: np.asarray(names[k], dtype=object)[v] for k, v in ids.items()}


@pytest.mark.parametrize("dim", [None, "g7", "g5k"])
@pytest.mark.parametrize("col", ["q", "price", "wide", "dbl"])
def test_quantiles_match_numpy(data, col, dim):
    ds, host, keep, keys = data
    q = S.GroupByQuerySpec("qt", [S.DefaultDimensionSpec(dim)] if dim else [], filter=S.SelectorFilterSpec("flt", "a"),
                           aggregations=[S.QuantilesAggregationSpec("p", col, FR, True),
                                         S.QuantilesAggregationSpec("e", col, FR, False)],
                           intervals=["2019-01-01/2021-01-01"])
    pq = Engine().prepare(q, ds)
    r = pq.run()
    qp = pq.__dict__.get("_quantile_prep")
    assert isinstance(qp, PreparedQuantile) and len(qp.plan) == 2  # the HIP select answered, not torch
    print(col, dim, "groups", r.num_rows, "(W, B, levels)", qp.plan)
    got = materialize(r.data[dim]).tolist() if dim else [None]
    v, k = host[col][keep], (keys[dim][keep] if dim else np.full(int(keep.sum()), None))
    want = sorted(set(k.tolist()), key=str)
    assert sorted(got, key=str) == want
    for g, p, e in zip(got, np.asarray(r.data["p"]), np.asarray(r.data["e"])):
        vg = v[k == g] if dim else v
        s = np.sort(vg)
        exact = np.array([s[max(0, math.ceil(f * len(s)) - 1)] for f in FR])
        assert e.dtype == exact.dtype and (e == exact).all(), (g, e, exact)
        # (np.quantile(v, p) is np.percentile(v, 100 p) with the fraction passed unchanged:
        # 100 * 0.999 / 100 is 0.9990000000000001, which moves a result near zero by more than 1e-12)
        np.testing.assert_allclose(p, np.quantile(vg.astype(np.float64), FR, method="linear"), rtol=1e-12, atol=0)
