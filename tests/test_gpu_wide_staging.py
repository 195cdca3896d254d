"""8-byte columns staged through LDS-DMA planes (sdo_device.h dma_b<3>): both dwords of every lane."""
import numpy as np
import pytest
import torch

from spark_druid_olap_amd.engine import device_exec as DE
from spark_druid_olap_amd.engine.columns import materialize
from spark_druid_olap_amd.engine.executor import Engine
from spark_druid_olap_amd.query import spec as S
from spark_druid_olap_amd.segment.datasource import make_datasource
from spark_druid_olap_amd.segment.dictionary import Dictionary

N = 2 * 4096 + 37


@pytest.mark.gpu
@pytest.mark.parametrize("stage", ["lds", "reg"])
def test_min_max_of_8_byte_columns(stage, monkeypatch):
    monkeypatch.setattr(DE, "JIT_STAGE", stage)
    rng = np.random.default_rng(11)
    wide = rng.integers(-(1 << 62), 1 << 62, N)   # every high dword differs from its neighbours'
    dbl = rng.choice([-1.0, 1.0], N) * 10.0 ** rng.uniform(-3, 12, N)
    g = rng.integers(0, 5, N)
    names = np.asarray([f"k{i}" for i in range(5)], dtype=object)
    dic, codes = Dictionary.build(names[g])
    days = torch.from_numpy(18262 + (np.arange(N) * 40) // N)
    ds = make_datasource("w8", N, days, 86400000, {"g": torch.from_numpy(np.asarray(codes, dtype=np.int64))},
                         {"g": dic}, {"wide": torch.from_numpy(wide), "dbl": torch.from_numpy(dbl)},
                         {"wide": "long", "dbl": "double"}).to("cuda")
    q = S.GroupByQuerySpec("w8", [S.DefaultDimensionSpec("g")],
                           aggregations=[S.FunctionAggregationSpec("longMin", "wmin", "wide"),
                                         S.FunctionAggregationSpec("longMax", "wmax", "wide"),
                                         S.FunctionAggregationSpec("doubleMin", "dmin", "dbl"),
                                         S.FunctionAggregationSpec("doubleMax", "dmax", "dbl")],
                           intervals=["2019-01-01/2021-01-01"])
    r = Engine().execute(q, ds)
    keys = materialize(r.data["g"]).tolist()
    assert sorted(keys) == sorted(names.tolist())
    for i, k in enumerate(keys):
        m = names[g] == k
        got = (int(r.data["wmin"][i]), int(r.data["wmax"][i]), float(r.data["dmin"][i]), float(r.data["dmax"][i]))
        assert got == (wide[m].min(), wide[m].max(), dbl[m].min(), dbl[m].max()), k
