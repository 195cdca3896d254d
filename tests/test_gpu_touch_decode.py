"""GPU: first-touch gather + sparse decode in one kernel (post_scan.hip touch_decode_kernel).

* the fused kernel against ``touch_compact`` + ``sparse_decode`` on synthetic tables: byte-equal
  columns for every column kind and output width, the table re-initialised, the bytes cleared;
* the Q3-shaped statement with ``FUSED_TOUCH_DECODE`` on and off: re-runs on buffers the previous
  run re-initialised, and re-runs over a deferred state that was dropped or is still held;
* statements that read the groups on the device (HAVING, ORDER BY aggregate LIMIT) unchanged.
"""
import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = 2 * 65536 + 70  # three 65536-group blocks, the last one a partial mask word
_W = {0: 2, 1: 4, 2: 8, 3: 8, 4: 8, 5: 8}


def _marks(name):
    m = torch.zeros(ROWS, dtype=torch.bool)
    if name == "one":
        m[0] = True
    elif name == "edge":
        m[65535] = m[65536] = True
    elif name == "last":
        m[ROWS - 1] = True
    elif name == "middle":
        m[65536:131072] = True
    elif name == "random":
        m = torch.rand(ROWS, generator=torch.Generator().manual_seed(11)) < 0.01
    return m.cuda()


@pytest.fixture(scope="module")
def tables():
    g = torch.Generator().manual_seed(5)
    orig = torch.randint(0, 300, (500,), generator=g, dtype=torch.int64).cuda()
    lut = torch.randint(-(1 << 30), 1 << 30, (300,), generator=g, dtype=torch.int32).cuda()
    # slot values: ordered-int encodings of doubles (what a float min slot holds; the integer and
    # raw-bit columns read the same words)
    bits = ((torch.rand(ROWS, 3, generator=g, dtype=torch.float64) - 0.5) * 2e6).view(torch.int64)
    vals = torch.where(bits >= 0, bits, bits ^ 0x7FFFFFFFFFFFFFFF).cuda()
    return orig, lut, vals


def _cols(ns, orig, lut):
    s1, s2 = (1, 2) if ns == 3 else (0, 0)
    return [
        (0, 0, 0, 0, 7, 1000, 0, 0, 0, 0.0),                               # key, int16
        (0, 1, 0, 0, 3, 50000, 0, 0, 0, 0.0),                              # key, int32
        (0, 2, 0, 0, 1, 1 << 40, 0, 0, 0, 0.0),                            # key, int64
        (0, 1, 1, 0, 11, 500, 0, orig.data_ptr(), lut.data_ptr(), 0.0),    # key -> orig -> int32 table
        (0, 2, 0, 0, 1, 1 << 40, 12345, 0, 0, 0.0),                        # range dictionary: start + id
        (1, 2, 0, 0, 1, 1, 0, 0, 0, 0.0),                                  # count
        (1, 3, 0, s1, 1, 1, 0, 0, 0, 100.0),                               # integer sum / 10^2
        (3, 4, 0, s2, 1, 1, 0, 0, 0, 0.0),                                 # f64 sum (raw bits)
        (2, 4, 0, s1, 1, 1, 0, 0, 0, 0.0),                                 # float min
        (2, 5, 0, s2, 1, 1, 0, 0, 0, 0.0),                                 # float min as long
        (4, 2, 0, 0, 1, 1, 0, 0, 0, 0.0),                                  # group id
    ]


@pytest.mark.parametrize("marks", ["none", "one", "edge", "last", "middle", "random"])
@pytest.mark.parametrize("ns", [1, 3])
def test_fused_kernel_matches_gather_then_decode(tables, ns, marks):
    from spark_druid_olap_amd.ops import native

    orig, lut, vals = tables
    sel = _marks(marks)
    ref_idx = torch.nonzero(sel).flatten()
    R = int(ref_idx.numel())
    init = torch.tensor([0, 1 << 62, -(1 << 62)][:ns], dtype=torch.int64, device="cuda")
    specs = _cols(ns, orig, lut)
    offs, off = [], 0
    for sp in specs:
        offs.append(off)
        off = (off + R * _W[sp[1]] + 15) // 16 * 16
    nbytes = off
    cols = [sp + (o,) for sp, o in zip(specs, offs)]
    hosts = []
    for fused in (False, True):
        acc = init.expand(ROWS, ns).clone()
        acc[ref_idx] = vals[ref_idx, :ns]
        touch = torch.zeros((ROWS + 63) // 64 * 64, dtype=torch.uint8, device="cuda")
        touch[:ROWS][sel] = 1
        host = torch.zeros(max(nbytes, 16), dtype=torch.uint8, pin_memory=True)
        if fused:
            c = native.touch_count(touch, acc, init)
            assert c.n == R
            native.touch_decode(c, cols, nbytes, host)
        else:
            idx, rows = native.touch_compact(touch, acc, init)
            assert torch.equal(idx, ref_idx)
            dev = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
            native.load().sparse_decode(idx.data_ptr(), rows.data_ptr(), R, ns, cols, dev.data_ptr(), nbytes,
                                        host.data_ptr(), native._stream(acc.device))
        assert torch.equal(acc, init.expand(ROWS, ns)), "rows not re-initialised"
        assert int(touch.sum()) == 0
        hosts.append(host.numpy().copy())
    for sp, o in zip(specs, offs):
        a, b = (h[o: o + R * _W[sp[1]]] for h in hosts)
        assert a.tobytes() == b.tobytes(), sp
    gid = hosts[1][offs[-1]: offs[-1] + R * 8].view(np.int64)
    assert gid.tolist() == ref_idx.tolist()  # ascending group ids, whatever the two kernels agree on


# ------------------------------------------------------------------------------------------------
T = "orderLineItemPartSupplier"
Q3_WHERE = f"""from {T} where c_mktsegment = 'BUILDING'
    and dateIsBefore(dateTime(`o_orderdate`), dateTime("1995-03-15"))
    and dateIsAfter(dateTime(`l_shipdate`), dateTime("1995-03-15"))"""
Q3_HAVING = f"""select o_orderkey, sum(l_extendedprice) as price, o_orderdate, o_shippriority {Q3_WHERE}
    group by o_orderkey, o_orderdate, o_shippriority having sum(l_extendedprice) > 250000"""
Q3_TOPK = f"""select o_orderkey, sum(l_extendedprice) as price, o_orderdate, o_shippriority {Q3_WHERE}
    group by o_orderkey, o_orderdate, o_shippriority order by price desc, o_orderkey limit 10"""


@pytest.fixture(scope="module")
def ds():
    from spark_druid_olap_amd.models import tpch

    return tpch.to_datasource(tpch.generate_flat(0.05, "cuda"), profile="bench")


def _session(ds, monkeypatch, fused):
    """A fresh session (its own prepared scans) whose large group-bys take the first-touch table."""
    from spark_druid_olap_amd.engine import partials as P
    from spark_druid_olap_amd.engine.executor import Engine
    from spark_druid_olap_amd.models import tpch
    from spark_druid_olap_amd.planner import cost
    from spark_druid_olap_amd.session import Session

    monkeypatch.setattr(cost, "TOUCH_MIN_G", 0)
    monkeypatch.setattr(P, "FUSED_TOUCH_DECODE", fused)
    s = Session(engine=Engine(), conf={"spark.sparklinedata.druid.approxCountDistinct": "true"})
    s.register_datasource(ds)
    s.register_table("orderLineItemPartSupplierBase", schema=tpch.FLAT_SCHEMA)
    s.sql(tpch.druid_ddl(source="orderLineItemPartSupplierBase", datasource="tpch", with_column_mapping=False))
    return s


def _touch_scan(d):
    scans = [p for dq in d.druid_queries() for _, _, p in dq._prepared.scans if p is not None and p.touch]
    assert scans, "the statement did not run with a first-touch table"
    return scans[0]


def _same(a, b):
    assert list(a.columns) == list(b.columns) and len(a) == len(b)
    for c in a.columns:
        assert a[c].dtype == b[c].dtype, c
        assert a[c].tolist() == b[c].tolist(), c


@pytest.fixture()
def fused_calls(monkeypatch):
    from spark_druid_olap_amd.ops import native

    calls, real = [], native.touch_decode

    def spy(c, *a, **k):
        calls.append(c.n)
        return real(c, *a, **k)

    monkeypatch.setattr(native, "touch_decode", spy)
    return calls


@pytest.fixture(scope="module")
def q3():
    from spark_druid_olap_amd.models import tpch

    return dict(tpch.BENCH_QUERIES)["TPCH Q3"]


@pytest.fixture()
def q3_unfused(ds, q3, monkeypatch):
    d = _session(ds, monkeypatch, False).sql(q3)
    ref = d.to_pandas()
    assert len(ref) > 100
    _touch_scan(d)
    return ref


def test_q3_fused_equals_unfused_across_reruns(ds, q3, q3_unfused, fused_calls, monkeypatch):
    assert not fused_calls
    d = _session(ds, monkeypatch, True).sql(q3)
    for _ in range(2):  # the second run scans into the rows the first one re-initialised
        _same(d.to_pandas(), q3_unfused)
    assert fused_calls == [len(q3_unfused)] * 2
    b = _touch_scan(d)._slots[0]
    assert b.clean and b.pending is None


def test_q3_rerun_over_a_dropped_or_held_deferred_state(ds, q3, q3_unfused, fused_calls, monkeypatch):
    d = _session(ds, monkeypatch, True).sql(q3)
    _same(d.to_pandas(), q3_unfused)
    prep = _touch_scan(d)
    sp = prep.run()
    assert sp.pending and sp.rows == len(q3_unfused) and not prep._slots[0].clean
    del sp  # dropped unconsumed: its marks and rows are still in the table
    _same(d.to_pandas(), q3_unfused)
    held = prep.run()
    _same(d.to_pandas(), q3_unfused)  # the re-run gathers the state somebody still holds first
    assert not held.pending and held.keys.numel() == len(q3_unfused) == held.rows
    assert sorted(held.keys.tolist()) == held.keys.tolist()
    _same(d.to_pandas(), q3_unfused)


@pytest.mark.parametrize("sql", [Q3_HAVING, Q3_TOPK])
def test_device_consumers_materialise_the_groups(ds, sql, fused_calls, monkeypatch):
    ref = _session(ds, monkeypatch, False).sql(sql).to_pandas()
    d = _session(ds, monkeypatch, True).sql(sql)
    for _ in range(2):
        _same(d.to_pandas(), ref)
    assert 0 < len(ref) < 5000
    pd.testing.assert_frame_equal(d.to_pandas(), ref)
