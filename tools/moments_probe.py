"""stddev / variance pushed down as per-group moment sums, against avg and median of the same column.

Over flattened TPC-H on one GPU, SQL end to end in one process, every statement is the median of 7
runs after 3 warm-ups, host clock around collect().  Per column: the variance-family call, ``avg``
and ``median`` of the same column by the same groups (avg is one fused scan; median is the producer
pass, a stats pass and the select passes; stddev is the producer pass and ONE pass over the
records).  For each pushed variance statement the accumulation pass alone is also timed with device
events against ``qsel_stats`` over the same records (both read every record once).  The flat schema
has no double metric, so the two-pass double path is not measured here.  The table goes to
profiles/moments_probe.json.

    python tools/moments_probe.py [--sf 100] [--out profiles/moments_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spark_druid_olap_amd.engine.device_exec import PART_POOL  # noqa: E402
from spark_druid_olap_amd.engine.executor import Engine  # noqa: E402
from spark_druid_olap_amd.models import tpch  # noqa: E402
from spark_druid_olap_amd.ops import native  # noqa: E402
from spark_druid_olap_amd.session import Session  # noqa: E402

T = "orderLineItemPartSupplier"
# (name, variance call, column, grouping)
SHAPES = [
    ("stddev_quantity_by_returnflag", "stddev", "l_quantity", "l_returnflag"),
    ("stddev_extendedprice_by_returnflag", "stddev", "l_extendedprice", "l_returnflag"),
    ("var_pop_extendedprice_by_returnflag", "var_pop", "l_extendedprice", "l_returnflag"),
    ("stddev_extendedprice_by_brand_type", "stddev", "l_extendedprice", "p_brand, p_type"),
]


def timed(df, runs: int = 7, warm: int = 3):
    for _ in range(warm):
        rows = df.collect()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        rows = df.collect()
        ts.append((time.perf_counter() - t0) * 1e3)
    return rows, {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def device_ms(fn, runs: int = 7, warm: int = 3) -> float:
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return round(statistics.median(ts), 3)


def passes_alone(mp) -> dict:
    """The first column's accumulation pass and qsel_stats over the same produced records."""
    nat, st = native.load(), native._stream(mp.dev)
    dev, G = mp.dev, mp.G
    i32, i64 = torch.int32, torch.int64
    pend = torch.empty(max(1, mp.nch), dtype=i32, device=dev)
    slab = PART_POOL.acquire(dev, mp.words)
    try:
        regions = mp.produce(nat, st, slab, pend)
        voff, mode, _ = next(iter(mp.passes.values()))
        state = torch.empty(G * 6, dtype=i64, device=dev)
        cnt, width, wmax = (torch.empty(n, dtype=i32, device=dev) for n in (G, G, 1))
        mn, mx = torch.empty(G, dtype=i64, device=dev), torch.empty(G, dtype=i64, device=dev)
        recs = slab.recs1.data_ptr()
        return {
            "producer_ms": device_ms(lambda: mp.produce(nat, st, slab, pend)),
            "moments_accum_ms": device_ms(lambda: nat.moments_accum(recs, mp.rw, voff, *regions, mode, -1, 0,
                                                                    state.data_ptr(), st)),
            "qsel_stats_ms": device_ms(lambda: nat.qsel_stats(recs, mp.rw, voff, *regions, cnt.data_ptr(), mn.data_ptr(),
                                                              mx.data_ptr(), width.data_ptr(), wmax.data_ptr(), st)),
            "records": int((pend.to(i64) - mp.seg_lo.to(i64)).sum().item()), "mode": int(mode), "tier": mp.tiers[0]}
    finally:
        PART_POOL.release(slab)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=100.0)
    ap.add_argument("--out", default="profiles/moments_probe.json")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    flat = tpch.generate_flat(args.sf, dev)
    ds = tpch.to_datasource(flat, profile="bench")
    del flat
    torch.cuda.empty_cache()
    sess = Session(engine=Engine())
    sess.register_datasource(ds)
    sess.register_table(T + "Base", schema=tpch.FLAT_SCHEMA)  # schema only
    sess.sql(tpch.druid_ddl(source=T + "Base", datasource="tpch", with_column_mapping=False))
    out = {"sf": args.sf, "rows": ds.num_rows, "device": torch.cuda.get_device_name(dev),
           "unit": "ms; statements: host clock around collect() (ends in the result copy), passes: device events; "
                   "median of 7 after 3 warm-ups",
           "shapes": {}}
    for name, fn, col, by in SHAPES:
        r = {}
        for side, call in ((fn, f"{fn}({col})"), ("avg", f"avg({col})"), ("median", f"median({col})")):
            q = f"select {by}, {call} from {T} group by {by}"
            df = sess.plan(q)
            rows, t = timed(df)
            t["sql"], t["pushed_queries"], t["groups"] = q, len(df.druid_query_specs()), len(rows)
            assert t["pushed_queries"] == 1, q
            if side == fn:
                mp = next(d._prepared._moments_prep for d in df.druid_queries())
                r["passes"] = passes_alone(mp)
            r[side] = t
        r[f"{fn}_over_avg"] = round(r[fn]["median_ms"] / r["avg"]["median_ms"], 2)
        r[f"{fn}_over_median"] = round(r[fn]["median_ms"] / r["median"]["median_ms"], 2)
        out["shapes"][name] = r
        print(json.dumps({name: r}), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
