"""skewness / kurtosis pushed down as per-group power sums, against stddev, avg and median of the
same column.

Over flattened TPC-H on one GPU, SQL end to end in one process, every statement is the median of 7
runs after 3 warm-ups, host clock around collect().  Per grouping and column: ``skewness``,
``kurtosis``, ``stddev``, ``avg`` and ``median`` (avg is one fused scan; stddev the producer pass
and one moments pass; skewness / kurtosis the producer pass and ONE pass over 7- / 11-word states).
For each pushed skewness / kurtosis statement the accumulation pass alone is timed with device
events in the tier the launcher picks and in every wider one, next to ``moments_accum`` over the
same records (the yardstick: the 4-word variance state).  The flat schema has no double metric and
no integer metric of range >= 2^32, so the two-pass f64 path is not measured here.  The table goes
to profiles/central_moments_probe.json.

    python tools/central_moments_probe.py [--sf 100] [--out profiles/central_moments_probe.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from moments_probe import T, device_ms, timed  # noqa: E402

from spark_druid_olap_amd.engine.device_exec import CM_WORDS, MOM_INT2, MOM_INT4, MOM_TIERS, PART_POOL  # noqa: E402
from spark_druid_olap_amd.engine.executor import Engine  # noqa: E402
from spark_druid_olap_amd.models import tpch  # noqa: E402
from spark_druid_olap_amd.ops import native  # noqa: E402
from spark_druid_olap_amd.session import Session  # noqa: E402

COLUMNS = ["l_quantity", "l_extendedprice"]
GROUPINGS = [("by_returnflag", "l_returnflag"), ("by_brand_type", "p_brand, p_type")]


def passes_alone(cp) -> dict:
    """The first column's accumulation pass over the produced records, per tier that holds G, and
    the variance sums' pass over the same records."""
    nat, st = native.load(), native._stream(cp.dev)
    dev, G = cp.dev, cp.G
    pend = torch.empty(max(1, cp.nch), dtype=torch.int32, device=dev)
    slab = PART_POOL.acquire(dev, cp.words)
    try:
        regions = cp.produce(nat, st, slab, pend)
        col, (voff, mode, order, pivot, dbl) = next(iter(cp.passes.items()))
        state = torch.empty(G * CM_WORDS[mode], dtype=torch.int64, device=dev)
        recs = slab.recs1.data_ptr()
        mom = MOM_INT2 if cp.prog.ds.metrics[col].data.dtype.itemsize <= 4 else MOM_INT4
        out = {"producer_ms": device_ms(lambda: cp.produce(nat, st, slab, pend)),
               "records": int((pend.to(torch.int64) - cp.seg_lo.to(torch.int64)).sum().item()), "mode": int(mode),
               "tier": cp.tiers[0],
               "moments_accum_ms": device_ms(lambda: nat.moments_accum(recs, cp.rw, voff, *regions, mom, -1, 0,
                                                                       state.data_ptr(), st))}
        for tier in range(MOM_TIERS.index(cp.tiers[0]), len(MOM_TIERS)):  # (the picked tier and every wider one)
            out[f"central_moments_accum_{MOM_TIERS[tier]}_ms"] = device_ms(
                lambda: nat.central_moments_accum(recs, cp.rw, voff, *regions, mode, tier, pivot, dbl, 0,
                                                  state.data_ptr(), st))
        return out
    finally:
        PART_POOL.release(slab)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=100.0)
    ap.add_argument("--out", default="profiles/central_moments_probe.json")
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
    for gname, by in GROUPINGS:
        for col in COLUMNS:
            r = {}
            for fn in ("skewness", "kurtosis", "stddev", "avg", "median"):
                q = f"select {by}, {fn}({col}) from {T} group by {by}"
                df = sess.plan(q)
                rows, t = timed(df)
                t["sql"], t["pushed_queries"], t["groups"] = q, len(df.druid_query_specs()), len(rows)
                assert t["pushed_queries"] == 1, q
                if fn in ("skewness", "kurtosis"):
                    t["passes"] = passes_alone(next(d._prepared._central_moments_prep for d in df.druid_queries()))
                r[fn] = t
            for fn in ("skewness", "kurtosis"):
                for other in ("stddev", "avg", "median"):
                    r[f"{fn}_over_{other}"] = round(r[fn]["median_ms"] / r[other]["median_ms"], 2)
                p = r[fn]["passes"]
                p["accum_over_moments_accum"] = round(p[f"central_moments_accum_{p['tier']}_ms"] / p["moments_accum_ms"], 2)
            out["shapes"][f"{col}_{gname}"] = r
            print(json.dumps({f"{col}_{gname}": r}), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
