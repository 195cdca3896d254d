"""corr / covar_samp pushed down as per-group co-moment sums, against stddev and avg of the same columns.

Over flattened TPC-H on one GPU, SQL end to end in one process, every statement is the median of 7
runs after 3 warm-ups, host clock around collect().  Per grouping: ``corr`` and ``covar_samp`` of
(l_quantity, l_extendedprice), and ``stddev`` and ``avg`` of both columns in one statement (avg is
one fused scan; stddev the producer pass and one moments pass per column; corr / covar_samp the
producer pass and ONE pass over the pair).  For each pushed co-moment statement the accumulation
pass alone is timed with device events in the tier the launcher picks and in the next wider one.
The flat schema has no double metric, so the two-pass double path is not measured here.  The table
goes to profiles/comoments_probe.json.

    python tools/comoments_probe.py [--sf 100] [--out profiles/comoments_probe.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from moments_probe import T, device_ms, timed  # noqa: E402

from spark_druid_olap_amd.engine.device_exec import MOM_TIERS, PART_POOL, co_words  # noqa: E402
from spark_druid_olap_amd.engine.executor import Engine  # noqa: E402
from spark_druid_olap_amd.models import tpch  # noqa: E402
from spark_druid_olap_amd.ops import native  # noqa: E402
from spark_druid_olap_amd.session import Session  # noqa: E402

X, Y = "l_quantity", "l_extendedprice"
GROUPINGS = [("by_returnflag", "l_returnflag"), ("by_brand_type", "p_brand, p_type")]


def passes_alone(cp) -> dict:
    """The first pair's accumulation pass over the produced records, per tier that holds G."""
    nat, st = native.load(), native._stream(cp.dev)
    dev, G = cp.dev, cp.G
    pend = torch.empty(max(1, cp.nch), dtype=torch.int32, device=dev)
    slab = PART_POOL.acquire(dev, cp.words)
    try:
        regions = cp.produce(nat, st, slab, pend)
        (vx, vy), mode, sq, dbl, _ = next(iter(cp.passes.values()))
        state = torch.empty(G * co_words(mode, sq), dtype=torch.int64, device=dev)
        recs = slab.recs1.data_ptr()
        out = {"producer_ms": device_ms(lambda: cp.produce(nat, st, slab, pend)),
               "records": int((pend.to(torch.int64) - cp.seg_lo.to(torch.int64)).sum().item()), "mode": int(mode),
               "squares": bool(sq), "tier": cp.tiers[0]}
        first = MOM_TIERS.index(cp.tiers[0])
        for tier in range(first, min(first + 2, len(MOM_TIERS))):  # (the picked tier and the next wider one)
            out[f"comoments_accum_{MOM_TIERS[tier]}_ms"] = device_ms(
                lambda: nat.comoments_accum(recs, cp.rw, vx, vy, *regions, mode, sq, dbl, tier, 0, state.data_ptr(), st))
        return out
    finally:
        PART_POOL.release(slab)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=100.0)
    ap.add_argument("--out", default="profiles/comoments_probe.json")
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
    for name, by in GROUPINGS:
        r = {}
        for side, call in (("corr", f"corr({X}, {Y})"), ("covar_samp", f"covar_samp({X}, {Y})"),
                           ("stddev", f"stddev({X}), stddev({Y})"), ("avg", f"avg({X}), avg({Y})")):
            q = f"select {by}, {call} from {T} group by {by}"
            df = sess.plan(q)
            rows, t = timed(df)
            t["sql"], t["pushed_queries"], t["groups"] = q, len(df.druid_query_specs()), len(rows)
            assert t["pushed_queries"] == 1, q
            if side in ("corr", "covar_samp"):
                t["passes"] = passes_alone(next(d._prepared._comoments_prep for d in df.druid_queries()))
            r[side] = t
        for side in ("corr", "covar_samp"):
            r[f"{side}_over_stddev"] = round(r[side]["median_ms"] / r["stddev"]["median_ms"], 2)
            r[f"{side}_over_avg"] = round(r[side]["median_ms"] / r["avg"]["median_ms"], 2)
        out["shapes"][name] = r
        print(json.dumps({name: r}), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
