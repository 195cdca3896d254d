"""max_by / min_by pushed down as per-group packed-key extremes, against max and median of the payload.

Over flattened TPC-H on one GPU, SQL end to end in one process, every statement is the median of 7
runs after 3 warm-ups, host clock around collect().  Per grouping: ``max_by(l_extendedprice,
l_quantity)`` (a packed 32-bit ordering column), ``max_by(l_extendedprice, l_shipdate)`` (the time
column: the row id alone, 2-word records), a ``min_by`` + ``max_by`` pair over one ordering column
(two-word states, one accumulation), and ``max`` (one fused scan) and ``median`` (the quantile
producer and the radix select) of the payload.  For each pushed statement the accumulation pass
alone is timed with device events in the tier the launcher picks and in every wider one.  Every
metric of the flat schema is stored in at most 32 bits, so the two wide passes are not measured
here.  The table goes to profiles/extreme_by_probe.json.

    python tools/extreme_probe.py [--sf 100] [--out profiles/extreme_by_probe.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from moments_probe import T, device_ms, timed  # noqa: E402

from spark_druid_olap_amd.engine.device_exec import EXT_BOTH, EXT_PACKED, MOM_TIERS, PART_POOL  # noqa: E402
from spark_druid_olap_amd.engine.executor import Engine  # noqa: E402
from spark_druid_olap_amd.models import tpch  # noqa: E402
from spark_druid_olap_amd.ops import native  # noqa: E402
from spark_druid_olap_amd.session import Session  # noqa: E402

X, Y, TIME = "l_extendedprice", "l_quantity", "cast(l_shipdate as date)"
GROUPINGS = [("by_returnflag", "l_returnflag"), ("by_brand_type", "p_brand, p_type")]
CALLS = [("max_by_quantity", f"max_by({X}, {Y})"), ("max_by_shipdate", f"max_by({X}, {TIME})"),
         ("min_by_max_by_quantity", f"min_by({X}, {Y}), max_by({X}, {Y})"), ("max", f"max({X})"),
         ("median", f"median({X})")]


def passes_alone(ep) -> dict:
    """The first ordering column's accumulation pass over the produced records, per tier that holds G."""
    nat, st = native.load(), native._stream(ep.dev)
    dev, G = ep.dev, ep.G
    pend = torch.empty(max(1, ep.nch), dtype=torch.int32, device=dev)
    slab = PART_POOL.acquire(dev, ep.words)
    try:
        regions = ep.produce(nat, st, slab, pend)
        voff, packed, dirs = next(iter(ep.passes.values()))
        assert packed
        state = torch.empty(G * 2, dtype=torch.int64, device=dev)
        recs = slab.recs1.data_ptr()
        out = {"producer_ms": device_ms(lambda: ep.produce(nat, st, slab, pend)),
               "records": int((pend.to(torch.int64) - ep.seg_lo.to(torch.int64)).sum().item()), "record_words": ep.rw,
               "state_words": 2 if dirs == EXT_BOTH else 1, "tier": ep.tiers[0]}
        for tier in range(MOM_TIERS.index(ep.tiers[0]), len(MOM_TIERS)):
            out[f"extreme_accum_{MOM_TIERS[tier]}_ms"] = device_ms(
                lambda: nat.extreme_accum(recs, ep.rw, voff, *regions, EXT_PACKED, dirs, tier, 0, state.data_ptr(), st))
        return out
    finally:
        PART_POOL.release(slab)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=100.0)
    ap.add_argument("--out", default="profiles/extreme_by_probe.json")
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
        for side, call in CALLS:
            q = f"select {by}, {call} from {T} group by {by}"
            df = sess.plan(q)
            rows, t = timed(df)
            t["sql"], t["pushed_queries"], t["groups"] = q, len(df.druid_query_specs()), len(rows)
            assert t["pushed_queries"] == 1, q
            if "_by_" in side:
                ep = next(d._prepared._extremes_prep for d in df.druid_queries())
                assert ep, q  # (the device extremes answered)
                t["passes"] = passes_alone(ep)
            r[side] = t
        for side, _ in CALLS[:3]:
            r[f"{side}_over_max"] = round(r[side]["median_ms"] / r["max"]["median_ms"], 2)
            r[f"{side}_over_median"] = round(r[side]["median_ms"] / r["median"]["median_ms"], 2)
        out["shapes"][name] = r
        print(json.dumps({name: r}), flush=True)
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
