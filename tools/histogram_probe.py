"""Fixed-bucket histograms pushed down as per-group bucket counts, against count(*), median and the
same counts written as conditional sums.

Over flattened TPC-H on one GPU, SQL end to end in one process, every statement is the median of 7
runs after 3 warm-ups, host clock around collect().  Per grouping: ``histogram(l_extendedprice, 0,
100000, 20)`` and ``histogram(l_quantity, 0, 50, 50)``, ``count(*)`` (one fused scan), ``median`` of
the price (the quantile producer and the radix select) and the only way to get the first
histogram's 22 numbers without the aggregator: one ``sum(case when ... then 1 else 0 end)`` per
counter -- in TWO statements of 11 counters, timed together, because a pushed query holds at most
12 aggregators (ops/desc.py MAX_AOPS).  For each histogram the accumulation pass alone is timed
with device events in every tier that can hold its counters, the tier forced.  The table goes to
profiles/histogram_probe.json.

    python tools/histogram_probe.py [--sf 100] [--out profiles/histogram_probe.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from moments_probe import T, device_ms, timed  # noqa: E402

from spark_druid_olap_amd.engine.device_exec import FBH_TIERS, PART_POOL  # noqa: E402
from spark_druid_olap_amd.engine.executor import Engine  # noqa: E402
from spark_druid_olap_amd.models import tpch  # noqa: E402
from spark_druid_olap_amd.ops import native  # noqa: E402
from spark_druid_olap_amd.session import Session  # noqa: E402

X, LO, HI, B = "l_extendedprice", 0, 100000, 20
GROUPINGS = [("by_returnflag", "l_returnflag"), ("by_brand_type", "p_brand, p_type")]


def case_sums() -> list:
    """The B + 2 counters of histogram(X, LO, HI, B) as conditional sums, 11 a statement."""
    e = [LO + i * (HI - LO) // B for i in range(B + 1)]
    conds = [f"{X} < {e[0]}"] + [f"{X} >= {a} and {X} < {b}" for a, b in zip(e, e[1:])] + [f"{X} >= {e[-1]}"]
    sums = [f"sum(case when {c} then 1 else 0 end)" for c in conds]
    return [", ".join(sums[i:i + 11]) for i in range(0, len(sums), 11)]


class Together:
    """Several planned statements collected one after the other: rows joined per group key."""

    def __init__(self, dfs, nk):
        self.dfs, self.nk = dfs, nk

    def collect(self):
        parts = [dict((r[:self.nk], r[self.nk:]) for r in df.collect()) for df in self.dfs]
        return [k + sum((p[k] for p in parts), ()) for k in parts[0]]

    def druid_query_specs(self):
        return [s for df in self.dfs for s in df.druid_query_specs()]


CALLS = [("histogram_price", f"histogram({X}, {LO}, {HI}, {B})"), ("histogram_quantity", "histogram(l_quantity, 0, 50, 50)"),
         ("count", "count(*)"), ("median", f"median({X})"), ("case_sums_price", case_sums())]


def passes_alone(ep) -> dict:
    """The accumulation pass over the produced records, forced into every tier that holds it."""
    nat, st = native.load(), native._stream(ep.dev)
    pend = torch.empty(max(1, ep.nch), dtype=torch.int32, device=ep.dev)
    slab = PART_POOL.acquire(ep.dev, ep.words)
    try:
        regions = ep.produce(nat, st, slab, pend)
        key = next(iter(ep.passes))
        recs = slab.recs1.data_ptr()
        out = {"producer_ms": device_ms(lambda: ep.produce(nat, st, slab, pend)),
               "records": int((pend.to(torch.int64) - ep.seg_lo.to(torch.int64)).sum().item()), "key_space": ep.G,
               "counters": ep.G * (ep.passes[key][1].numel() + 1), "tier": ep.tiers[0]}
        want = None
        for tier, name in enumerate(FBH_TIERS):
            try:
                got, _ = ep.accumulate(nat, st, recs, regions, key, tier)
            except ValueError:
                continue  # (the tier does not hold the counters)
            want = got if want is None else want
            assert torch.equal(got, want), name  # every tier counts the same
            out[f"histogram_accum_{name}_ms"] = device_ms(lambda: ep.accumulate(nat, st, recs, regions, key, tier))
        return out
    finally:
        PART_POOL.release(slab)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=100.0)
    ap.add_argument("--out", default="profiles/histogram_probe.json")
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
        r, answers, nk = {}, {}, len(by.split(","))
        for side, call in CALLS:
            qs = [f"select {by}, {c} from {T} group by {by}" for c in (call if isinstance(call, list) else [call])]
            df = sess.plan(qs[0]) if len(qs) == 1 else Together([sess.plan(q) for q in qs], nk)
            q = "; ".join(qs)
            try:
                rows, t = timed(df)
            except RuntimeError as e:
                if side != "case_sums_price":
                    raise
                r[side] = {"sql": q, "error": str(e)}  # (the engine does not answer the conditional sums here)
                continue
            answers[side] = rows
            t["sql"], t["pushed_queries"], t["groups"] = q, len(df.druid_query_specs()), len(rows)
            assert t["pushed_queries"] == len(qs), q
            if side.startswith("histogram"):
                ep = next(d._prepared._histogram_prep for d in df.druid_queries())
                assert ep, q  # (the device counts answered)
                t["passes"] = passes_alone(ep)
            r[side] = t
        # (both ways to the 22 numbers agree)
        assert "case_sums_price" not in answers or \
            sorted((row[:nk], list(row[nk])) for row in answers["histogram_price"]) == \
            sorted((row[:nk], [int(c) for c in row[nk:]]) for row in answers["case_sums_price"]), name
        for side in ("histogram_price", "histogram_quantity"):
            for other in ("count", "median", "case_sums_price"):
                if "median_ms" in r[other]:
                    r[f"{side}_over_{other}"] = round(r[side]["median_ms"] / r[other]["median_ms"], 2)
        out["shapes"][name] = r
        print(json.dumps({name: r}), flush=True)
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
