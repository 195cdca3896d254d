"""Exact COUNT(DISTINCT dim): the pushed ``distinctCount`` bitsets against the two-level plan.

Over flattened TPC-H on one GPU, SQL end to end, it times every statement below twice in one
process: as the rewrite routes it now (one pushed groupBy whose ``distinctCount`` aggregators run
ops/csrc/distinct.hip) and with the routing switched off (sql/druid_rewrite.py DIRECT_DISTINCT =
False: the optimizer's two-level aggregation -- inner GROUP BY (groups, x), outer regroup, and a
join with the ordinary aggregates' own query).  Each is the median of 7 runs after 3 warm-ups, host
clock around collect(); both sides must return the same rows.  The table goes to
profiles/distinct_count_sf100.json.

    python tools/distinct_probe.py [--sf 100] [--out profiles/distinct_count_sf100.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spark_druid_olap_amd.engine.executor import Engine  # noqa: E402
from spark_druid_olap_amd.models import tpch  # noqa: E402
from spark_druid_olap_amd.session import Session  # noqa: E402
from spark_druid_olap_amd.sql import druid_rewrite  # noqa: E402

T = "orderLineItemPartSupplier"
# (name, statement): counted dimensions of 10^5 (o_clerk) .. 2 x 10^7 (l_partkey) values at SF100
STATEMENTS = [
    ("clerks_by_returnflag", f"select l_returnflag, count(distinct o_clerk) from {T} group by l_returnflag"),
    ("clerks_by_returnflag_with_sum",
     f"select l_returnflag, count(distinct o_clerk), sum(l_quantity) from {T} group by l_returnflag"),
    ("suppliers_by_shipmode", f"select l_shipmode, count(distinct l_suppkey) from {T} group by l_shipmode"),
    ("suppliers_by_shipmode_with_sum",
     f"select l_shipmode, count(distinct l_suppkey), sum(l_quantity), count(*) from {T} group by l_shipmode"),
    ("parts_by_nation", f"select s_nation, count(distinct l_partkey) from {T} group by s_nation"),
    ("suppliers_by_brand_type_q16_like",
     f"select p_brand, p_type, count(distinct l_suppkey) from {T} group by p_brand, p_type"),
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=100.0)
    ap.add_argument("--out", default="profiles/distinct_count_sf100.json")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    flat = tpch.generate_flat(args.sf, dev)
    ds = tpch.to_datasource(flat, profile="bench")
    del flat
    torch.cuda.empty_cache()
    sess = Session(engine=Engine(), conf={"spark.sparklinedata.druid.distinctCount.pushdown": "all"})
    sess.register_datasource(ds)
    sess.register_table(T + "Base", schema=tpch.FLAT_SCHEMA)  # schema only
    sess.sql(tpch.druid_ddl(source=T + "Base", datasource="tpch", with_column_mapping=False))
    out = {"sf": args.sf, "rows": ds.num_rows, "device": torch.cuda.get_device_name(dev),
           "unit": "ms, host clock around collect() (ends in the result copy), median of 7 after 3 warm-ups",
           "statements": {}}
    for name, q in STATEMENTS:
        r = {"sql": q}
        for side, on in (("distinct_count", True), ("two_level", False)):
            druid_rewrite.DIRECT_DISTINCT = on
            try:
                df = sess.plan(q)  # (planned afresh: the session's plan cache does not see the switch)
                rows, t = timed(df)
            finally:
                druid_rewrite.DIRECT_DISTINCT = True
            specs = df.druid_query_specs()
            t["pushed_queries"] = len(specs)
            if on:
                stats = [getattr(getattr(d, "_prepared", None), "last_stats", None) or {} for d in df.druid_queries()]
                t["tier"] = next((s["distinct_count_device"] for s in stats if "distinct_count_device" in s), None)
            r[side] = (t, sorted(map(tuple, rows), key=str))
        assert r["distinct_count"][1] == r["two_level"][1], name
        r["groups"] = len(r["distinct_count"][1])
        r["distinct_count"], r["two_level"] = r["distinct_count"][0], r["two_level"][0]
        r["speedup"] = round(r["two_level"]["median_ms"] / r["distinct_count"]["median_ms"], 2)
        out["statements"][name] = r
        print(json.dumps({name: r}), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
