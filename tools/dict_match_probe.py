"""Host against device for text predicates over a materialized string dictionary.

For dictionaries of 10^2 .. 4*10^6 random entries (mean length ~24 and ~96 bytes, 1 % of them
non-ASCII) and the predicates LIKE '%abc%', LIKE 'abc%' and insensitive_contains 'abc' it times

* the host path as lowering runs it without the matcher: for LIKE the vectorised regex of
  sql/functions.py ``_like`` that a filter's ``_pyvec`` evaluates over ``all_values()``
  (``Series.str.match(like_to_regex(p), flags=re.S)``), for insensitive_contains
  ``Dictionary.eval_mask`` with the lowerer's lambda;
* the device path end to end (engine/dict_match.py ``match_mask``): program compile, launch, the
  copy back, unpack and -- when folding -- the recheck of the flagged entries;

each as the median of 7 runs after 3 warm-ups, and the one-time heap build + upload on its own.
The table goes to profiles/dict_match_probe.json; ``crossover`` is the smallest cardinality from
which the device wins for every predicate and both lengths (engine/dict_match.py DEVICE_MIN_CARD).

    python tools/dict_match_probe.py [--out profiles/dict_match_probe.json] [--max 4000000]
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spark_druid_olap_amd.engine import dict_match  # noqa: E402
from spark_druid_olap_amd.segment.dictionary import Dictionary  # noqa: E402
from spark_druid_olap_amd.segment.textheap import text_heap  # noqa: E402
from spark_druid_olap_amd.sql.functions import like_to_regex  # noqa: E402

CARDS = [100, 1000, 10_000, 100_000, 1_000_000, 4_000_000]
LENGTHS = [24, 96]


def make_dictionary(n: int, mean_len: int, seed: int) -> Dictionary:
    rng = np.random.default_rng(seed)
    hi = mean_len * 3 // 2
    buf = rng.integers(97, 123, size=(n, hi), dtype=np.uint8)
    lens = rng.integers(mean_len // 2, hi + 1, size=n)
    vals = {buf[i, :l].tobytes().decode() + ("é" if i % 100 == 0 else "") for i, l in enumerate(lens.tolist())}
    return Dictionary(np.array(sorted(vals), dtype=object))


def median_ms(fn, runs: int = 7, warm: int = 3) -> float:
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def cases(d: Dictionary, dev):
    for pat in ("%abc%", "abc%"):
        rx = like_to_regex(pat)
        yield (f"LIKE '{pat}'",
               lambda rx=rx: np.asarray(pd.Series(d.all_values()).str.match(rx, flags=re.S), dtype=bool),
               lambda pat=pat: dict_match.match_mask(d, dev, dict_match.compile_like(pat)))
    pred = lambda v: v is not None and "abc" in str(v).lower()  # noqa: E731
    yield ("insensitive_contains 'abc'", lambda: d.eval_mask(pred),
           lambda: dict_match.match_mask(d, dev, dict_match.compile_needles(["abc"], True), pred))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/dict_match_probe.json")
    ap.add_argument("--max", type=int, default=CARDS[-1])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for n in [c for c in CARDS if c <= args.max]:
        for L in LENGTHS:
            d = make_dictionary(n, L, seed=n + L)
            t0 = time.perf_counter()
            th = text_heap(d, dev)
            build_ms = (time.perf_counter() - t0) * 1e3
            for name, host, device in cases(d, dev):
                assert np.array_equal(host(), device()), name
                r = {"cardinality": len(d), "mean_len": L, "predicate": name, "host_ms": round(median_ms(host), 3),
                     "device_ms": round(median_ms(device), 3), "heap_build_upload_ms": round(build_ms, 2),
                     "heap_bytes": th.nbytes}
                rows.append(r)
                print(json.dumps(r), flush=True)
    wins = {n: all(r["device_ms"] < r["host_ms"] for r in rows if r["cardinality"] >= n) for n in
            sorted({r["cardinality"] for r in rows})}
    out = {"device": torch.cuda.get_device_name(dev), "runs": "median of 7 after 3 warm-ups",
           "crossover": next((n for n, w in wins.items() if w), None), "rows": rows}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("crossover", out["crossover"])


if __name__ == "__main__":
    main()
