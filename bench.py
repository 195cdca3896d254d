#!/usr/bin/env python3
"""Benchmark: the reference's TPC-H benchmark suite (sd/tools/TpchBenchMark.scala:135-323) on
MI355X -- 8 queries over the flattened, Druid-indexed TPC-H table, geometric-mean latency.

Contract (driver): ``python bench.py --gpus N --steps K --warmup W``; for N > 1 launched by
torchrun, one rank per GPU.  A "step" = one pass over the 8-query suite (each query planned
once like the reference's DataFrame, executed per step with results collected to host numpy
columns, i.e. ``df.collect()``).  Weak scaling: every GPU holds SF=--sf (default 100) of
synthetic TPC-H (random dictionary values), so N GPUs hold SF=100*N.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the line.  ``--full`` adds the untimed
passes reported alongside (``collect_ms``: every result column decoded to host objects;
``kernels.shape_shared_geomean_ms``: the suite on the shape-shared kernels).  ``--dump-outputs DIR``
writes the result columns of the last timed step as ``DIR/<query>__<column>.npy`` (the data is
seeded, so two builds run with the same arguments can be compared output for output).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# The benchmark repeats a fixed statement set: each prepared scan compiles its literal-specialized
# kernel at its first (warmup) execution (engine/device_exec.py SPECIALIZE), as a server does for
# its repeated statements in the background.
os.environ.setdefault("SDO_JIT_SPECIALIZE", "sync")
os.environ.setdefault("SDO_JIT_SPECIALIZE_AFTER", "1")

BASELINE_GEOMEAN_MS = 5163.0  # reference Druid-backed geomean, 8 queries (SF10, 4x2-core)
DUMP_MAX_BYTES = 64_000_000  # --dump-outputs: all files together stay below this


def log(*a):
    if int(os.environ.get("RANK", "0")) == 0:
        print(*a, file=sys.stderr, flush=True)


def _result_columns(r):
    """(name, column) of a timed run's result: a SQL statement's Batch or a spec query's QueryResult."""
    if hasattr(r, "refs"):
        return [(ref.name, r.cols[ref.rid]) for ref in r.refs]
    return [(c, r.data[c]) for c in r.columns]


def _as_float(col):
    """A result column as float64: numbers as they are (NULL -> NaN), timestamps as epoch
    nanoseconds, everything else (strings, decoded from their dictionary) as the CRC-32 of its text."""
    import zlib

    import numpy as np
    import pandas as pd

    if hasattr(col, "codes") and hasattr(col, "dictionary"):  # engine/columns.py DictColumn
        col = col.to_numpy()
    s = col if isinstance(col, pd.Series) else pd.Series(np.asarray(col))
    if s.dtype.kind == "M":
        return s.astype("int64").to_numpy(dtype=np.float64)
    if pd.api.types.is_bool_dtype(s.dtype) or pd.api.types.is_numeric_dtype(s.dtype):
        return s.to_numpy(dtype=np.float64, na_value=np.nan)
    return np.array([np.nan if v is None or v is pd.NA else zlib.crc32(str(v).encode()) for v in s.tolist()],
                    dtype=np.float64)


def dump_outputs(outdir, results):
    """Write every query's result columns as ``<query>__<column>.npy`` (float64).  Each query gets
    an equal share of DUMP_MAX_BYTES; a larger result is cut to a fixed, seeded sample of its rows
    (in result order)."""
    import re

    import numpy as np

    os.makedirs(outdir, exist_ok=True)
    share = DUMP_MAX_BYTES // max(1, len(results))
    for qi, (qname, r) in enumerate(results):
        cols = _result_columns(r)
        n = len(cols[0][1]) if cols else 0
        keep = share // (8 * max(1, len(cols)))
        idx = None
        if n > keep:
            idx = np.sort(np.random.default_rng(20260101).choice(n, size=keep, replace=False))
        for ci, (cname, col) in enumerate(cols):
            a = _as_float(col)
            if idx is not None:
                a = a[idx]
            q, c = (re.sub(r"[^A-Za-z0-9]+", "_", x).strip("_") for x in (qname, cname))
            np.save(os.path.join(outdir, f"{qi:02d}_{q}__{ci:02d}_{c}.npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sf", type=float, default=100.0,
                    help="scale factor PER GPU (weak scaling: N GPUs hold N x SF)")
    ap.add_argument("--total-sf", type=float, default=None,
                    help="scale factor of the WHOLE job, split over the GPUs (strong scaling: the fixed-SF100 "
                         "curve at 1/2/4/8 GPUs, or SF1000 over 8 GPUs = 125 per GPU)")
    ap.add_argument("--mode", choices=["sql", "spec"], default="sql")
    ap.add_argument("--model", choices=["tpch", "ssb", "tpch22"], default="tpch",
                    help="tpch: the reference's 8-query TPC-H suite (headline); ssb: BASELINE config 4; "
                         "tpch22: the full 22-query TPC-H sweep over the flattened index (BASELINE config 2)")
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also run the untimed passes reported alongside: collect_ms (every result column "
                         "decoded to host objects) and the suite on the shape-shared kernels")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the result columns of the last timed step as DIR/<query>__<column>.npy")
    # diagnostics (the JSON line then describes what was run)
    ap.add_argument("--only", default="", help="comma-separated subset of the suite's query names")
    ap.add_argument("--profile-rank", type=int, default=None, help="cProfile this rank's timed steps (stderr)")
    ap.add_argument("--keep-cache", action="store_true", help="keep the allocator cache of data generation")
    ap.add_argument("--no-shape", action="store_true", help="(--full) skip the untimed shape-shared kernel pass")
    ap.add_argument("--per-rank", action="store_true", help="every rank's own per-query means")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # one process per GPU, started here (never from a process that touched the GPU)
        from spark_druid_olap_amd.utils.launch import spawn_ranks

        sys.exit(spawn_ranks(args.gpus, [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]))

    import torch

    from spark_druid_olap_amd.parallel.world import init_world

    world = init_world()
    if world.size != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the process group has {world.size} rank(s)")
    strong = args.total_sf is not None
    if strong:
        args.sf = args.total_sf / world.size  # each rank generates its disjoint share of the total
    dev = world.device()
    if dev.type == "cuda":
        torch.cuda.set_device(dev)
    t0 = time.time()
    from spark_druid_olap_amd.engine.executor import Engine
    from spark_druid_olap_amd.models import ssb, tpch

    if args.model in ("ssb", "tpch22"):
        args.mode = "sql"
    if args.model == "ssb":
        flat = ssb.generate_flat(args.sf, dev, rank=world.rank, world=world.size)
        ds = ssb.to_datasource(flat)
    else:
        flat = tpch.generate_flat(args.sf, dev, rank=world.rank, world=world.size)
        ds = tpch.to_datasource(flat, profile="bench")
    nrows = ds.num_rows
    del flat
    gen_peak = None
    if dev.type == "cuda":
        torch.cuda.synchronize()
        if not args.keep_cache:
            torch.cuda.empty_cache()
        # synthetic data generation holds the raw columns next to the index: its peak is not the
        # engine's, so the run's peak is measured from here on
        gen_peak = torch.cuda.max_memory_reserved(dev) / 1e9
        torch.cuda.reset_peak_memory_stats(dev)
    log(f"[bench] rank0 shard: {nrows} rows, {ds.size_bytes() / 1e9:.1f} GB resident, gen+index {time.time() - t0:.1f}s")

    engine = Engine(world)
    if args.model == "ssb":
        from spark_druid_olap_amd.session import Session

        sess = Session(engine=engine)
        sess.register_datasource(ds)
        ssb.register(sess)
        queries = [(name, sess.sql(q).prepared()) for name, q in ssb.ALL_QUERIES]
        for name, df in queries:
            assert df.druid_queries(), f"{name} was not pushed to the GPU engine"
    elif args.model == "tpch22":
        from spark_druid_olap_amd.models import tpch22
        from spark_druid_olap_amd.session import Session

        # exact count(distinct) (TPC-H answers), unlike the reference's 8-query benchmark
        sess = Session(engine=engine)
        sess.register_datasource(ds)
        sess.register_table("orderLineItemPartSupplierBase", schema=tpch.FLAT_SCHEMA)  # schema only
        sess.sql(tpch.druid_ddl(source="orderLineItemPartSupplierBase", datasource="tpch",
                                with_column_mapping=False))
        queries = [(name, sess.sql(q).prepared()) for name, q in tpch22.QUERIES]
        for name, df in queries:
            assert df.druid_queries(), f"{name} was not pushed to the GPU engine"
    elif args.mode == "sql":
        from spark_druid_olap_amd.session import Session

        # count(distinct o_orderkey) is pushed as the cardinality (HLL) aggregator, exactly as in the
        # reference's published benchmark queries (docs/benchmark/druid/queries/*.json)
        sess = Session(engine=engine, conf={"spark.sparklinedata.druid.approxCountDistinct": "true"})
        sess.register_datasource(ds)
        sess.register_table("orderLineItemPartSupplierBase", schema=tpch.FLAT_SCHEMA)  # schema only
        sess.sql(tpch.druid_ddl(source="orderLineItemPartSupplierBase", datasource="tpch",
                                with_column_mapping=False))
        queries = [(name, sess.sql(q).prepared()) for name, q in tpch.BENCH_QUERIES]
        for name, df in queries:
            assert df.druid_queries(), f"{name} was not pushed to the GPU engine"
    else:
        from spark_druid_olap_amd.models.bench_queries import bench_specs

        queries = [(name, engine.prepare(q, ds)) for name, q in bench_specs()]

    only = [x for x in args.only.split(",") if x]
    if only:  # diagnostics: a subset of the suite (the JSON line then describes only that subset)
        queries = [(n, q) for n, q in queries if n in only]
    nsuite = len(queries)

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    from spark_druid_olap_amd.engine.executor import results_on_root

    # rank 0 consumes the answers (df.collect() on the reference's driver): the final groups are
    # gathered to rank 0 only and only rank 0 decodes them (engine/executor.py results_on_root)
    ctx = results_on_root(os.environ.get("SDO_RESULTS_ON_ROOT", "1") != "0")
    ctx.__enter__()
    lat = {name: [] for name, _ in queries}
    stats = {name: {} for name, _ in queries}
    last = {}  # (--dump-outputs) every query's most recent timed result
    # the serving process's collector settings (server/gateway.py start): everything built so far --
    # shards, dictionaries, plans -- moves to the permanent generation and young collections come
    # less often, so a full collection does not walk it in the middle of a query
    from spark_druid_olap_amd.utils.memory import serving_gc

    serving_gc()
    for _ in range(args.warmup):
        for name, pq in queries:
            pq.run()
    world.barrier()
    sync()
    prof = None
    if args.profile_rank is not None and world.rank == args.profile_rank:
        import cProfile

        prof = cProfile.Profile()
        prof.enable()
    tstart = time.perf_counter()
    for _ in range(args.steps):
        for name, pq in queries:
            a = time.perf_counter()
            r = pq.run()
            lat[name].append((time.perf_counter() - a) * 1e3)
            if args.dump_outputs:
                last[name] = r
            st = getattr(r, "stats", None) if args.verbose else None
            if st:
                for k, v in st.items():
                    if k.endswith("_ms"):
                        stats[name].setdefault(k, []).append(v)
    sync()
    world.barrier()
    total_ms = (time.perf_counter() - tstart) * 1e3
    ctx.__exit__(None, None, None)
    if prof is not None:
        import pstats

        prof.disable()
        pstats.Stats(prof, stream=sys.stderr).sort_stats("cumulative").print_stats(60)
    if args.dump_outputs and world.rank == 0:  # (the answers are on rank 0)
        dump_outputs(args.dump_outputs, [(n, last[n]) for n, _ in queries if last.get(n) is not None])
    last.clear()
    # (--full) untimed, reported alongside: each query end to end INCLUDING host materialization of every result
    # column (dictionary-coded strings decoded to Python objects, as the reference's df.collect() returns
    # them): the timed value leaves string columns dictionary-coded (engine/columns.py DictColumn)
    coll = {}
    if args.full and args.mode == "sql":
        with results_on_root(os.environ.get("SDO_RESULTS_ON_ROOT", "1") != "0"):
            for _ in range(max(2, min(args.steps, 3))):
                for name, pq in queries:
                    a = time.perf_counter()
                    b = pq.run()
                    if world.rank == 0 and b is not None:
                        for r in b.refs:
                            b.cols[r.rid].to_numpy()
                    coll.setdefault(name, []).append((time.perf_counter() - a) * 1e3)
                world.barrier()
    shape_geo = None
    if args.full and args.mode == "sql" and not only and not args.no_shape:
        # (--full) untimed, reported alongside: the same suite on the shape-shared kernels a first-seen
        # parameterization runs (query constants read from the descriptor, no literal-specialized
        # code object) -- freshly planned statements with specialization switched off
        from spark_druid_olap_amd.engine import device_exec as DE

        texts = {n: df.sql_text for n, df in queries}
        queries = pq = None  # (release the specialized statements' buffers first)
        import gc

        gc.collect()
        if dev.type == "cuda":
            torch.cuda.empty_cache()
        DE.SPECIALIZE = "off"
        sess._plan_cache.clear()
        shaped = [(n, sess.sql(t).prepared()) for n, t in texts.items()]
        with results_on_root(os.environ.get("SDO_RESULTS_ON_ROOT", "1") != "0"):
            for n, q in shaped:
                q.run()
            world.barrier()
            slat = {n: [] for n, _ in shaped}
            for _ in range(max(2, min(args.steps, 5))):
                for n, q in shaped:
                    a = time.perf_counter()
                    q.run()
                    slat[n].append((time.perf_counter() - a) * 1e3)
            world.barrier()
        smeans = {k: world.max_float(sum(v) / len(v)) for k, v in slat.items()}
        shape_geo = math.exp(sum(math.log(max(m, 1e-6)) for m in smeans.values()) / len(smeans))
    if args.per_rank:  # diagnostics: every rank's own means
        print(f"[bench] rank {world.rank}: " + " ".join(f"{k[:12]}={sum(v) / len(v):.3f}" for k, v in lat.items()),
              file=sys.stderr, flush=True)
    total_ms = world.max_float(total_ms)
    hbm = None
    if dev.type == "cuda":  # peak device memory of the run (index + scan buffers + kernels), max over ranks
        hbm = {"index_gb": round(world.max_float(ds.size_bytes() / 1e9), 2),
               "max_reserved_gb": round(world.max_float(torch.cuda.max_memory_reserved(dev) / 1e9), 2),
               "max_allocated_gb": round(world.max_float(torch.cuda.max_memory_allocated(dev) / 1e9), 2),
               "datagen_peak_reserved_gb": round(world.max_float(gen_peak), 2),
               "device_total_gb": round(torch.cuda.get_device_properties(dev).total_memory / 1e9, 1)}
    means = {k: world.max_float(sum(v) / len(v)) for k, v in lat.items()}
    geo = math.exp(sum(math.log(max(m, 1e-6)) for m in means.values()) / len(means))
    nq = nsuite * args.steps
    mins = {k: world.max_float(min(v)) for k, v in lat.items()}
    maxs = {k: world.max_float(max(v)) for k, v in lat.items()}
    cmeans = {k: world.max_float(sum(v) / len(v)) for k, v in coll.items()}
    cgeo = math.exp(sum(math.log(max(m, 1e-6)) for m in cmeans.values()) / len(cmeans)) if cmeans else None
    if world.rank == 0:
        if args.verbose:
            for k, v in means.items():
                log(f"[bench] {k:55s} avg {v:9.3f}  min {mins[k]:9.3f}  max {maxs[k]:9.3f} ms  " +
                    " ".join(f"{sk}={sum(sv) / len(sv):.3f}" for sk, sv in stats[k].items()))
        if args.model == "ssb":
            metric = "ssb_17query_geomean_latency_ms"
            model = f"SSB lineorder star schema, SF{args.sf:g} per GPU (SF{args.sf * world.size:g} total)"
            vs = None  # the reference publishes no SSB numbers
        elif args.model == "tpch22":
            metric = "tpch_flat_22query_geomean_latency_ms"
            model = (f"TPC-H 22 queries over flattened orderLineItemPartSupplier, SF{args.sf:g} per GPU "
                     f"(SF{args.sf * world.size:g} total)")
            vs = None  # the reference publishes no 22-query numbers
        else:
            metric = "tpch_flat_8query_geomean_latency_ms"
            model = (f"TPC-H flattened orderLineItemPartSupplier, SF{args.sf:g} per GPU "
                     f"(SF{args.sf * world.size:g} total), Druid bench index")
            vs = round(geo / BASELINE_GEOMEAN_MS, 8)
        total_sf = args.sf * world.size
        if strong:
            model = model.replace(f"SF{args.sf:g} per GPU (SF{total_sf:g} total)", f"SF{total_sf:g} total "
                                  f"(SF{args.sf:g} per GPU)")
        out = {
            "metric": metric,
            "value": round(geo, 4),
            "unit": "ms",
            "n_gpus": world.size,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(total_ms / args.steps, 4),
            "higher_is_better": False,
            "scaling": "strong" if strong else "weak",
            "vs_baseline": vs,
            "dtype": "int64-exact-decimal/f64",
            "data": f"synthetic ({args.model.upper()} dbgen-like distributions, random dictionary values, generated on device)",
            "config": {"model": model,
                       "global_batch": nq, "seq_len": int(nrows), "parallelism": f"dp{world.size} (segment shards)",
                       "queries": nsuite, "mode": args.mode, "scale_factor_total": total_sf,
                       "scale_factor_per_gpu": args.sf,
                       "world": {"size": world.size, "backend": world.backend}},
            "qps": round(nq / (total_ms / 1e3), 3),
            "per_query_ms": {k: round(v, 4) for k, v in means.items()},
            "per_query_min_ms": {k: round(v, 4) for k, v in mins.items()},
            "per_query_max_ms": {k: round(v, 4) for k, v in maxs.items()},
            # (--full) untimed: run + decode of every result column to host objects (df.collect()'s work)
            "collect_ms": {k: round(v, 4) for k, v in cmeans.items()} or None,
            "collect_geomean_ms": round(cgeo, 4) if cgeo is not None else None,
            "rows_per_gpu": int(nrows),
            "hbm": hbm,
            # the timed steps run each prepared statement's literal-specialized kernel (compiled
            # synchronously at its first warmup run, SDO_JIT_SPECIALIZE=sync / _AFTER=1; a server
            # compiles it in the background for statements that repeat); the shape-shared kernels
            # of a first-seen parameterization are reported untimed next to it (--full)
            "kernels": {"timed": f"literal-specialized ({os.environ.get('SDO_JIT_SPECIALIZE')}, after "
                                 f"{os.environ.get('SDO_JIT_SPECIALIZE_AFTER')} run)",
                        "shape_shared_geomean_ms": round(shape_geo, 4) if shape_geo is not None else None},
        }
        print(json.dumps(out), flush=True)
    from spark_druid_olap_amd.parallel.world import shutdown

    shutdown()


if __name__ == "__main__":
    main()
