"""Execute Druid QuerySpecs against device-resident datasource shards.

Per query: lower (engine/lower.py) -> scan on every rank (HIP kernel on GPU, torch reference on
CPU) -> merge partials across ranks (parallel/merge.py, RCCL) -> finalize -> query-type semantics
(GroupBy having/limit/post-aggregations, TopN thresholds, Search, Select paging), i.e. what the
reference gets back from the Druid broker and post-processes in Spark
(``asd/DruidStrategy.scala:284-462``, ``asd/Druid*ResultIterator.scala``).
"""
from __future__ import annotations

import contextlib
import contextvars
import math
import os
import time
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..ops import desc as D
from ..parallel.merge import merge_partials
from ..parallel.world import World, get_world
from ..utils import trace as T
from ..query import spec as S
from ..query.jsfunc import compile_function
from ..segment.datasource import DataSource
from .columns import DictColumn, materialize, take
from .lower import Lowerer, LoweringError, ScanProgram
from .partials import Partials, finalize
from ..parallel import p2p as _p2p
from ..parallel.fault import FAULTS, P2PRetry
from ..utils.cancel import checkpoint


# segment-batched execution overlaps batch j's merge collectives with batch j+1's scan
PIPELINE_MERGE = True
# ... and is chosen by itself across ranks (no segments_per_query asked for) when the dense state
# is large and keyed by a leading time bucket: each batch then merges only its time slice of the
# table while the next batch scans, so all but the last slice's collective hide behind scans.
# Small states are never split: their merge is latency-bound, every batch would pay it again and
# the last one stays exposed anyway.
AUTO_PIPELINE = True
# (below this a merge is latency-bound: never split, whatever the price)
AUTO_PIPELINE_MIN_BYTES = 4 << 20
AUTO_PIPELINE_BATCHES = 3   # (at most: planner/cost.py plan_pipeline prices 2..3)
AUTO_PIPELINE_FORCE = False  # (tests: split whatever the price)
# existence-only group-bys over the key's dictionary domain (engine/dict_exist.py)
DICT_EXIST = True
# thetaSketch aggregators fused into one producer scan with an in-place radix select
# (engine/device_exec.py PreparedTheta) instead of emitting (key, row) of every selected row
THETA_FUSED = True
# GPU-event phase attribution of PreparedQuery.run (scan / merge / gather / finalize)
PHASE_EVENTS = os.environ.get("SDO_PHASE_EVENTS", "0") not in ("0", "")

# Multi-rank result placement.  Set (``results_on_root``) by callers that consume a statement's
# result on rank 0 only -- the benchmark, the SPMD server answering its client: the final groups
# are gathered to rank 0 alone and only rank 0 finalizes, decodes and copies them to the host; the
# other ranks take part in every collective and return an empty result of the same schema.
_ROOT_ONLY: contextvars.ContextVar = contextvars.ContextVar("sdo_results_on_root", default=False)


@contextlib.contextmanager
def results_on_root(flag: bool = True):
    tok = _ROOT_ONLY.set(bool(flag))
    try:
        yield
    finally:
        _ROOT_ONLY.reset(tok)


def root_only_results() -> bool:
    return bool(_ROOT_ONLY.get())


@dataclass
class QueryResult:
    columns: List[str]
    data: Dict[str, np.ndarray]
    query_type: str = "groupBy"
    stats: Dict[str, Any] = field(default_factory=dict)
    paging: Optional[Dict[str, int]] = None

    @property
    def num_rows(self) -> int:
        return len(self.data[self.columns[0]]) if self.columns else 0

    def column(self, name: str) -> np.ndarray:
        return self.data[name]

    def rows(self) -> List[tuple]:
        cols = [materialize(self.data[c]).tolist() for c in self.columns]
        return list(zip(*cols)) if cols else []

    def to_pandas(self):
        import pandas as pd

        data = {c: materialize(self.data[c]) for c in self.columns}
        # (a quantiles column is [groups, fractions]: one array per row)
        return pd.DataFrame({c: (list(v) if v.ndim == 2 else v) for c, v in data.items()}, columns=self.columns)

    def sorted_rows(self) -> List[tuple]:
        return sorted(self.rows(), key=lambda r: tuple((x is None, str(x)) for x in r))


class _SmallDenseRunner:
    """The repeated-execution path of the dashboard shape on one GPU: a groupBy over a small dense
    LDS key space (every headline benchmark query) whose answer is its groups as produced -- no
    HAVING / limitSpec / post-aggregations / sketches needing host work.  Built once per prepared
    query from its layout; each run is the fused reset + scan launch (``run_scan``), the one
    estimate + copy + sync call (``_fetch_small`` through ``finalize``) and the column decode,
    without the general path's merge / HAVING / prune / status plumbing -- each a no-op here but
    together a large share of a 0.1 ms query's host time (``tools/host_floor.py``).  Returns None
    when a run must take the general path (buffers without a fused launch, e.g. right after an
    eviction), so answers never differ."""

    __slots__ = ("pq", "prog", "prep", "qt", "out_cols")

    @staticmethod
    def build(pq: "PreparedQuery") -> Optional["_SmallDenseRunner"]:
        from .device_exec import PreparedScan

        qs = pq.qs
        if pq.world.distributed or qs.queryType != "groupBy" or len(pq.scans) != 1 or pq.window is not None \
                or pq.segments_per_query or PHASE_EVENTS or getattr(pq, "phase_events", False):
            return None
        if getattr(qs, "having", None) is not None or qs.limitSpec is not None or getattr(qs, "postAggregations", None):
            return None
        _, prog, prep = pq.scans[0]
        if not isinstance(prep, PreparedScan) or prep.mode != D.M_DENSE_LDS or prep.touch or prep.pres_bytes:
            return None
        if prog.empty or prog.stored_hll or prog.needs_rows or getattr(prog, "derived_aggs", None) or \
                any(kc.collapse for kc in prog.keys) or pq._dict_exist_plan(prog) is not None:
            return None
        from .partials import SMALL_DENSE_WORDS

        if prog.G * prog.nslots > SMALL_DENSE_WORDS or (prog.nhll and prog.G * (1 << prog.hll_p) > (1 << 26)):
            return None
        r = _SmallDenseRunner()
        r.pq, r.prog, r.prep, r.qt = pq, prog, prep, qs.queryType
        out: List[str] = []  # (exactly _post's identity column list)
        for name in (prog.key_order or [kc.name for kc in prog.keys]):
            if name not in out:
                out.append(name)
        r.out_cols = out + [a.name for a in prog.aggs]
        return r

    def run(self) -> Optional[QueryResult]:
        from ..ops import native

        t0 = time.perf_counter()
        prep = self.prep
        if FAULTS.times > 0:
            FAULTS.maybe_fail("scan", 0)
        checkpoint()
        b = prep.fast_launch()
        if b is None:
            return None
        prog = self.prog
        from .partials import _fetch_small

        hll = [h.view(b.rows, prep.m) for h in b.hll]
        G = b.rows
        host = _fetch_small(b.acc, hll if prog.nhll else [], G, prog.hll_p, None, b.run_args[1:7])
        b.clean = True  # (reset behind the copies: the next run launches the scan alone)
        part = Partials("dense", b.acc, None, hll)
        cols = finalize(prog, part, getattr(self.pq, "out_types", None), prefetched=host)
        res = QueryResult(self.out_cols, {c: cols[c] for c in self.out_cols}, self.qt,
                          {"groups": len(cols["__rows__"]), "exec_ms": (time.perf_counter() - t0) * 1e3})
        self.pq.last_stats = res.stats
        return res


def _py(v):
    if isinstance(v, np.generic):
        return v.item()
    return v


def is_cuda_ds(ds: DataSource) -> bool:
    return ds.device.type == "cuda"


# below this many merged groups HAVING is left to the host (_post re-applies it either way)
HAVING_MIN_ROWS = 4096
# planner group estimate above which a groupBy result streams (iter_pages)
STREAM_MIN_GROUPS = int(os.environ.get("SDO_STREAM_MIN_GROUPS", str(1 << 18)))


class PreparedQuery:
    """A lowered query bound to a shard; run() can be called repeatedly (benchmarks, dashboards)."""

    def __init__(self, engine: "Engine", qs: S.QuerySpec, ds: DataSource, segments_per_query: Optional[int] = None):
        self.engine = engine
        self.qs = qs
        self.ds = ds
        self.world = engine.world
        ctx = getattr(qs, "context", None)
        self.deterministic = bool(engine.deterministic or (ctx is not None and getattr(ctx, "deterministic", None)))
        self.low = Lowerer(ds, world=engine.world, deterministic=self.deterministic,
                           device_match=is_cuda_ds(ds) and bool(engine.use_native))
        self.scans: List[tuple] = []  # (tag, prog, prepared)
        self.segments_per_query = segments_per_query
        self._nbatches: Optional[int] = None   # batch count agreed across ranks (pipelined merge)
        self._pipeline_ok: Optional[bool] = None
        self._slices = None   # per-batch dense-key slices (time-leading keys), agreed across ranks
        self._having_fused: Optional[bool] = None  # HAVING handed to a partitioned scan (decided once)
        self.window: Optional["ShardWindow"] = None
        qt = qs.queryType
        if qt in ("groupBy", "timeseries", "topN"):
            dims = []
            if qt == "groupBy":
                dims = qs.dimensions
            elif qt == "topN":
                dims = [qs.dimension]
            prog = self.low.lower_aggregate(qs.intervals, qs.filter, dims, qs.granularity, qs.aggregations)
            self._full_prog = prog
            if prog.quantiles:
                _check_quantile_refs(qs, {name for name, _, _, _ in prog.quantiles})
            if prog.histograms:
                _check_quantile_refs(qs, {name for name, _, _, _ in prog.histograms}, "fixedBucketsHistogram",
                                     "count per bucket")
            # grouped on the shard key across several ranks: scan this shard's key window only
            self.window = shard_window(prog, ds, self.world)
            if self.window is not None:
                prog = self.window.local
            if not segments_per_query and self.window is None:
                segments_per_query = self._auto_batches(prog, ds)
                self.segments_per_query = segments_per_query
            if segments_per_query:
                # "historical" execution: one partial query per batch of segments, merged here
                for bprog in segment_batches(prog, ds, segments_per_query):
                    self.scans.append(("agg", bprog, self._prepare(bprog)))
                if not self.scans:
                    self.scans.append(("agg", prog, self._prepare(prog)))
            else:
                self.scans.append(("agg", prog, self._prepare(prog)))
        elif qt == "search":
            for dim in (qs.searchDimensions or list(ds.dims)):
                f = _search_filter(dim, qs.query)
                filt = S.LogicalFilterSpec("and", [qs.filter, f]) if qs.filter is not None else f
                prog = self.low.lower_aggregate(qs.intervals, filt, [S.DefaultDimensionSpec(dim, "value")],
                                                qs.granularity, [S.FunctionAggregationSpec("count", "count")])
                self.scans.append((dim, prog, self._prepare(prog)))
        elif qt == "select":
            prog = self.low.lower_mask(qs.intervals, qs.filter)
            self.scans.append(("mask", prog, self._prepare_mask(prog)))
        else:
            raise LoweringError(f"unsupported query type {qt}")
        if segments_per_query and self.world.distributed and self.window is None and PIPELINE_MERGE \
                and qt in ("groupBy", "timeseries", "topN"):
            # the pipelined merge's cross-rank agreements (batch count, per-batch key slices) are
            # collectives: made here, while preparing -- in the same order on every rank -- and never
            # lazily at run time, where two execution slots running this shared prepared query
            # could each issue them on a different process group (server/spmd.py slots)
            self._nbatches = int(self.world.max_float(float(len(self.scans))))
            if self._nbatches > 1:
                self._slices = self._batch_key_slices(self.scans[0][1])

    def _auto_batches(self, prog: ScanProgram, ds: DataSource) -> Optional[int]:
        """Segments per batch for an automatically pipelined multi-rank scan (``AUTO_PIPELINE``), or
        None.  Decided from the layout alone -- the packed key, slots and sketches are the same on
        every rank, the shard's row ranges are not -- plus one agreement that every rank's scan keeps
        dense partials, so all ranks take the same (pipelined or one-merge) collective pattern."""
        if not (AUTO_PIPELINE and PIPELINE_MERGE and self.world.distributed) or \
                self.qs.queryType not in ("groupBy", "timeseries", "topN"):
            return None
        G = int(prog.G)
        lead = [kc for kc in prog.keys if kc.stride * max(1, kc.card) == G]
        if not lead or not getattr(lead[0], "is_timestamp", False) or max(1, lead[0].card) < AUTO_PIPELINE_BATCHES:
            return None
        nbytes = G * max(1, prog.nslots) * 8 + prog.nhll_total * G * (1 << prog.hll_p)
        if nbytes < AUTO_PIPELINE_MIN_BYTES:
            return None
        # priced (planner/cost.py plan_pipeline): only where the hidden merge outweighs the extra
        # batches' table passes -- never over host-staged (gloo) collectives
        from ..planner.cost import plan_pipeline
        from .lower import column_tensor

        rows = sum(max(0, hi - lo) for lo, hi in prog.ranges)
        row_bytes = sum(column_tensor(ds, c).element_size() for c in prog.cols)
        nb = plan_pipeline(nbytes, rows * row_bytes, self.world.size, self.world.backend == "gloo",
                           AUTO_PIPELINE_BATCHES)
        if nb <= 1 and not AUTO_PIPELINE_FORCE:
            return None
        nb = max(nb, AUTO_PIPELINE_BATCHES if AUTO_PIPELINE_FORCE else nb)
        probe = self._prepare(prog)
        # dense table scans only: a batch of a partitioned scan repeats its whole split pipeline (a
        # 2-rank rehearsal of day x ship mode at SF10: 3 partitioned batches 4.3 ms against one scan
        # + one merge 2.8 ms, profiles/r5/rehearsal_auto_pipeline_sf10.txt)
        dense = probe is None or getattr(probe, "mode", None) in (D.M_DENSE_LDS, D.M_DENSE_GLOBAL)
        if -self.world.max_float(-float(dense)) < 1.0:  # (min over ranks)
            return None
        nseg = sum(1 for sg in ds.segments if any(min(hi, sg.row_hi) > max(lo, sg.row_lo) for lo, hi in prog.ranges))
        return max(1, -(-nseg // nb))

    def _prepare(self, prog: ScanProgram):
        if is_cuda_ds(self.ds) and self.engine.use_native:
            from .device_exec import PreparedScan

            # one GPU: a dense HBM table of up to 16 GB beats a hash table over the same key space
            # (TPC-H Q18: 150M order groups); with several ranks dense partials are reduced whole,
            # so huge key spaces stay sparse (hash) and merge by present keys
            local = not self.world.distributed or (self.window is not None and prog is not self._full_prog)
            from ..planner.cost import DENSE_MAX_1GPU

            return PreparedScan(prog, dense_max=DENSE_MAX_1GPU if local else None)
        return None

    def _prepare_mask(self, prog: ScanProgram):
        if is_cuda_ds(self.ds) and self.engine.use_native:
            from .device_exec import PreparedMask

            return PreparedMask(prog)
        return None

    def _placeholder(self, prog, prep) -> Partials:
        """Layout-compatible empty partials for a rank whose scan failed (same collective pattern as
        its peers, so the failure can be agreed on inside the merge)."""
        part = self._placeholder_scan(prog, prep)
        m = 1 << prog.hll_p
        extra = [torch.zeros((part.rows, m), dtype=torch.uint8, device=self.ds.device)
                 for _ in range(prog.nhll_total - len(part.hll))]
        return Partials(part.kind, part.acc, part.keys, list(part.hll) + extra) if extra else part

    def _placeholder_scan(self, prog, prep) -> Partials:
        dev = self.ds.device
        m = 1 << prog.hll_p
        if self.window is not None:
            return self.window.empty(dev)
        if prep is not None:
            from ..ops import desc as D_

            if prep.mode == D_.M_HASH:
                return prep._empty()
            return Partials("dense", _init_acc(prog, prog.G, dev), None,
                            [torch.zeros((prog.G, m), dtype=torch.uint8, device=dev) for _ in range(prog.nhll)])
        if prog.G > (1 << 22):
            return Partials("sparse", torch.empty((0, prog.nslots), dtype=torch.int64, device=dev),
                            torch.zeros(0, dtype=torch.int64, device=dev),
                            [torch.zeros((0, m), dtype=torch.uint8, device=dev) for _ in range(prog.nhll)])
        return Partials("dense", _init_acc(prog, prog.G, dev), None,
                        [torch.zeros((prog.G, m), dtype=torch.uint8, device=dev) for _ in range(prog.nhll)])

    def _scan(self, prog, prep) -> Partials:
        FAULTS.maybe_fail("scan", self.world.rank)
        de = self._dict_exist_plan(prog)
        part = None
        if de is not None:
            from . import dict_exist

            part = dict_exist.run(prog, *de)
        if part is not None:
            pass
        elif prep is not None:
            part = prep.run()
        else:
            from ..ops.reference import run_reference

            part = run_reference(prog)
        if prog.stored_hll and not getattr(prep, "stored_fused", False):
            part = self._merge_stored_hll(prog, part)
        return part

    def _dict_exist_plan(self, prog):
        """engine/dict_exist.py: existence-only group-bys answered over the key's dictionary
        (one GPU / process: the FD tables it reads are shard-local decisions otherwise)."""
        if not DICT_EXIST or self.world.distributed:
            return None
        cache = self.__dict__.setdefault("_dict_exist", {})
        k = id(prog)
        if k not in cache:
            from . import dict_exist

            cache[k] = dict_exist.plan(prog)
        return cache[k]

    def _merge_stored_hll(self, prog, part: Partials) -> Partials:
        """Registers of hyperUnique aggregators over rolled-up sketch metrics: the stored sparse
        sketches of every selected row are unioned into its group's registers (sketch.hip
        hll_merge_stored on the GPU; a torch scatter-max on the CPU).  Appended after the scan's own
        HLL blocks, so merge / estimate / finalize treat them like query-time cardinality."""
        from ..ops.reference import _rows, compute_keys, eval_bexpr

        dev = self.ds.device
        m = 1 << prog.hll_p
        rows = _rows(prog) if not prog.empty else torch.zeros(0, dtype=torch.int64, device=dev)
        if rows.numel():
            rows = rows[eval_bexpr(prog, prog.bexpr, rows)]
        keys = compute_keys(prog, rows)
        if part.kind == "dense":
            slot = keys
        else:  # group key -> row of the sparse partials
            order = torch.argsort(part.keys)
            sk = part.keys[order]
            pos = torch.searchsorted(sk, keys).clamp_(max=max(0, part.rows - 1))
            slot = order[pos] if part.rows else torch.full_like(keys, -1)
            if part.rows and keys.numel() and not bool((sk[pos] == keys).all()):
                raise RuntimeError("stored-sketch rows map to groups missing from the scan's partials")
        hll = list(part.hll)
        for name, metric, filt in prog.stored_hll:
            sk = self.ds.metrics[metric].sketch
            regs = torch.zeros((part.rows, m), dtype=torch.uint8, device=dev)
            r, g = rows, slot
            if filt is not None and rows.numel():
                keep = eval_bexpr(prog, filt, rows)
                r, g = rows[keep], slot[keep]
            if regs.is_cuda and self.engine.use_native:
                from ..ops import native

                native.hll_merge_stored(regs, r, g, sk.offsets, sk.values, prog.hll_p)
            elif r.numel():
                lo, hi = sk.offsets[r], sk.offsets[r + 1]
                cnt = hi - lo
                gi = torch.repeat_interleave(g, cnt)
                first = torch.repeat_interleave(lo - (torch.cumsum(cnt, 0) - cnt), cnt)
                pk = sk.values[torch.arange(int(cnt.sum()), device=dev) + first].to(torch.int64)
                flat = regs.view(-1)
                flat.scatter_reduce_(0, gi * m + ((pk >> 8) & (m - 1)), (pk & 0xFF).to(torch.uint8), reduce="amax")
            hll.append(regs)
        return Partials(part.kind, part.acc, part.keys, hll)

    def _merged(self, prog, prep) -> Partials:
        if not self.world.distributed:
            from ..utils.cancel import checkpoint

            checkpoint()
        part = self._scan(prog, prep)
        disjoint = bool(self.ds.shard_key) and any(k.col == self.ds.shard_key for k in prog.keys)
        return merge_partials(self.world, prog, part, disjoint_keys=disjoint)

    # ------------------------------------------------------------------ run
    def _mark(self, name: str) -> None:
        """GPU phase attribution (``SDO_PHASE_EVENTS=1`` / ``phase_events``): a HIP event recorded
        on the compute stream at each phase boundary, so scan / merge / gather / finalize are the
        device's own times, not host stamps around asynchronous launches."""
        ev = self.__dict__.get("_events")
        if ev is not None and self.ds.device.type == "cuda":
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream(self.ds.device))
            ev.append((name, e))

    def _phase_stats(self) -> Dict[str, float]:
        ev = self.__dict__.get("_events")
        self._events = None
        if not ev:
            return {}
        ev[-1][1].synchronize()
        out: Dict[str, float] = {}
        for (_, a), (name, b) in zip(ev, ev[1:]):
            out["gpu_" + name + "_ms"] = out.get("gpu_" + name + "_ms", 0.0) + a.elapsed_time(b)
        return out

    def run(self) -> QueryResult:
        """Execute once.  A peer-to-peer merge epoch abandoned by every rank (parallel/p2p.py)
        raises ``P2PRetry`` on every rank together: the statement then re-runs with its merges over
        RCCL, so a slow or unreachable peer costs a retry, not a failed statement."""
        res = self._run_once()
        if self.low.dict_match_device:  # id masks the device matcher answered while lowering
            res.stats["dict_match_device"] = self.low.dict_match_device
        return res

    def _run_once(self) -> QueryResult:
        fast = self.__dict__.get("_fast")
        if fast is None:
            fast = self._fast = _SmallDenseRunner.build(self) or False
        if fast:
            res = fast.run()
            if res is not None:
                return res
        try:
            return self._run()
        except P2PRetry:
            _p2p.note_retry(self.world)
            with _p2p.suppressed():
                res = self._run()
            res.stats["p2p_retry"] = 1
            return res

    def _run(self) -> QueryResult:
        t0 = time.perf_counter()
        qt = self.qs.queryType
        self._events = [] if (PHASE_EVENTS or getattr(self, "phase_events", False)) else None
        self._mark("start")
        if qt in ("groupBy", "timeseries", "topN"):
            root_only = self.world.distributed and root_only_results()
            prog, part, t1 = self.run_partials(t0, root_only, check=False)
            t2 = time.perf_counter()
            with T.span("sdo.finalize"):
                if root_only and self.world.rank != 0:
                    # a peer: the root answers; finalize an empty slice for the schema (on the
                    # device: device-resident FD / decode tables must not be copied to the host)
                    from ..parallel.p2p import check_status

                    check_status(part)
                    part = empty_partials(prog, self.ds.device)
                cols = finalize(prog, part, getattr(self, "out_types", None))
            self._mark("finalize")
            t3 = time.perf_counter()
            with T.span("sdo.post"):
                self._theta(self._full_prog, cols)
                self._quantile(self._full_prog, cols)
                tiers = self._distinct(self._full_prog, cols)
                self._moments(self._full_prog, cols)
                co_tiers = self._comoments(self._full_prog, cols)
                ext_tiers = self._extremes(self._full_prog, cols)
                hist_tiers = self._histograms(self._full_prog, cols)
                cm_tiers = self._central_moments(self._full_prog, cols)
                res = self._post(prog, cols)
                if cm_tiers:
                    res.stats["central_moments_device"] = cm_tiers
                if hist_tiers:
                    res.stats["histogram_device"] = hist_tiers
                if tiers:
                    res.stats["distinct_count_device"] = tiers
                if co_tiers:
                    res.stats["comoments_device"] = co_tiers
                if ext_tiers:
                    res.stats["extremes_device"] = ext_tiers
            t4 = time.perf_counter()
            res.stats.update(scan_ms=(t1 - t0) * 1e3, merge_ms=(t2 - t1) * 1e3, finalize_ms=(t3 - t2) * 1e3,
                             post_ms=(t4 - t3) * 1e3)
            res.stats.update(self._phase_stats())
        elif qt == "search":
            res = self._search()
        else:
            res = self._select()
        res.stats["exec_ms"] = (time.perf_counter() - t0) * 1e3
        self.last_stats = res.stats
        return res

    def streamable(self) -> bool:
        """A groupBy whose result is its groups in production order (no HAVING / limitSpec / topN
        ordering on the host, no theta sketches, no re-aggregating key formats) over a key space the
        planner expects to be large: ``iter_pages`` can then decode and ship it a page at a time
        (the reference streams group-by rows from Druid, DruidQueryResultIterator.scala:58-90)."""
        qs = self.qs
        if qs.queryType != "groupBy" or getattr(qs, "having", None) is not None or qs.limitSpec is not None \
                or not self.scans:
            return False
        prog = self.scans[0][1]
        if self._full_prog.needs_rows or any(kc.collapse for kc in prog.keys):
            return False
        return min(float(prog.G), float(getattr(prog, "est_rows", prog.G) or prog.G)) >= STREAM_MIN_GROUPS

    def iter_pages(self, page_rows: int, root_only: Optional[bool] = None):
        """The result as QueryResult pages of at most ``page_rows`` groups: the merged partials stay
        on the device and each page is finalized (decoded, copied to the host) only when it is
        pulled, so host memory holds one page of a million-group answer.  Multi-rank with
        ``root_only``: the groups are gathered to rank 0 alone and the other ranks yield one empty
        page (only the first step issues collectives, so ranks pulling pages in lock step stay
        matched); without it every rank pages through the whole answer."""
        t0 = time.perf_counter()
        root_only = self.world.distributed and (root_only_results() if root_only is None else root_only)
        prog, part, _ = self.run_partials(t0, root_only)
        if root_only and self.world.rank != 0:
            part = empty_partials(prog, self.ds.device)
        part = part.compact()
        # private copies: the slot's scan buffers may be reused by its next execution while the
        # client is still paging through this one
        part = Partials("sparse", part.acc.clone(), part.keys.clone(), [h.clone() for h in part.hll],
                        part.scattered, part.status)
        if part.acc.is_cuda:
            torch.cuda.current_stream(part.acc.device).synchronize()  # pages may be pulled on other threads
        R = part.rows
        out_types = getattr(self, "out_types", None)
        for a in range(0, max(R, 1), page_rows):
            b = min(R, a + page_rows)
            sub = Partials("sparse", part.acc[a:b], part.keys[a:b], [h[a:b] for h in part.hll])
            res = self._post(prog, finalize(prog, sub, out_types))
            res.stats.update(page=a // page_rows, groups_total=R)
            yield res

    def run_partials(self, t0: float, root_only: bool = False, check: bool = True):
        """scan -> merge across ranks -> device HAVING / top-K pruning; (prog, merged partials,
        scan end time).  The partials stay on the device (nested queries consume them there).

        Across ranks, sparse partials are merged into disjoint per-rank slices first; HAVING and the
        top-K prune run on every slice (distributed), and only the survivors are gathered -- to
        rank 0 alone with ``root_only`` (the other ranks then hold an empty slice).

        ``check``: a P2P merge's status words are read here (one host sync) -- the default, for
        consumers that transform the state further (nested levels, grouping sets, paging).
        ``run()`` passes False and reads them with the result's copy in ``finalize``.  An epoch
        every rank abandoned re-runs the scan with the merge over RCCL (parallel/p2p.py)."""
        try:
            out = self._run_partials(t0, root_only)
            if check:
                _p2p.check_status(out[1])
            return out
        except P2PRetry:
            _p2p.note_retry(self.world)
            with _p2p.suppressed():
                out = self._run_partials(t0, root_only)
            _p2p.check_status(out[1])  # (no P2P state: RCCL statuses were checked in the merge)
            return out

    def _run_partials(self, t0: float, root_only: bool):
        _, prog, prep = self.scans[0]
        if self.segments_per_query and self.world.distributed and self.window is None and PIPELINE_MERGE:
            out = self._run_pipelined(prog)
            if out is not None:
                part, t1 = out
                part, hv = self._device_having(prog, part)
                return prog, self._device_prune(prog, part, hv), t1
        err = None
        disjoint = bool(self.ds.shard_key) and any(k.col == self.ds.shard_key for k in self._full_prog.keys) \
            if getattr(self, "_full_prog", None) is not None else False
        if self._having_fused is None:
            self._having_fused = self._fuse_having(prog, prep, disjoint)
            self._fuse_topk(prog, prep, disjoint)
        try:
            with T.span("sdo.scan"):
                checkpoint()  # inside the merge's failure agreement: every rank aborts together
                part = self._scan(prog, prep)
                if len(self.scans) > 1:
                    parts = [part]
                    for _, p_, q_ in self.scans[1:]:
                        checkpoint()  # between segment batches
                        parts.append(self._scan(p_, q_))
                    part = combine_local(prog, parts)
            if self.window is not None:
                part = self.window.to_global(part)
        except Exception as e:  # noqa: BLE001  (peers learn about it in the merge collective)
            if not self.world.distributed:
                raise
            err, part = e, self._placeholder(prog, prep)
        if self.window is not None:
            prog = self._full_prog
        self._mark("scan")
        t1 = time.perf_counter()
        disjoint = bool(self.ds.shard_key) and any(k.col == self.ds.shard_key for k in prog.keys)
        with T.span("sdo.merge"):
            part = merge_partials(self.world, prog, part, disjoint_keys=disjoint, local_error=err,
                                  finish="local" if self.world.distributed else "all", defer_status=True)
        merged = part
        part, hv = self._device_having(prog, part)
        part = self._device_extreme(prog, part, hv)
        part = self._device_prune(prog, part, hv)
        if part is not merged:
            from ..parallel.p2p import check_status

            check_status(merged)  # (a P2P merge's status words: read now, the state was transformed)
        self._mark("merge")
        if part.scattered:
            from ..parallel.merge import gather_groups

            with T.span("sdo.gather"):
                part = gather_groups(self.world, part, root_only, part.status, err)
            if self.world.rank == 0 or not root_only:
                part = self._device_prune(prog, part, hv)  # the union of per-slice supersets
            self._mark("gather")
        return prog, part, t1

    def _run_pipelined(self, prog):
        """Segment-batched execution with each batch's merge overlapping the next batch's scan:
        batch j's dense partials start their collectives (``parallel/merge.start_dense_merge``:
        RCCL runs them on the process group's stream) and batch j+1's kernel is launched behind
        them on the compute stream; the merged batches combine locally at the end.  Ranks agree on
        the batch count once per prepared query (shards hold different segment counts: a rank with
        fewer batches contributes identity partials), so every rank issues the same collectives.
        Returns None -- before any collective -- when the partials are sparse (hash group-by):
        those merge once after a local combine (``run_partials``)."""
        from ..parallel.fault import STATUS_FAILED, STATUS_OK, raise_if_failed
        from ..parallel.merge import start_dense_merge
        from ..utils.cancel import checkpoint

        if self._nbatches is None or self._nbatches <= 1 or self._pipeline_ok is False:
            return None  # (agreed in __init__)
        slices = self._slices
        # one merge in flight: merge j runs while batch j+1 scans, then merge j completes (RCCL:
        # the compute stream waits for it -- no host sync until the final status check)
        done, inflight, err = [], None, None
        for j in range(self._nbatches):
            _, p_, q_ = self.scans[min(j, len(self.scans) - 1)]
            with T.span("sdo.scan"):
                try:
                    if j >= len(self.scans) or err is not None:
                        part = self._placeholder(p_, q_)  # identity (nothing left here) / failed
                    else:
                        checkpoint()
                        part = self._scan(p_, q_)
                except Exception as e:  # noqa: BLE001  (peers learn about it in the merge)
                    err, part = e, self._placeholder(p_, q_)
            if self._pipeline_ok is None:
                # decided from the layout (identical on every rank), before the first collective
                self._pipeline_ok = part.kind == "dense"
                if not self._pipeline_ok:
                    return None
            if inflight is not None:
                done.append(inflight.result())
            if slices is not None:
                # time-leading key: this batch's groups live in one slice of the table, so only
                # that slice crosses the wire (the agreed union over ranks)
                lo, hi = slices[j]
                part = Partials("dense", part.acc[lo:hi], None, [h[lo:hi] for h in part.hll])
            inflight = start_dense_merge(self.world, prog, part, STATUS_FAILED if err else STATUS_OK)
        t1 = time.perf_counter()
        with T.span("sdo.merge"):
            done.append(inflight.result())
            sts = torch.stack([d[1] for d in done]).amax(dim=0).tolist()
            if err is not None or any(sts):
                raise_if_failed(sts, self.world.rank, err)
            if slices is None:
                part = combine_local(prog, [d[0] for d in done])
            else:
                part = self._combine_slices(prog, slices, [d[0] for d in done])
        return part, t1

    def _batch_key_slices(self, prog) -> Optional[List[Tuple[int, int]]]:
        """Dense-table row slice of every segment batch when the leading (most significant) group
        key is a granularity time bucket: a batch's rows span a time range, so its groups occupy
        [bucket(t_min) * stride, (bucket(t_max) + 1) * stride) -- the Druid historical's interval
        partitioning.  Agreed across ranks (min / max over the batch's slices) so every rank sends
        the same collective; None when the layout has no such key."""
        from ..ops.reference import _time_field

        G = prog.G
        lead = [kc for kc in prog.keys if kc.stride * max(1, kc.card) == G]
        if not lead or not getattr(lead[0], "is_timestamp", False) or len(self.scans) < 1:
            return None
        kc = lead[0]
        ds = self.ds
        t = ds.time
        out = torch.zeros((self._nbatches, 2), dtype=torch.int64)
        out[:, 0] = G
        for j, (_, bprog, _) in enumerate(self.scans[: self._nbatches]):
            lo_t, hi_t = None, None
            for a, b in bprog.ranges:
                if b <= a:
                    continue
                mn, mx = torch.aminmax(t[a:b])
                lo_t = int(mn) if lo_t is None else min(lo_t, int(mn))
                hi_t = int(mx) if hi_t is None else max(hi_t, int(mx))
            if lo_t is None:
                continue
            v = torch.tensor([lo_t, hi_t], dtype=torch.int64) * ds.time_unit_ms
            idx = (_time_field(v, kc) - kc.base).clamp(0, max(0, kc.card - 1))
            out[j, 0] = int(idx[0]) * kc.stride
            out[j, 1] = -(int(idx[1]) + 1) * kc.stride
        if self.world.distributed:
            out = self.world.all_reduce(out, "min")
        sl = [(int(a), max(int(a), -int(b))) for a, b in out.tolist()]
        return [(min(a, G), min(b, G)) for a, b in sl]

    def _combine_slices(self, prog, slices, parts: List[Partials]) -> Partials:
        """Assemble the full dense table from per-batch merged slices (slices may overlap at a
        shared time bucket: overlapping rows combine with the slot operators)."""
        from ..parallel.merge import _reduce_stacked

        dev = self.ds.device
        G = prog.G
        acc = torch.tensor([init for _, init in prog.slots], dtype=torch.int64, device=dev).expand(G, -1).clone()
        m = 1 << prog.hll_p
        hll = [torch.zeros((G, m), dtype=torch.uint8, device=dev) for _ in parts[0].hll] if parts else []
        for (lo, hi), p in zip(slices, parts):
            if hi <= lo:
                continue
            acc[lo:hi] = _reduce_stacked(prog, torch.stack([acc[lo:hi], p.acc.to(dev)]))
            for i, h in enumerate(p.hll):
                hll[i][lo:hi] = torch.maximum(hll[i][lo:hi], h.to(dev).view(hi - lo, m))
        return Partials("dense", acc, None, hll)

    def _fuse_having(self, prog: ScanProgram, prep, disjoint: bool) -> bool:
        """Hand a simple HAVING (comparisons of count / integer / double aggregates, AND-ed or OR-ed)
        to a partitioned group-by scan (engine/device_exec.py set_part_having): the aggregation
        kernel then emits only the surviving groups -- TPC-H Q18 keeps ~6K of 150M orders without
        writing or compacting the 150M-row table.  Only where a group's partial is already final:
        one rank, or keys that never span ranks (shard-key groups)."""
        from ..ops import desc as D_

        h = getattr(self.qs, "having", None)
        if h is None or self.qs.queryType != "groupBy" or prog.needs_rows or any(kc.collapse for kc in prog.keys):
            return False
        if prep is None or getattr(prep, "mode", None) != D_.M_PART or len(self.scans) != 1:
            return False
        if self.world.distributed and not disjoint:
            return False
        aggs = {a.name: a for a in prog.aggs}

        def term(x):
            if not isinstance(x, S.ComparisonHavingSpec) or x.type not in ("equalTo", "greaterThan", "lessThan"):
                return None
            a = aggs.get(x.aggregation)
            if a is None or a.slot < 0 or a.kind not in ("count", "sum_i", "sum_f", "min_i", "max_i"):
                return None
            op = {"equalTo": 0, "greaterThan": 1, "lessThan": 2}[x.type]
            return (a.slot, 1 if a.kind == "sum_f" else 0, op, float(10.0 ** a.scale) if a.scale else 1.0,
                    float(x.value))

        if isinstance(h, S.LogicalHavingSpec) and h.type in ("and", "or"):
            terms = [term(y) for y in h.havingSpecs]
            conj = h.type == "and"
        else:
            terms, conj = [term(h)], True
        if not terms or any(t is None for t in terms) or len(terms) > 4:
            return False
        return bool(prep.set_part_having(terms, conj))

    def _fuse_topk(self, prog: ScanProgram, prep, disjoint: bool) -> bool:
        """Hand ORDER BY <aggregate> LIMIT k (one order column, k <= 16) to a partitioned group-by
        scan (engine/device_exec.py set_part_topk): each sub-bucket emits only its candidates -- the
        BI plan's TopVolumeCustomers keeps a few hundred of ~60M (customer, month) groups without
        writing the survivors of its HAVING or radix-selecting over them.  Only where a group's
        partial is final (as ``_fuse_having``), any HAVING went into the kernel too and no window
        pre-filter (``partition_extreme``) runs between the aggregation and the limit."""
        from ..ops import desc as D_

        qs = self.qs
        if prog.needs_rows or any(kc.collapse for kc in prog.keys):
            return False
        if prep is None or getattr(prep, "mode", None) != D_.M_PART or len(self.scans) != 1:
            return False
        if (self.world.distributed and not disjoint) or getattr(self, "partition_extreme", None) is not None:
            return False
        if qs.queryType == "groupBy":
            if getattr(qs, "having", None) is not None and not self._having_fused:
                return False
            ls = qs.limitSpec
            if ls is None or ls.limit is None or not ls.columns or len(ls.columns) != 1:
                return False
            oc = ls.columns[0]
            oc = S.OrderByColumnSpec(oc) if isinstance(oc, str) else oc
            name, desc, limit = oc.dimension, not oc.ascending, int(ls.limit)
        elif qs.queryType == "topN" and isinstance(qs.metric, S.NumericTopNMetricSpec) and len(prog.keys) == 1:
            name, desc, limit = qs.metric.metric, True, int(qs.threshold)
        else:
            return False
        agg = next((a for a in prog.aggs if a.name == name), None)
        if not (1 <= limit <= 16) or agg is None or agg.slot < 0 or \
                agg.kind not in ("count", "sum_i", "sum_f", "min_i", "max_i"):
            return False
        return bool(prep.set_part_topk(limit, agg.slot, agg.kind == "sum_f", desc))

    def _device_having(self, prog: ScanProgram, part: Partials):
        """groupBy havingSpec evaluated over the merged accumulators ON THE DEVICE (TPC-H Q18:
        15M order groups -> a few hundred survive ``sum(l_quantity) > 300``), so only survivors are
        shipped and decoded.  Returns (partials, applied); the host re-applies the same spec in
        ``_post`` (idempotent).  Specs over sketches / post-aggregations stay on the host."""
        h = getattr(self.qs, "having", None)
        if h is None or self.qs.queryType != "groupBy" or prog.needs_rows or any(kc.collapse for kc in prog.keys):
            return part, h is None
        if self._having_fused and part.kind == "sparse" and not part.scattered:
            # the partitioned aggregation already emitted only the groups passing it: a second pass
            # would re-gather every survivor (TopVolumeCustomers: ~50M groups, 9 ms of index_select)
            return part, True
        if part.rows <= HAVING_MIN_ROWS and not part.scattered:
            # (a scattered slice's row count differs per rank: the flag must not, because the
            # post-gather top-K prune on the root trusts it for the union of every rank's slice)
            return part, False
        aggs = {a.name: a for a in prog.aggs}

        def value(name):
            a = aggs.get(name)
            if a is None or a.slot < 0 or a.kind not in ("count", "sum_i", "sum_f", "sum_fx", "min_i", "max_i",
                                                         "min_f", "max_f"):
                return None
            col = part.acc[:, a.slot]
            if a.kind == "sum_f":
                return col.view(torch.float64)
            if a.kind == "sum_fx":
                from .lower import fixed_value

                return fixed_value(col, part.acc[:, a.slot2])
            if a.kind in ("min_f", "max_f"):
                return torch.where(col >= 0, col, col ^ 0x7FFFFFFFFFFFFFFF).view(torch.float64)
            v = col.to(torch.float64)
            return v / (10.0 ** a.scale) if a.scale else v

        def ev(x):
            if isinstance(x, S.ComparisonHavingSpec):
                v = value(x.aggregation)
                if v is None:
                    return None
                c = float(x.value)
                return v == c if x.type == "equalTo" else (v > c if x.type == "greaterThan" else v < c)
            if isinstance(x, S.LogicalHavingSpec):
                ms = [ev(y) for y in x.havingSpecs]
                if any(m is None for m in ms):
                    return None
                out = ms[0]
                for m in ms[1:]:
                    out = (out & m) if x.type == "and" else (out | m)
                return out
            if isinstance(x, S.NotHavingSpec):
                m = ev(x.havingSpec)
                return None if m is None else ~m
            return None

        if part.kind == "dense":
            part = part.compact()
        mask = ev(h)
        if mask is None:
            return part, False
        keep = torch.nonzero(mask).flatten()
        return Partials("sparse", part.acc.index_select(0, keep), part.keys.index_select(0, keep),
                        [x.index_select(0, keep) for x in part.hll], part.scattered, part.status), True

    def _device_extreme(self, prog: ScanProgram, part: Partials, having_done: bool = True) -> Partials:
        """``rank() / dense_rank() OVER (PARTITION BY p ORDER BY metric) = 1`` above this groupBy
        (sql/window.py push_rank_one): keep only the groups whose metric equals their partition's
        minimum (maximum for DESC) -- rank 1 under either function -- ON THE DEVICE, so ~10^5 groups
        are not decoded and shipped to be ranked on the host.  Partition ids are the groups' key
        components (or functionally dependent keys through their FD tables); over per-rank disjoint
        slices the per-partition extremes are all-reduced.  Left to the host when the HAVING could
        not be applied here first, when a metric value is NaN (Spark sorts NaN last), or when the
        partition space is too large for a table."""
        pe = getattr(self, "partition_extreme", None)
        if not pe or self.qs.queryType != "groupBy" or prog.needs_rows or any(kc.collapse for kc in prog.keys):
            return part
        pnames, metric, asc = pe
        agg = next((a for a in prog.aggs if a.name == metric), None)
        if agg is None or agg.slot < 0 or agg.kind not in ("count", "sum_i", "sum_f", "min_i", "max_i", "min_f",
                                                          "max_f") or not having_done:
            return part
        if part.kind == "dense":
            part = part.compact()
        keys = part.keys
        dev = keys.device
        pid = torch.zeros_like(keys)
        npart = 1
        for name in pnames:
            kc = next((k for k in prog.keys if k.name == name), None)
            if kc is not None:
                ids, card = torch.remainder(torch.div(keys, kc.stride, rounding_mode="floor"), max(1, kc.card)), \
                    max(1, kc.card)
            else:
                d = next(((k, det, lut) for k, det, lut in getattr(prog, "derived", ()) if k.name == name), None)
                if d is None:
                    return part
                k, det, lut = d
                kd = prog.keys[det]
                did = torch.remainder(torch.div(keys, kd.stride, rounding_mode="floor"), max(1, kd.card))
                if kd.orig is not None:
                    did = torch.as_tensor(np.asarray(kd.orig, dtype=np.int64), device=dev)[did]
                lut_t = torch.as_tensor(lut).to(device=dev, dtype=torch.int64)
                ids, card = lut_t[did], max(1, int(getattr(k, "card", 0)) or int(lut_t.max().item()) + 1)
            npart *= card
            if npart > (1 << 22):
                return part
            pid = pid * card + ids
        col = part.acc[:, agg.slot]
        if agg.kind == "sum_f":
            v = col.contiguous().view(torch.float64)
        elif agg.kind in ("min_f", "max_f"):
            v = torch.where(col >= 0, col, col ^ 0x7FFFFFFFFFFFFFFF).view(torch.float64)
        else:
            v = col.to(torch.float64)
        nan = torch.isnan(v).any().to(torch.float64).reshape(1) if part.rows else \
            torch.zeros(1, dtype=torch.float64, device=dev)
        if part.scattered and self.world.distributed:
            # per-rank disjoint slices see different values: every rank must take the same branch
            # before the extremes' all-reduce below (one NaN anywhere leaves it to the host)
            nan = self.world.all_reduce(nan, "max")
        if bool(nan.item()):
            return part
        # extremes over the order-preserving int64 image of the f64 values: a native integer atomic
        # per group instead of a float compare-and-swap loop -- the BI MinCost template's five
        # region partitions took 6 ms of CAS retries on five addresses (scatter_reduce on f64);
        # few partitions skip the atomics entirely (one masked reduction each)
        bits = v.contiguous().view(torch.int64)
        o = torch.where(bits >= 0, bits, bits ^ 0x7FFFFFFFFFFFFFFF)
        if npart <= 16:
            big = torch.iinfo(torch.int64).max
            fill = torch.full_like(o, big if asc else -big - 1)
            ext = torch.stack([(torch.where(pid == p_, o, fill).amin() if asc else torch.where(pid == p_, o, fill).amax())
                               for p_ in range(npart)]) if part.rows else torch.full((npart,), 0, dtype=torch.int64,
                                                                                     device=dev)
        else:
            ext = torch.full((npart,), torch.iinfo(torch.int64).max if asc else torch.iinfo(torch.int64).min,
                             dtype=torch.int64, device=dev)
            ext.scatter_reduce_(0, pid, o, reduce="amin" if asc else "amax", include_self=True)
        if part.scattered and self.world.distributed:
            ext = self.world.all_reduce(ext, "min" if asc else "max")
        keep = torch.nonzero(o == ext[pid]).flatten()
        return Partials("sparse", part.acc.index_select(0, keep), keys.index_select(0, keep),
                        [h.index_select(0, keep) for h in part.hll], part.scattered, part.status)

    def _device_prune(self, prog: ScanProgram, part: Partials, having_done: bool = True) -> Partials:
        """ORDER BY <aggregate> LIMIT k (groupBy limitSpec) and numeric topN, applied to the merged
        partials ON THE DEVICE before finalize: keep only groups whose leading sort key ties or
        beats the k-th best (torch.topk), so a million-group query (TPC-H Q3 by o_orderkey) ships and
        decodes a few rows instead of every group.  Ties at the k-th value are all kept, so the host
        ``order_and_limit`` over the survivors gives exactly the unpruned answer."""
        qs = self.qs
        qt = qs.queryType
        if qt == "groupBy":
            ls = qs.limitSpec
            if ls is None or ls.limit is None or ls.limit < 0 or not ls.columns or not having_done:
                return part
            oc = ls.columns[0]
            oc = S.OrderByColumnSpec(oc) if isinstance(oc, str) else oc
            name, desc, limit = oc.dimension, not oc.ascending, int(ls.limit)
        elif qt == "topN" and isinstance(qs.metric, S.NumericTopNMetricSpec) and len(prog.keys) == 1:
            name, desc, limit = qs.metric.metric, True, int(qs.threshold)
        else:
            return part
        if limit <= 0 or part.rows <= max(4 * limit, 4096) or prog.needs_rows or any(kc.collapse for kc in prog.keys):
            return part
        agg = next((a for a in prog.aggs if a.name == name), None)
        if agg is None or agg.slot < 0 or agg.kind not in ("count", "sum_i", "sum_f", "min_i", "max_i"):
            return part
        if part.kind == "dense":
            part = part.compact()
            if part.rows <= max(4 * limit, 4096):
                return part
        if part.acc.is_cuda and self.engine.use_native:
            # device radix select (ops/csrc/post_scan.hip topk_*): keeps every group in or above the
            # k-th best key's 48-bit bucket -- a superset of the top k, no host round trip
            from ..ops import native

            keep = native.topk_keep(part.acc.contiguous(), agg.slot, agg.kind == "sum_f", desc, limit)
        else:
            col = part.acc[:, agg.slot]
            v = col.view(torch.float64) if agg.kind == "sum_f" else col.to(torch.float64)
            key = v if desc else -v
            key = torch.nan_to_num(key, nan=-math.inf)  # NaN sorts last either way
            kth = torch.topk(key, limit, sorted=False).values.min()
            keep = torch.nonzero(key >= kth).flatten()
        return Partials("sparse", part.acc.index_select(0, keep), part.keys.index_select(0, keep),
                        [h.index_select(0, keep) for h in part.hll], part.scattered, part.status)

    # ------------------------------------------------------------------ theta sketches
    def _theta(self, prog: ScanProgram, cols: Dict[str, np.ndarray]) -> None:
        """thetaSketch aggregators (KMV, k = size): per group the k smallest distinct 62-bit hashes of
        the selected rows -- from the rows' value hashes, or from the rows' stored sketches when the
        metric was rolled up at ingest -- selected by a device radix sort; ranks exchange their
        per-group candidates (all-gather) and re-select.  Estimate = (k-1) / (h_k / 2^62), or the
        exact distinct count below k hashes."""
        if not prog.thetas:
            return
        from ..ops.reference import _rows, compute_keys, eval_bexpr
        from ..segment.ingest import theta_hash

        ds = self.ds
        dev = ds.device
        gid_order = np.asarray(cols["__gid__"], dtype=np.int64)
        local = not self.world.distributed
        fused = self._theta_fused(prog, estimates=local)
        if fused is not None:
            for (name, _, size), res in zip(prog.thetas, fused):
                if local:  # one rank: the per-group estimates came back from the select itself
                    ok = (gid_order >= 0) & (gid_order < len(res))
                    cols[name] = np.where(ok, res[np.clip(gid_order, 0, max(0, len(res) - 1))], 0.0)
                else:
                    cols[name] = _kmv_estimates(self._theta_union(res, size), size, gid_order)
            return
        keys = rows = None
        if not prog.empty and dev.type == "cuda" and self.engine.use_native:
            # the JIT scan emits (key, row) of the selected rows (engine/device_exec.py PreparedEmit)
            try:
                em = self.__dict__.get("_emit")
                if em is None:
                    from .device_exec import PreparedEmit

                    em = self._emit = PreparedEmit(prog)
                keys, rows = em.run()
            except RuntimeError:
                keys = rows = None
        if rows is None:
            rows = _rows(prog) if not prog.empty else torch.zeros(0, dtype=torch.int64, device=dev)
            if rows.numel():
                rows = rows[eval_bexpr(prog, prog.bexpr, rows)]
            keys = compute_keys(prog, rows)
        for name, col, size in prog.thetas:
            from .lower import column_tensor

            m = ds.metrics.get(col)
            if m is not None and m.sketch is not None:
                sk = m.sketch
                lo, hi = sk.offsets[rows], sk.offsets[rows + 1]
                cnt = hi - lo
                g = torch.repeat_interleave(keys, cnt)
                first = torch.repeat_interleave(lo - (torch.cumsum(cnt, 0) - cnt), cnt)
                h = sk.values[torch.arange(int(cnt.sum()), device=dev) + first]
            else:
                g, h = keys, theta_hash(column_tensor(ds, col)[rows])
            G = int(prog.G) if 0 < prog.G < (1 << 62) else 0
            pairs = kmv_select(g, h, size, G)
            cols[name] = _kmv_estimates(self._theta_union(pairs, size), size, gid_order)

    def _theta_fused(self, prog: ScanProgram, estimates: bool = False) -> Optional[list]:
        """Per theta aggregator its KMV pairs from the fused producer (engine/device_exec.py
        PreparedTheta), or None where it does not apply (CPU, stored sketches, float columns, wide
        key spaces, an empty shard): the (key, row) emit path then runs.  The choice is per shard
        but issues no collective, so ranks may differ."""
        if prog.empty or self.ds.device.type != "cuda" or not self.engine.use_native or not THETA_FUSED:
            return None
        th = self.__dict__.get("_theta_prep")
        if th is None:
            try:
                from .device_exec import PreparedTheta

                th = PreparedTheta(prog, [c for _, c, _ in prog.thetas], THETA_SELECT_MAX_G)
            except RuntimeError:
                th = False
            self._theta_prep = th
        if th is False:
            return None
        return th.select([size for _, _, size in prog.thetas], estimates=estimates)

    def _theta_union(self, pairs: torch.Tensor, size: int) -> torch.Tensor:
        """Across ranks: every rank's k candidates per group travel to the root only when the answer
        is needed there (results_on_root), else to every rank; the receivers re-select."""
        if not self.world.distributed:
            return pairs
        root_only = root_only_results()
        if root_only:
            got, _ = self.world.gather_varlen(pairs, root=0)
        else:
            got = self.world.all_gather_varlen(pairs)
        if got:
            allp = torch.cat(got)
            return _kmv(_sorted_unique_pairs(allp[:, 0], allp[:, 1]), size)
        return pairs[:0]

    # ------------------------------------------------------------------ order statistics
    def _quantile(self, prog: ScanProgram, cols: Dict[str, np.ndarray]) -> None:
        """``quantiles`` aggregators: per group and fraction the exact order statistic of the
        selected rows' values, a result column [groups, fractions].  On the device the radix rank
        select answers (engine/device_exec.py PreparedQuantile); everywhere else -- CPU, no native
        code, programs or columns the select does not take -- the (group, value) pairs of the
        selected rows are sorted with torch."""
        if not prog.quantiles:
            return
        gid_order = np.asarray(cols["__gid__"], dtype=np.int64)
        fused = self._quantile_fused(prog)
        if fused is not None:
            for (name, _, _, _), res in zip(prog.quantiles, fused):
                cols[name] = res[np.clip(gid_order, 0, max(0, len(res) - 1))]
            return
        from ..ops.reference import _rows, compute_keys, eval_bexpr
        from .lower import column_tensor, dim_numeric_lut

        ds = self.ds
        dev = ds.device
        keys = rows = None
        if not prog.empty and dev.type == "cuda" and self.engine.use_native:
            try:
                em = self.__dict__.get("_emit")
                if em is None:
                    from .device_exec import PreparedEmit

                    em = self._emit = PreparedEmit(prog)
                keys, rows = em.run()
            except RuntimeError:
                keys = rows = None
        if rows is None:
            rows = _rows(prog) if not prog.empty else torch.zeros(0, dtype=torch.int64, device=dev)
            if rows.numel():
                rows = rows[eval_bexpr(prog, prog.bexpr, rows)]
            keys = compute_keys(prog, rows)
        for name, col, fr, interp in prog.quantiles:
            m = ds.metrics.get(col)
            v = column_tensor(ds, col)[rows]
            if m is None:  # a dimension: its dictionary's numeric values
                v = dim_numeric_lut(ds, col)[v.to(torch.int64)]
            v = v.to(torch.float64 if v.dtype.is_floating_point else torch.int64)
            scale = int(m.scale) if m is not None and m.kind == "decimal" else 0
            gids, res = _sorted_quantiles(keys, v, fr, interp, scale)
            at = np.searchsorted(gids, gid_order)
            cols[name] = res[np.clip(at, 0, max(0, len(res) - 1))] if len(res) else \
                np.zeros((len(gid_order), len(fr)), dtype=res.dtype)

    def _quantile_fused(self, prog: ScanProgram) -> Optional[list]:
        """Per quantiles aggregator its values [G, fractions] from the device select, or None where
        it does not apply (CPU, dimensions, wide key spaces, an empty shard, a failed run)."""
        if prog.empty or self.ds.device.type != "cuda" or not self.engine.use_native:
            return None
        qp = self.__dict__.get("_quantile_prep")
        if qp is None:
            try:
                from .device_exec import PreparedQuantile

                qp = PreparedQuantile(prog, prog.quantiles, QUANTILE_SELECT_MAX_G)
            except RuntimeError:
                qp = False
            self._quantile_prep = qp
        if qp is False:
            return None
        try:
            return qp.select()
        except RuntimeError:
            return None

    # ------------------------------------------------------------------ exact distinct counts
    def _distinct(self, prog: ScanProgram, cols: Dict[str, np.ndarray]) -> Optional[str]:
        """``distinctCount`` aggregators: per group the number of distinct non-null dictionary ids of
        the selected rows, an int64 column (0 for groups other aggregators alone produced).  On the
        device the id bitsets answer (engine/device_exec.py PreparedDistinct); everywhere else --
        CPU, no native code, hashed keys, bit matrices beyond the cap -- torch.unique over the packed
        (group, id) pairs does (ops/reference.py distinct_counts).  Returns the tiers the device
        used ("lds", "global", joined by commas), or None."""
        if not prog.distincts:
            return None
        gid_order = np.asarray(cols["__gid__"], dtype=np.int64)
        fused = self._distinct_fused(prog)
        if fused is not None:
            for (name, _, _, _), res in zip(prog.distincts, fused):
                ok = (gid_order >= 0) & (gid_order < len(res))
                cols[name] = np.where(ok, res[np.clip(gid_order, 0, max(0, len(res) - 1))], 0).astype(np.int64)
            return ",".join(self._distinct_prep.tiers)
        from ..ops.reference import _rows, compute_keys, distinct_counts, eval_bexpr
        from .lower import column_tensor, distinct_null_id

        ds = self.ds
        rows = _rows(prog) if not prog.empty else torch.zeros(0, dtype=torch.int64, device=ds.device)
        if rows.numel():
            rows = rows[eval_bexpr(prog, prog.bexpr, rows)]
        keys = compute_keys(prog, rows)
        for name, col, filt, _ in prog.distincts:
            r, k = rows, keys
            if filt is not None and rows.numel():
                keep = eval_bexpr(prog, filt, rows)
                r, k = rows[keep], keys[keep]
            dic = ds.dims[col].dictionary
            gids, cnt = distinct_counts(k, column_tensor(ds, col)[r], len(dic), distinct_null_id(dic))
            gids, cnt = gids.cpu().numpy(), cnt.cpu().numpy().astype(np.int64)
            at = np.clip(np.searchsorted(gids, gid_order), 0, max(0, len(gids) - 1))
            cols[name] = np.where(gids[at] == gid_order, cnt[at], 0).astype(np.int64) if len(gids) else \
                np.zeros(len(gid_order), dtype=np.int64)
        return None

    def _distinct_fused(self, prog: ScanProgram) -> Optional[list]:
        """Per distinctCount aggregator its counts [G] from the device bitsets, or None where they
        do not apply (CPU, hashed or ineligible keys, a bit matrix beyond the cap, an empty shard)."""
        if prog.empty or self.ds.device.type != "cuda" or not self.engine.use_native:
            return None
        dp = self.__dict__.get("_distinct_prep")
        if dp is None:
            try:
                from .device_exec import PreparedDistinct

                dp = PreparedDistinct(prog, prog.distincts)
            except RuntimeError:
                dp = False
            self._distinct_prep = dp
        if dp is False:
            return None
        return dp.count()

    # ------------------------------------------------------------------ variances
    def _moments(self, prog: ScanProgram, cols: Dict[str, np.ndarray]) -> None:
        """``variance`` aggregators: per group the variance of the selected rows' values, a float64
        column (NaN where the group holds too few rows) that HAVING, ordering and post-aggregations
        read like a double sum.  On the native GPU engine the moment sums answer
        (engine/device_exec.py PreparedMoments: exact for long / decimal metrics); everywhere else
        -- CPU, the reference executor, hashed keys, more than QUANTILE_SELECT_MAX_G groups -- a
        centred two-pass in float64 over the selected rows does (ops/reference.py group_variances),
        which is NOT exact."""
        if not prog.moments:
            return
        gid_order = np.asarray(cols["__gid__"], dtype=np.int64)
        fused = self._moments_fused(prog)
        if fused is not None:
            for (name, _, _), res in zip(prog.moments, fused):
                ok = (gid_order >= 0) & (gid_order < len(res))
                cols[name] = np.where(ok, res[np.clip(gid_order, 0, max(0, len(res) - 1))], np.nan)
            return
        from ..ops.reference import _rows, compute_keys, eval_bexpr, group_variances
        from .lower import column_tensor

        ds = self.ds
        rows = _rows(prog) if not prog.empty else torch.zeros(0, dtype=torch.int64, device=ds.device)
        if rows.numel():
            rows = rows[eval_bexpr(prog, prog.bexpr, rows)]
        keys = compute_keys(prog, rows)
        for name, col, ddof in prog.moments:
            m = ds.metrics[col]
            v = column_tensor(ds, col)[rows].to(torch.float64)
            if m.kind == "decimal" and m.scale:
                v = v / (10.0 ** int(m.scale))
            gids, var = group_variances(keys, v, ddof)
            gids, var = gids.cpu().numpy(), var.cpu().numpy()
            at = np.clip(np.searchsorted(gids, gid_order), 0, max(0, len(gids) - 1))
            cols[name] = np.where(gids[at] == gid_order, var[at], np.nan) if len(gids) else \
                np.full(len(gid_order), np.nan)

    def _moments_fused(self, prog: ScanProgram) -> Optional[list]:
        """Per variance aggregator its values [G] from the device moment sums, or None where they do
        not apply (CPU, hashed or ineligible keys, too many groups, an empty shard)."""
        if prog.empty or self.ds.device.type != "cuda" or not self.engine.use_native:
            return None
        mp = self.__dict__.get("_moments_prep")
        if mp is None:
            try:
                from .device_exec import PreparedMoments

                mp = PreparedMoments(prog, prog.moments, QUANTILE_SELECT_MAX_G)
            except RuntimeError:
                mp = False
            self._moments_prep = mp
        if mp is False:
            return None
        return mp.variances()

    # ------------------------------------------------------------------ covariances / correlations
    def _comoments(self, prog: ScanProgram, cols: Dict[str, np.ndarray]) -> Optional[list]:
        """``covariance`` / ``correlation`` aggregators: per group the statistic of the selected
        rows' value pairs, a float64 column (NaN where undefined) that HAVING, ordering and
        post-aggregations read like a double sum.  On the native GPU engine the co-moment sums
        answer (engine/device_exec.py PreparedComoments: exact for long / decimal pairs); everywhere
        else -- CPU, the reference executor, hashed keys, more than QUANTILE_SELECT_MAX_G groups --
        a centred two-pass in float64 does (ops/reference.py group_comoments), which is NOT exact.
        Returns the tier per pair when the device sums answered (the result's ``comoments_device``
        stats entry: without it the answer is the float64 one), else None."""
        if not prog.comoments:
            return None
        gid_order = np.asarray(cols["__gid__"], dtype=np.int64)
        fused = self._comoments_fused(prog)
        if fused is not None:
            for (name, _, _, _), res in zip(prog.comoments, fused):
                ok = (gid_order >= 0) & (gid_order < len(res))
                cols[name] = np.where(ok, res[np.clip(gid_order, 0, max(0, len(res) - 1))], np.nan)
            return list(self._comoments_prep.tiers)
        from ..ops.reference import _rows, compute_keys, eval_bexpr, group_comoments
        from .lower import column_tensor

        ds = self.ds
        rows = _rows(prog) if not prog.empty else torch.zeros(0, dtype=torch.int64, device=ds.device)
        if rows.numel():
            rows = rows[eval_bexpr(prog, prog.bexpr, rows)]
        keys = compute_keys(prog, rows)

        def values(col):
            m = ds.metrics[col]
            v = column_tensor(ds, col)[rows].to(torch.float64)
            return v / (10.0 ** int(m.scale)) if m.kind == "decimal" and m.scale else v

        for name, cx, cy, kind in prog.comoments:
            gids, val = group_comoments(keys, values(cx), values(cy), kind)
            gids, val = gids.cpu().numpy(), val.cpu().numpy()
            at = np.clip(np.searchsorted(gids, gid_order), 0, max(0, len(gids) - 1))
            cols[name] = np.where(gids[at] == gid_order, val[at], np.nan) if len(gids) else \
                np.full(len(gid_order), np.nan)
        return None

    def _comoments_fused(self, prog: ScanProgram) -> Optional[list]:
        """Per covariance / correlation aggregator its values [G] from the device co-moment sums, or
        None where they do not apply (CPU, hashed or ineligible keys, too many groups, an empty
        shard)."""
        if prog.empty or self.ds.device.type != "cuda" or not self.engine.use_native:
            return None
        cp = self.__dict__.get("_comoments_prep")
        if cp is None:
            try:
                from .device_exec import PreparedComoments

                cp = PreparedComoments(prog, prog.comoments, QUANTILE_SELECT_MAX_G)
            except RuntimeError:
                cp = False
            self._comoments_prep = cp
        if cp is False:
            return None
        return cp.values()

    # ------------------------------------------------------------------ max_by / min_by
    def _extremes(self, prog: ScanProgram, cols: Dict[str, np.ndarray]) -> Optional[list]:
        """``maxBy`` / ``minBy`` aggregators: per group the payload of the selected row at the
        lexicographic extreme of (ordering value, row id), an int64 (long payloads) or float64 column
        that HAVING, ordering and post-aggregations read like a sum.  On the native GPU engine the
        packed-key extremes answer (engine/device_exec.py PreparedExtremes); everywhere else -- CPU,
        the reference executor, hashed keys, more than QUANTILE_SELECT_MAX_G groups, ``__time`` over a
        shard that is not time-sorted -- torch takes the same extreme (ops/reference.py
        group_extremes): both are exact.  Returns the tier per ordering column when the device
        answered (the result's ``extremes_device`` stats entry), else None."""
        if not prog.extremes:
            return None
        gid_order = np.asarray(cols["__gid__"], dtype=np.int64)
        fused = self._extremes_fused(prog)
        if fused is not None:
            for (name, _, _, _), res in zip(prog.extremes, fused):
                ok = (gid_order >= 0) & (gid_order < len(res))
                cols[name] = np.where(ok, res[np.clip(gid_order, 0, max(0, len(res) - 1))], 0).astype(res.dtype)
            return list(self._extremes_prep.tiers)
        from ..ops.reference import _rows, compute_keys, eval_bexpr, group_extremes
        from .lower import column_tensor

        ds = self.ds
        rows = _rows(prog) if not prog.empty else torch.zeros(0, dtype=torch.int64, device=ds.device)
        if rows.numel():
            rows = rows[eval_bexpr(prog, prog.bexpr, rows)]
        keys = compute_keys(prog, rows)
        picks = {}  # (ordering column, direction) -> (group keys, the row at the extreme)
        for name, x, by, is_max in prog.extremes:
            if (by, is_max) not in picks:
                y = ds.time[rows] if by == "__time" else column_tensor(ds, by)[rows]
                gids, at = group_extremes(keys, y, rows, is_max)
                picks[(by, is_max)] = (gids.cpu().numpy(), at)
            gids, at = picks[(by, is_max)]
            m = ds.metrics[x]
            val = column_tensor(ds, x)[at].cpu().numpy()
            val = val.astype(np.int64) if m.kind == "long" else val.astype(np.float64)
            if m.kind == "decimal":
                val = val / float(10 ** int(m.scale))
            pos = np.clip(np.searchsorted(gids, gid_order), 0, max(0, len(gids) - 1))
            cols[name] = np.where(gids[pos] == gid_order, val[pos], 0).astype(val.dtype) if len(gids) else \
                np.zeros(len(gid_order), dtype=val.dtype)
        return None

    def _extremes_fused(self, prog: ScanProgram) -> Optional[list]:
        """Per maxBy / minBy aggregator its payloads [G] from the device extremes, or None where they
        do not apply (CPU, hashed or ineligible keys, too many groups, an empty shard, ordering by
        time over a shard that is not time-sorted)."""
        if prog.empty or self.ds.device.type != "cuda" or not self.engine.use_native:
            return None
        ep = self.__dict__.get("_extremes_prep")
        if ep is None:
            try:
                from .device_exec import PreparedExtremes

                ep = PreparedExtremes(prog, prog.extremes, QUANTILE_SELECT_MAX_G)
            except RuntimeError:
                ep = False
            self._extremes_prep = ep
        if ep is False:
            return None
        return ep.values()

    # ------------------------------------------------------------------ fixed-bucket histograms
    def _histograms(self, prog: ScanProgram, cols: Dict[str, np.ndarray]) -> Optional[list]:
        """``fixedBucketsHistogram`` aggregators: per group the int64 counts [below, c_0 .. c_{B-1},
        above] of the selected rows' values, a result column [groups, B + 2] like a quantiles
        column.  On the native GPU engine the HIP bucket counts answer (engine/device_exec.py
        PreparedHistogram); everywhere else -- CPU, the reference executor, hashed keys, more than
        QUANTILE_SELECT_MAX_G groups -- torch counts against the same thresholds (ops/reference.py
        group_histogram): both are exact.  Returns the tier per accumulation when the device
        answered (the result's ``histogram_device`` stats entry), else None."""
        if not prog.histograms:
            return None
        gid_order = np.asarray(cols["__gid__"], dtype=np.int64)
        fused = self._histograms_fused(prog)
        if fused is not None:
            for (name, _, _, _), res in zip(prog.histograms, fused):
                cols[name] = res[np.clip(gid_order, 0, max(0, len(res) - 1))]
            return list(self._histogram_prep.tiers)
        from ..ops import buckets
        from ..ops.reference import _rows, compute_keys, eval_bexpr, group_histogram
        from .lower import column_tensor

        ds = self.ds
        rows = _rows(prog) if not prog.empty else torch.zeros(0, dtype=torch.int64, device=ds.device)
        if rows.numel():
            rows = rows[eval_bexpr(prog, prog.bexpr, rows)]
        keys = compute_keys(prog, rows)
        mats = {}  # (column, thresholds) -> (group keys, counts)
        for name, c, edges, mode in prog.histograms:
            m = ds.metrics[c]
            thr = buckets.bucket_thresholds(edges, m.kind, int(m.scale))
            if (c, thr.tobytes()) not in mats:
                gids, cnt = group_histogram(keys, column_tensor(ds, c)[rows], thr)
                mats[(c, thr.tobytes())] = (gids.cpu().numpy(), cnt.cpu().numpy())
            gids, cnt = mats[(c, thr.tobytes())]
            pos = np.clip(np.searchsorted(gids, gid_order), 0, max(0, len(gids) - 1))
            hit = gids[pos] == gid_order if len(gids) else np.zeros(len(gid_order), dtype=bool)
            cols[name] = buckets.apply_mode(np.where(hit[:, None], cnt[pos], 0), mode) if len(gids) else \
                np.zeros((len(gid_order), len(thr) + 1), dtype=np.int64)
        return None

    def _histograms_fused(self, prog: ScanProgram) -> Optional[list]:
        """Per fixedBucketsHistogram aggregator its counts [G, B + 2] from the device, or None where
        it does not apply (CPU, hashed or ineligible keys, too many groups or counters, an empty
        shard)."""
        if prog.empty or self.ds.device.type != "cuda" or not self.engine.use_native:
            return None
        ep = self.__dict__.get("_histogram_prep")
        if ep is None:
            try:
                from .device_exec import PreparedHistogram

                ep = PreparedHistogram(prog, prog.histograms, QUANTILE_SELECT_MAX_G)
            except RuntimeError:
                ep = False
            self._histogram_prep = ep
        if ep is False:
            return None
        return ep.counts()

    # ------------------------------------------------------------------ skewness / kurtosis
    def _central_moments(self, prog: ScanProgram, cols: Dict[str, np.ndarray]) -> Optional[list]:
        """``skewness`` / ``kurtosis`` aggregators: per group the statistic of the selected rows'
        values, a float64 column (NaN where the rows hold one value only) that HAVING, ordering and
        post-aggregations read like a double sum.  On the native GPU engine the power sums answer
        (engine/device_exec.py PreparedCentralMoments: exact for long / decimal metrics of a range
        below 2^32); everywhere else -- CPU, the reference executor, hashed keys, more than
        QUANTILE_SELECT_MAX_G groups -- a centred two-pass in float64 does (ops/reference.py
        group_central_moments), which is NOT exact.  Returns the tier per distinct column when the
        device sums answered (the result's ``central_moments_device`` stats entry), else None."""
        if not prog.central_moments:
            return None
        gid_order = np.asarray(cols["__gid__"], dtype=np.int64)
        fused = self._central_moments_fused(prog)
        if fused is not None:
            for (name, _, _), res in zip(prog.central_moments, fused):
                ok = (gid_order >= 0) & (gid_order < len(res))
                cols[name] = np.where(ok, res[np.clip(gid_order, 0, max(0, len(res) - 1))], np.nan)
            return list(self._central_moments_prep.tiers)
        from ..ops.reference import _rows, compute_keys, eval_bexpr, group_central_moments
        from .lower import column_tensor

        ds = self.ds
        rows = _rows(prog) if not prog.empty else torch.zeros(0, dtype=torch.int64, device=ds.device)
        if rows.numel():
            rows = rows[eval_bexpr(prog, prog.bexpr, rows)]
        keys = compute_keys(prog, rows)
        for name, col, order in prog.central_moments:
            # (both statistics are invariant under a decimal's scale)
            gids, val = group_central_moments(keys, column_tensor(ds, col)[rows].to(torch.float64), order)
            gids, val = gids.cpu().numpy(), val.cpu().numpy()
            at = np.clip(np.searchsorted(gids, gid_order), 0, max(0, len(gids) - 1))
            cols[name] = np.where(gids[at] == gid_order, val[at], np.nan) if len(gids) else \
                np.full(len(gid_order), np.nan)
        return None

    def _central_moments_fused(self, prog: ScanProgram) -> Optional[list]:
        """Per skewness / kurtosis aggregator its values [G] from the device power sums, or None
        where they do not apply (CPU, hashed or ineligible keys, too many groups, an empty shard)."""
        if prog.empty or self.ds.device.type != "cuda" or not self.engine.use_native:
            return None
        cp = self.__dict__.get("_central_moments_prep")
        if cp is None:
            try:
                from .device_exec import PreparedCentralMoments

                cp = PreparedCentralMoments(prog, prog.central_moments, QUANTILE_SELECT_MAX_G)
            except RuntimeError:
                cp = False
            self._central_moments_prep = cp
        if cp is False:
            return None
        return cp.values()

    # ------------------------------------------------------------------ post processing
    def _post(self, prog: ScanProgram, cols: Dict[str, np.ndarray]) -> QueryResult:
        qs = self.qs
        qt = qs.queryType
        n = len(cols["__rows__"])
        out_cols: List[str] = []
        if qt == "timeseries":
            if prog.keys and prog.keys[0].is_timestamp:
                out_cols.append("timestamp")
            elif n == 0:
                # Druid timeseries with granularity all returns one row even when nothing matched
                for a in prog.aggs:
                    cols[a.name] = np.zeros(1, dtype=np.int64 if a.out_type == "long" else np.float64)
                cols["__rows__"] = np.zeros(1, dtype=np.int64)
                n = 1
        for name in (prog.key_order or [kc.name for kc in prog.keys]):
            if name not in out_cols:
                out_cols.append(name)
        for a in prog.aggs:
            out_cols.append(a.name)
        for pa in (getattr(qs, "postAggregations", None) or []):
            cols[pa.name] = np.asarray(eval_postagg(pa, cols, n), dtype=np.float64) * np.ones(n)
            out_cols.append(pa.name)
        having = getattr(qs, "having", None)
        identity = having is None and qt != "topN" and not (qt == "groupBy" and qs.limitSpec is not None) \
            and not (qt == "timeseries" and "timestamp" in cols)
        if identity:  # result order as produced: no index array, no copies (million-group results)
            return QueryResult(out_cols, {c: cols[c] for c in out_cols}, qt, {"groups": n})
        idx = np.arange(n)
        if having is not None:
            idx = idx[eval_having(having, cols)[idx]]
        if qt == "topN":
            idx = self._topn_order(cols, idx, prog)
        elif qt == "groupBy" and qs.limitSpec is not None:
            idx = order_and_limit(cols, idx, qs.limitSpec.columns, qs.limitSpec.limit)
        elif qt == "timeseries" and "timestamp" in cols:
            idx = idx[np.argsort(cols["timestamp"][idx], kind="stable")]
            if getattr(qs, "descending", False):
                idx = idx[::-1]
        data = {c: take(cols[c], idx) for c in out_cols}
        return QueryResult(out_cols, data, qt, {"groups": n})

    def _topn_order(self, cols, idx, prog) -> np.ndarray:
        qs = self.qs
        metric = qs.metric
        invert = False
        while isinstance(metric, S.InvertedTopNMetricSpec):
            invert = not invert
            metric = metric.metric
        dimname = (prog.key_order or [kc.name for kc in prog.keys])[-1]
        if isinstance(metric, S.NumericTopNMetricSpec):
            key = np.asarray(cols[metric.metric], dtype=np.float64)[idx]
            order = np.argsort(key if invert else -key, kind="stable")
        else:
            vals = materialize(take(cols[dimname], idx))
            if isinstance(metric, S.AlphaNumericTopNMetricSpec):
                skey = [(_alnum_key(v)) for v in vals]
            else:
                skey = [(v is None, str(v)) for v in vals]
            order = np.array(sorted(range(len(idx)), key=lambda i: skey[i], reverse=invert), dtype=np.int64)
            prev = getattr(metric, "previousStop", None)
            if prev is not None:
                order = np.array([i for i in order if str(vals[i]) > str(prev)], dtype=np.int64)
        idx = idx[order] if len(order) else idx[:0]
        if "timestamp" in cols:
            ts = cols["timestamp"][idx]
            keep, seen = [], {}
            for j, t in enumerate(ts):
                c = seen.get(t, 0)
                if c < qs.threshold:
                    keep.append(j)
                    seen[t] = c + 1
            idx = idx[np.array(keep, dtype=np.int64)] if keep else idx[:0]
            idx = idx[np.argsort(cols["timestamp"][idx], kind="stable")]
            return idx
        return idx[: qs.threshold]

    def _search(self) -> QueryResult:
        qs = self.qs
        dims, vals, counts = [], [], []
        for dim, prog, prep in self.scans:
            cols = finalize(prog, self._merged(prog, prep))
            v = cols["value"]
            c = cols["count"]
            for i in range(len(v)):
                if v[i] is None:
                    continue
                dims.append(dim)
                vals.append(v[i])
                counts.append(int(c[i]))
        order = sorted(range(len(vals)), key=lambda i: (str(vals[i]), dims[i]))
        if qs.sort and str(qs.sort.get("type", "")).lower() == "strlen":
            order = sorted(range(len(vals)), key=lambda i: (len(str(vals[i])), str(vals[i])))
        order = order[: qs.limit]
        data = {"dimension": np.array([dims[i] for i in order], dtype=object),
                "value": np.array([vals[i] for i in order], dtype=object),
                "count": np.array([counts[i] for i in order], dtype=np.int64)}
        return QueryResult(["dimension", "value", "count"], data, "search")

    def selected_rows(self) -> torch.Tensor:
        """This shard's row ids passing the Select filter (device, ascending), computed once per
        prepared query -- datasources are immutable, so every later page is a slice + gather, not
        a re-scan (the reference re-issues the Select per page, asd/DruidSelectResultIterator.scala
        116-137).  Compacted by the mask kernel + compact_rows (O(selected) memory)."""
        rows = getattr(self, "_sel_rows", None)
        if rows is None:
            from ..ops.reference import run_reference_mask

            _, prog, prep = self.scans[0]
            rows = prep.run() if prep is not None else run_reference_mask(prog)
            if self.qs.descending:
                rows = rows.flip(0)
            self._sel_rows = rows
        return rows

    def run_page(self, paging: Optional[S.PagingSpec] = None) -> QueryResult:
        """One Select page (``paging`` overrides the spec's pagingSpec): the cursor protocol of
        Druid's select query -- pagingIdentifiers map each shard (``<datasource>_<rank>``) to the
        last row offset returned."""
        t0 = time.perf_counter()
        res = self._select(paging)
        res.stats["exec_ms"] = (time.perf_counter() - t0) * 1e3
        return res

    def _select(self, paging: Optional[S.PagingSpec] = None) -> QueryResult:
        from .lower import column_tensor

        qs = self.qs
        ds = self.ds
        rows = self.selected_rows()
        paging = paging or qs.pagingSpec or S.PagingSpec()
        ids_in = paging.pagingIdentifiers or {}
        thr = int(paging.threshold)
        W = self.world.size if self.world.distributed else 1

        def start_of(r):
            k = f"{ds.name}_{r}"
            return int(ids_in[k]) + 1 if k in ids_in else 0

        start = start_of(self.world.rank if W > 1 else 0)
        page = rows[start: start + thr]
        dims = qs.dimensions or list(ds.dims)
        mets = qs.metrics or list(ds.metrics)
        # one int64 block per page: time, dimension ids, metric bit patterns -> a single device
        # gather across ranks (C4: per-GPU compaction, then a GatherV of the page)
        parts = [ds.time[page].to(torch.int64)]
        parts += [column_tensor(ds, d)[page].to(torch.int64) for d in dims]
        for m in mets:
            v = ds.metrics[m].data[page]
            parts.append(v.contiguous().view(torch.int64) if v.dtype == torch.float64 else v.to(torch.int64))
        block = torch.stack(parts, dim=1) if page.numel() else \
            torch.zeros((0, len(parts)), dtype=torch.int64, device=rows.device)
        if W > 1:
            blocks = self.world.all_gather_varlen(block)
            ns = [int(x.shape[0]) for x in blocks]
            block = torch.cat(blocks)
        else:
            ns = [int(block.shape[0])]
        host = block.cpu().numpy()
        data: Dict[str, np.ndarray] = {"timestamp": host[:, 0] * ds.time_unit_ms}
        for j, d in enumerate(dims):
            data[d] = DictColumn(host[:, 1 + j], ds.dims[d].dictionary)
        for j, m in enumerate(mets):
            mc = ds.metrics[m]
            v = host[:, 1 + len(dims) + j]
            if mc.data.dtype == torch.float64:
                v = v.view(np.float64)
            elif mc.kind == "decimal" and mc.scale:
                v = v.astype(np.float64) / (10.0 ** mc.scale)
            data[m] = v
        cols = ["timestamp"] + list(dims) + list(mets)
        nxt = {f"{ds.name}_{r}": start_of(r) + ns[r] - 1 for r in range(W)}
        return QueryResult(cols, data, "select", {"rows": int(rows.numel())}, paging=nxt)


class ShardWindow:
    """Grouping on the datasource's shard key across ranks: every rank only holds its own key range
    (TPC-H orders are range-partitioned on ``o_orderkey``), so the scan accumulates into a dense
    table of the LOCAL key window -- the same table size as one GPU instead of an N-times larger
    key space that would force the hash table -- and the partial keys are rebased to the global
    packed layout before the (disjoint, concatenating) merge.  The reference's equivalent is the
    historical query over a server's own segments (``sd/DruidRDD.scala:62-84``)."""

    MIN_SAVING = 4  # only when the local window is at most 1/4 of the global key space

    def __init__(self, glob: ScanProgram, local: ScanProgram):
        self.glob = glob
        self.local = local

    def empty(self, dev) -> Partials:
        m = 1 << self.glob.hll_p
        return Partials("sparse", torch.empty((0, self.glob.nslots), dtype=torch.int64, device=dev),
                        torch.zeros(0, dtype=torch.int64, device=dev),
                        [torch.zeros((0, m), dtype=torch.uint8, device=dev) for _ in range(self.glob.nhll)])

    def to_global(self, part: Partials) -> Partials:
        sp = part.compact()
        g = sp.keys.to(torch.int64)
        out = torch.zeros_like(g)
        for kl, kg in zip(self.local.keys, self.glob.keys):
            ids = torch.remainder(torch.div(g, kl.stride, rounding_mode="floor"), max(1, kl.card)) + kl.base
            out += (ids - kg.base) * kg.stride
        return Partials("sparse", sp.acc, out, sp.hll)


_ID_RANGE_CACHE: Dict[tuple, tuple] = {}


def shard_id_range(ds: DataSource, col: str) -> tuple:
    """(min, max) dictionary id of ``col`` on this shard (cached per datasource + column)."""
    from .lower import column_tensor

    key = (id(ds), col)
    hit = _ID_RANGE_CACHE.get(key)
    if hit is not None and hit[0] is ds:
        return hit[1]
    t = column_tensor(ds, col)
    if t.numel() == 0:
        r = (0, -1)
    else:
        lo, hi = torch.aminmax(t)
        r = (int(lo), int(hi))
    _ID_RANGE_CACHE[key] = (ds, r)
    return r


def shard_window(prog: ScanProgram, ds: DataSource, world: World) -> Optional[ShardWindow]:
    import copy

    # (everything up to the agreement below depends on the plan only -- identical on every rank)
    if world is None or not world.distributed or not ds.shard_key or prog.needs_rows:
        return None
    idx = next((i for i, kc in enumerate(prog.keys)
                if kc.kind == D.K_ID and kc.col == ds.shard_key and kc.orig is None and kc.base == 0), None)
    if idx is None or prog.G < int(os.environ.get("SDO_SHARD_WINDOW_MIN_G", 1 << 16)):
        return None
    lo, hi = shard_id_range(ds, ds.shard_key)
    card = max(1, hi - lo + 1)
    # the window changes this rank's partials from the dense global table to rebased sparse groups,
    # and the merge's collective pattern follows the partials' layout: every rank must window, or
    # none.  A shard's own key range decides locally (4 range shards hold ~1/4 of the keys each,
    # right at MIN_SAVING), so the ranks agree -- one small all-gather, in broadcast order at
    # prepare time.  (A rank whose filter selects nothing still windows: its empty local table
    # compacts to no groups.)
    ok = card * ShardWindow.MIN_SAVING <= prog.keys[idx].card
    if world.max_float(0.0 if ok else 1.0) != 0.0:
        return None
    keys = [copy.copy(kc) for kc in prog.keys]
    keys[idx].base, keys[idx].card = max(0, lo), card
    G = 1
    for kc in reversed(keys):
        kc.stride = G
        G *= max(1, kc.card)
    import dataclasses

    local = dataclasses.replace(prog, keys=keys, G=G)
    return ShardWindow(prog, local)


def empty_partials(prog: ScanProgram, dev) -> Partials:
    """No groups, in the program's layout (a peer's share of a result answered on rank 0)."""
    m = 1 << prog.hll_p
    return Partials("sparse", torch.empty((0, prog.nslots), dtype=torch.int64, device=dev),
                    torch.zeros(0, dtype=torch.int64, device=dev),
                    [torch.zeros((0, m), dtype=torch.uint8, device=dev) for _ in range(prog.nhll_total)])


def _init_acc(prog: ScanProgram, rows: int, dev) -> torch.Tensor:
    init = torch.tensor([int(i) for _, i in prog.slots], dtype=torch.int64, device=dev)
    return init.reshape(1, -1).repeat(rows, 1)


def segment_batches(prog: ScanProgram, ds: DataSource, per_query: int) -> List[ScanProgram]:
    """Split a lowered scan into per-segment-batch scans (same key/slot layout, row ranges cut to
    each batch of ``per_query`` consecutive segments), like the reference's HistoricalPartitions
    sliding over a server's (segment, interval) list (``sd/DruidRDD.scala:244-269``)."""
    import dataclasses

    if prog.empty:
        return []
    segs = [sg for sg in ds.segments
            if any(min(hi, sg.row_hi) > max(lo, sg.row_lo) for lo, hi in prog.ranges)]
    out = []
    per_query = max(1, int(per_query))
    for i in range(0, len(segs), per_query):
        batch = segs[i:i + per_query]
        spans = _merge_spans(sorted((sg.row_lo, sg.row_hi) for sg in batch))
        ranges = []
        for lo, hi in prog.ranges:
            for a, b in spans:
                x, y = max(lo, a), min(hi, b)
                if y > x:
                    ranges.append((x, y))
        if not ranges:
            continue
        ranges = _merge_spans(sorted(ranges))
        if len(ranges) > D.MAX_RANGES:
            raise ValueError("segment batch spans too many row ranges")
        out.append(dataclasses.replace(prog, ranges=ranges))
    return out


def _merge_spans(spans):
    out = []
    for a, b in spans:
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def combine_local(prog: ScanProgram, parts: List[Partials]) -> Partials:
    """Merge partial aggregates of one query computed over disjoint row sets (same layout)."""
    from ..engine.partials import merge_sparse
    from ..parallel.merge import _reduce_stacked

    if all(p.kind == "dense" for p in parts):
        acc = _reduce_stacked(prog, torch.stack([p.acc for p in parts]))
        hll = [torch.stack([p.hll[i] for p in parts]).amax(dim=0) for i in range(len(parts[0].hll))]
        return Partials("dense", acc, None, hll)
    return merge_sparse([p.compact() for p in parts], prog.slots)


def _sorted_unique_pairs(g: torch.Tensor, h: torch.Tensor, groups: int = 0, hmax: int = -1) -> torch.Tensor:
    """Distinct (group, hash) pairs sorted by group then hash: two stable device radix sorts (LSD)
    instead of a lexicographic unique over rows -- or ONE sort of ``g << s | h`` when every hash is
    below ``hmax`` < 2^s and the ``groups`` fit the bits above (a theta select's candidates: the
    per-group bounds are far below 2^62)."""
    if g.numel() == 0:
        return torch.zeros((0, 2), dtype=torch.int64, device=g.device)
    gb = max(1, int(groups - 1).bit_length()) if groups > 0 else 64
    if 0 <= hmax and gb < 63 and hmax <= (1 << (63 - gb)):
        sh = 63 - gb
        key = torch.sort((g.to(torch.int64) << sh) | h.to(torch.int64)).values
        keep = torch.ones(key.numel(), dtype=torch.bool, device=key.device)
        keep[1:] = key[1:] != key[:-1]
        key = key[keep]
        return torch.stack([key >> sh, key & ((1 << sh) - 1)], dim=1)
    o = torch.sort(h, stable=True).indices
    o = o[torch.sort(g[o], stable=True).indices]
    g, h = g[o].to(torch.int64), h[o].to(torch.int64)
    keep = torch.ones(g.numel(), dtype=torch.bool, device=g.device)
    keep[1:] = (g[1:] != g[:-1]) | (h[1:] != h[:-1])
    return torch.stack([g[keep], h[keep]], dim=1)


def _kmv_estimates(pairs: torch.Tensor, k: int, gid_order: np.ndarray) -> np.ndarray:
    """Theta estimate per group of ``gid_order`` from sorted per-group KMV pairs (vectorized)."""
    if pairs.numel() == 0:
        return np.zeros(len(gid_order), dtype=np.float64)
    g = pairs[:, 0]
    ug, counts = torch.unique_consecutive(g, return_counts=True)
    start = torch.cumsum(counts, 0) - counts
    kth = pairs[(start + min(k, 1 << 62) - 1).clamp(max=g.numel() - 1), 1].to(torch.float64)
    est = torch.where(counts < k, counts.to(torch.float64), (k - 1) / (kth / float(1 << 62)))
    ug, est = ug.cpu().numpy(), est.cpu().numpy()
    pos = np.searchsorted(ug, gid_order)
    ok = (pos < len(ug)) & (ug[np.minimum(pos, len(ug) - 1)] == gid_order)
    return np.where(ok, est[np.minimum(pos, len(ug) - 1)], 0.0)


THETA_SELECT_MAX_G = 4096  # groups the device radix select handles (histogram G x 2^bits u32)
QUANTILE_SELECT_MAX_G = 1 << 16  # groups the device rank select handles (state rows G x targets)


def _check_quantile_refs(qs, names, what: str = "quantiles", per: str = "value per fraction") -> None:
    """A quantiles column holds one value per fraction (a fixedBucketsHistogram column one count per
    bucket): HAVING, limitSpec ordering, a topN metric or a post-aggregation cannot read it as a
    number (SQL projects the fractions out first)."""
    import dataclasses

    def walk(x):
        if isinstance(x, str):
            if x in names:
                raise LoweringError(f"the {what} aggregator {x!r} holds one {per}: it cannot be "
                                    "read by having / limitSpec / metric / postAggregations")
        elif isinstance(x, (list, tuple)):
            for y in x:
                walk(y)
        elif dataclasses.is_dataclass(x):
            for f in dataclasses.fields(x):
                walk(getattr(x, f.name))

    for attr in ("having", "limitSpec", "metric", "postAggregations"):
        walk(getattr(qs, attr, None))


def _sorted_quantiles(g: torch.Tensor, v: torch.Tensor, fractions, interpolate: bool, scale: int):
    """Order statistics by sorting: (group ids ascending, values [groups, fractions]) of the
    (group, value) pairs -- ``v`` int64 (a decimal's unscaled digits) or float64.  Interpolated:
    lo + (hi - lo) * (pos - floor(pos)) at pos = p (n-1), float64, a decimal's scale applied to lo
    and hi; else the element at rank max(0, ceil(p n) - 1) (a decimal as float64)."""
    nf = len(fractions)
    is_f = v.dtype.is_floating_point
    if not g.numel():
        return np.zeros(0, dtype=np.int64), np.zeros((0, nf), dtype=np.float64 if (interpolate or is_f or scale) else np.int64)
    o1 = torch.sort(v, stable=True).indices
    o2 = torch.sort(g[o1], stable=True).indices
    order = o1[o2]
    gs, vs = g[order], v[order]
    gids, cnt = torch.unique_consecutive(gs, return_counts=True)
    start = torch.cumsum(cnt, 0) - cnt
    n = cnt.to(torch.float64)
    p = torch.tensor(list(fractions), dtype=torch.float64, device=v.device)

    def value(x):
        x = x.to(torch.float64)
        return x / (10.0 ** scale) if scale else x

    if interpolate:
        pos = p[None, :] * (n[:, None] - 1.0)
        lo_r = torch.floor(pos)
        lo = value(vs[start[:, None] + lo_r.to(torch.int64)])
        hi = value(vs[start[:, None] + torch.ceil(pos).to(torch.int64)])
        gm = pos - lo_r  # (anchored at the nearer rank: no cancellation error across a sign change)
        res = torch.where(gm >= 0.5, hi - (hi - lo) * (1.0 - gm), lo + (hi - lo) * gm)
    else:
        r = torch.clamp(torch.ceil(p[None, :] * n[:, None]) - 1.0, min=0.0).to(torch.int64)
        res = vs[start[:, None] + r]
        if scale:
            res = value(res)
    return gids.cpu().numpy(), res.cpu().numpy()


def kmv_select(g: torch.Tensor, h: torch.Tensor, k: int, G: int) -> torch.Tensor:
    """Per group the k smallest distinct hashes, as sorted unique (group, hash) pairs.  On the GPU a
    radix select per group (ops/csrc/sketch.hip theta_*) keeps ~2k candidates per group before the
    sort -- a 600M-row scan's pairs never reach the sort; groups whose candidates hold fewer than k
    distinct hashes although their bound cut some pairs off (duplicate-heavy groups) are selected
    again with a 4x larger target.  Elsewhere (CPU, huge key spaces) the full sort."""
    if g.numel() == 0:
        return torch.zeros((0, 2), dtype=torch.int64, device=g.device)
    if not (g.is_cuda and 0 < G <= THETA_SELECT_MAX_G):
        return _kmv(_sorted_unique_pairs(g, h), k)
    from ..ops import native

    g = g.to(torch.int64).contiguous()
    h = h.to(torch.int64).contiguous()
    bits = 16 if G <= 256 else 12
    target = torch.full((G,), 2 * k, dtype=torch.int64, device=g.device)
    for _ in range(6):
        cg, ch, bound = native.theta_select(g, h, G, target, bits)
        pairs = _sorted_unique_pairs(cg, ch)
        distinct = torch.bincount(pairs[:, 0], minlength=G) if pairs.numel() else torch.zeros(G, dtype=torch.int64,
                                                                                               device=g.device)
        short = (distinct < k) & (bound < (1 << 62))
        if not bool(short.any()):
            return _kmv(pairs, k)
        target = torch.where(short, target * 4, target)
    return _kmv(_sorted_unique_pairs(g, h), k)


def _kmv(pairs: torch.Tensor, k: int) -> torch.Tensor:
    """keep the k smallest hashes per group; pairs [n, 2] (group, hash) unique & sorted"""
    if pairs.numel() == 0:
        return pairs
    g = pairs[:, 0]
    change = torch.ones_like(g, dtype=torch.bool)
    change[1:] = g[1:] != g[:-1]
    start_idx = torch.nonzero(change).flatten()
    counts = torch.diff(torch.cat([start_idx, torch.tensor([g.numel()], device=g.device)]))
    first = torch.repeat_interleave(start_idx, counts)
    rank_in_group = torch.arange(g.numel(), device=g.device) - first
    return pairs[rank_in_group < k]


def _search_filter(dim: str, q):
    if q is None:
        return S.NoopFilterSpec()
    t = q.type
    if t == "fragment":
        vals = [v.lower() for v in (q.values or [])]
        f = _PyFilter(dim, lambda v: v is not None and all(x in str(v).lower() for x in vals))
        f._pyneedles = vals  # type: ignore[attr-defined]  (the lowerer may hand them to the device matcher)
        return f
    if t == "regex":
        return S.RegexFilterSpec(dim, str(q.value))
    cs = q.caseSensitive and t != "insensitive_contains"
    return S.ContainsFilterSpec(dim, {"type": "contains" if cs else "insensitive_contains", "value": q.value,
                                      "caseSensitive": cs})


def _PyFilter(dim, fn):
    f = S.JavascriptFilterSpec(dim, "function(x) { return true; }")
    f._pyfn = fn  # type: ignore[attr-defined]
    return f


def _alnum_key(v):
    import re

    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", str(v))]


# ================================================================================== post-aggs
def eval_postagg(pa, cols: Dict[str, np.ndarray], n: int):
    if isinstance(pa, S.FieldAccessPostAggregationSpec):
        return np.asarray(cols[pa.fieldName], dtype=np.float64)
    if isinstance(pa, S.ConstantPostAggregationSpec):
        return np.full(n, float(pa.value))
    if isinstance(pa, S.HyperUniqueCardinalityPostAggregationSpec):
        return np.asarray(cols[pa.fieldName], dtype=np.float64)
    if isinstance(pa, S.StddevPostAggregationSpec):
        return np.sqrt(np.asarray(cols[pa.fieldName], dtype=np.float64))
    if isinstance(pa, S.ArithmeticPostAggregationSpec):
        vals = [np.asarray(eval_postagg(f, cols, n), dtype=np.float64) for f in pa.fields]
        out = vals[0].copy()
        for v in vals[1:]:
            if pa.fn == "+":
                out = out + v
            elif pa.fn == "-":
                out = out - v
            elif pa.fn == "*":
                out = out * v
            elif pa.fn == "/":
                with np.errstate(divide="ignore", invalid="ignore"):
                    out = np.where(v == 0, 0.0, out / np.where(v == 0, 1.0, v))
            elif pa.fn == "quotient":
                with np.errstate(divide="ignore", invalid="ignore"):
                    out = out / v
            else:
                raise LoweringError(f"unsupported arithmetic fn {pa.fn}")
        return out
    if isinstance(pa, S.JavascriptPostAggregationSpec):
        fn = compile_function(pa.function)
        args = [np.asarray(cols[f]) for f in pa.fieldNames]
        return np.array([float(fn(*[a[i] for a in args])) for i in range(n)], dtype=np.float64)
    raise LoweringError(f"unsupported post-aggregation {type(pa).__name__}")


def eval_having(h, cols: Dict[str, np.ndarray]) -> np.ndarray:
    if isinstance(h, S.ComparisonHavingSpec):
        v = np.asarray(cols[h.aggregation], dtype=np.float64)
        if h.type == "equalTo":
            return v == float(h.value)
        if h.type == "greaterThan":
            return v > float(h.value)
        return v < float(h.value)
    if isinstance(h, S.LogicalHavingSpec):
        ms = [eval_having(x, cols) for x in h.havingSpecs]
        out = ms[0]
        for m in ms[1:]:
            out = (out & m) if h.type == "and" else (out | m)
        return out
    if isinstance(h, S.NotHavingSpec):
        return ~eval_having(h.havingSpec, cols)
    raise LoweringError(f"unsupported having {type(h).__name__}")


def order_and_limit(cols: Dict[str, np.ndarray], idx: np.ndarray, order_cols, limit: int) -> np.ndarray:
    if order_cols:
        keys = []
        for oc in reversed(order_cols):
            if isinstance(oc, str):
                oc = S.OrderByColumnSpec(oc)
            col = cols[oc.dimension]
            if isinstance(col, DictColumn):  # sorted dictionaries: code order == value order
                v = col.codes[idx]
                keys.append(v.astype(np.float64) if oc.ascending else -v.astype(np.float64))
                continue
            v = np.asarray(col)[idx]
            if v.dtype == object:
                _, codes = np.unique(np.array([("" if x is None else str(x)) for x in v], dtype=object).astype(str),
                                     return_inverse=True)
                v = codes
            v = v.astype(np.float64)
            keys.append(v if oc.ascending else -v)
        order = np.lexsort(keys) if keys else np.arange(len(idx))
        idx = idx[order]
    return idx[: limit] if limit is not None and limit >= 0 else idx


def default_slots(dev) -> int:
    """Execution slots (concurrent statements, one HIP stream each) of a serving engine: 8 on a GPU
    -- the BI plan's closed loop peaks there (520 executions/s; 473/s at 10 slots, 457/s at 12:
    profiles/r6/thrift_jmx_s{8,10,12}_*cold*.json) now that the slots carve one arena each -- and 4
    on the host."""
    return 8 if getattr(dev, "type", "cpu") == "cuda" else 4


class Engine:
    """Executes QuerySpecs on the current rank's shards, merging across the process group."""

    def __init__(self, world: Optional[World] = None, use_native: Optional[bool] = None,
                 deterministic: Optional[bool] = None):
        from ..utils.memory import tune_host_malloc

        tune_host_malloc()
        self.world = world or get_world()
        if use_native is None:
            use_native = torch.cuda.is_available()
        self.use_native = use_native
        # bitwise reproducible float sums for every query (engine/lower.py Lowerer.deterministic);
        # per query: context {"deterministic": true}
        if deterministic is None:
            deterministic = os.environ.get("SDO_DETERMINISTIC", "0") not in ("", "0")
        self.deterministic = deterministic
        self._coalescer = None

    def coalescer(self, slots: Optional[int] = None):
        """The engine's stream scheduler + identical-statement batching (engine/scheduler.py),
        created on first use with ``slots`` HIP streams (``SDO_STREAMS``; default
        default_slots())."""
        if self._coalescer is None:
            from .scheduler import Coalescer, StreamScheduler

            n = slots or int(os.environ.get("SDO_STREAMS", "0")) or default_slots(self.world.device())
            self._coalescer = Coalescer(StreamScheduler(n, self.world.device()))
        return self._coalescer

    def prepare(self, qs: S.QuerySpec, ds: DataSource, segments_per_query: Optional[int] = None,
                key_passes: bool = True) -> PreparedQuery:
        """``segments_per_query`` set = historical execution (``sd/DruidRDD.scala:62-84, 244-277``):
        the query runs as one partial per batch of that many segments and the partials are merged
        by the engine (the reference's Spark-side PostAggregate, ``asd/PostAggregate.scala``);
        unset = broker execution, one fused scan over every segment."""
        if isinstance(getattr(qs, "dataSource", None), S.QueryDataSourceSpec):
            from .nested import NestedPreparedQuery

            return NestedPreparedQuery(self, qs, ds, segments_per_query)
        from ..segment.streamed import HostShard

        if isinstance(ds, HostShard):  # larger than HBM: streamed window by window
            from ..segment.streamed import StreamedQuery

            return StreamedQuery(self, qs, ds)
        pq = PreparedQuery(self, qs, ds, segments_per_query)
        if key_passes and qs.queryType == "groupBy" and not self.world.distributed and not segments_per_query \
                and len(pq.scans) == 1 and pq.window is None:
            from ..planner.cost import plan_key_passes

            passes = plan_key_passes(pq.scans[0][2])
            from ..planner import cost as _cost

            forced = _cost.FORCE_KEY_PASSES > 1
            key = _pass_key(pq.scans[0][1], 2 if forced else 1 << 20) if passes > 1 else None
            if key is not None:
                return KeyRangePasses(self, qs, ds, key, passes)
        return pq

    def execute_sets(self, specs, ds: DataSource, out_types=None) -> Optional[List[QueryResult]]:
        """Grouping-set queries from one scan (``execute_grouping_sets``); None if not fusable."""
        return execute_grouping_sets(self, specs, ds, out_types)

    def execute(self, qs: S.QuerySpec, ds: DataSource, segments_per_query: Optional[int] = None) -> QueryResult:
        return self.prepare(qs, ds, segments_per_query).run()


# ---------------------------------------------------------------------------------------------
# Grouping sets in one scan (SURVEY C5 / 2.5 "query-level fan-out": the reference issues one Druid
# query per grouping set and unions them, asd/DruidStrategy.scala:74-75)
_SET_FIELDS = ("dataSource", "intervals", "granularity", "filter")


def _set_signature(qs) -> str:
    import json

    d = qs.to_json()
    return json.dumps({k: d.get(k) for k in _SET_FIELDS}, sort_keys=True, default=str)


def _set_dims(qs):
    return list(getattr(qs, "dimensions", None) or [])  # a timeseries is the empty grouping set


def _union_by_name(items, name_of) -> Optional[list]:
    """Union of specs keyed by output name; None if one name carries two different specs."""
    import json

    out, seen = [], {}
    for it in items:
        enc = json.dumps(it.to_json(), sort_keys=True, default=str)
        k = name_of(it)
        if k in seen:
            if seen[k] != enc:
                return None
            continue
        seen[k] = enc
        out.append(it)
    return out


def fused_spec(specs):
    """The one groupBy answering every grouping set: the union of their dimensions and aggregators
    (None when the specs are not fusable: different source / filter / intervals / granularity,
    post-processing of their own, or one output name meaning two things)."""
    if len(specs) < 2 or any(not isinstance(q, (S.GroupByQuerySpec, S.TimeSeriesQuerySpec)) for q in specs):
        return None
    if not any(isinstance(q, S.GroupByQuerySpec) for q in specs):
        return None
    if any(getattr(q, "having", None) is not None or getattr(q, "limitSpec", None) is not None or q.postAggregations
           or getattr(q, "descending", False) or isinstance(q.dataSource, S.QueryDataSourceSpec) for q in specs):
        return None
    sig = _set_signature(specs[0])
    if any(_set_signature(q) != sig for q in specs[1:]):
        return None
    dims = _union_by_name([d for q in specs for d in _set_dims(q)], lambda d: d.outputName)
    aggs = _union_by_name([a for q in specs for a in (q.aggregations or [])], lambda a: a.name)
    if dims is None or aggs is None:
        return None
    q0 = specs[0]
    return S.GroupByQuerySpec(q0.dataSource, dims, filter=q0.filter, granularity=q0.granularity,
                              aggregations=aggs, intervals=q0.intervals)


def fusable_sets(specs) -> bool:
    """Plain groupBys (and the empty set's timeseries) over the same source, filter, intervals and
    granularity -- a CUBE / ROLLUP / GROUPING SETS expansion."""
    return fused_spec(specs) is not None


def _shell(engine, qs, ds) -> "PreparedQuery":
    """A PreparedQuery without a scan of its own: runs the post-merge tail (having / top-k prune /
    finalize / post-processing) for ``qs`` over partials computed elsewhere."""
    sh = PreparedQuery.__new__(PreparedQuery)
    sh.engine, sh.qs, sh.ds, sh.world = engine, qs, ds, engine.world
    sh.window, sh.scans, sh.segments_per_query = None, [], None
    return sh


def execute_grouping_sets(engine, specs, ds, out_types=None) -> Optional[List[QueryResult]]:
    """Answer several grouping-set queries from ONE scan: the widest set's groupBy runs once (scan
    + cross-GPU merge), then each set re-aggregates the merged fine partials on the device by its
    projected key (sum / min / max slot ops, HLL registers by max -- every pushed aggregator is
    decomposable).  None when the specs are not fusable (theta sketches, functionally-eliminated
    keys, non-injective key formats): the caller runs them one by one."""
    import copy
    import dataclasses
    import json

    widest = fused_spec(specs)
    if widest is None:
        return None
    cache = engine.__dict__.setdefault("_sets_cache", {})
    key = (json.dumps(widest.to_json(), sort_keys=True, default=str), id(ds))
    pq = cache.get(key)
    if pq is None:
        pq = PreparedQuery(engine, widest, ds)
        if len(cache) > 32:
            cache.clear()
        cache[key] = pq
    fine = pq._full_prog
    if fine.needs_rows or fine.stored_hll or fine.derived_aggs or any(kc.collapse for kc in fine.keys):
        return None
    t0 = time.perf_counter()
    root_only = engine.world.distributed and root_only_results()
    prog, part, _ = pq.run_partials(t0, root_only)
    if root_only and engine.world.rank != 0:
        part = empty_partials(prog, ds.device)  # rank 0 answers every set
    fp = part.compact()
    g = fp.keys.to(torch.int64)
    from .partials import merge_sparse

    fine_ids = [torch.remainder(torch.div(g, kc.stride, rounding_mode="floor"), max(1, kc.card)) for kc in prog.keys]
    out = []
    for i, qs in enumerate(specs):
        names = {d.outputName for d in _set_dims(qs)}
        keep = [j for j, kc in enumerate(prog.keys) if kc.name in names or kc.is_timestamp]
        keys = [copy.copy(prog.keys[j]) for j in keep]
        comps = [fine_ids[j] for j in keep]
        derived = []
        for kc, det, lut in prog.derived:
            if kc.name not in names:
                continue
            if det in keep:  # still functionally determined by a kept key: stays derived
                derived.append((kc, keep.index(det), lut))
                continue
            # its determinant is not in this set: the dependent dimension becomes a real key,
            # its ids looked up from the fine determinant ids (the FD table)
            did = fine_ids[det]
            orig = prog.keys[det].orig
            if orig is not None:
                did = torch.from_numpy(orig).to(did.device)[did]
            k2 = copy.copy(kc)
            k2.orig, k2.remap = None, None
            keys.append(k2)
            comps.append(lut.to(did.device)[did].to(torch.int64))
        G = 1
        for kc in reversed(keys):
            kc.stride = G
            G *= max(1, kc.card)
        coarse = dataclasses.replace(prog, keys=keys, G=G, derived=derived,
                                     key_order=[n for n in prog.key_order if n in names or n == "timestamp"])
        ck = torch.zeros_like(g)
        for kc, ids in zip(keys, comps):
            ck += ids * kc.stride
        cp = merge_sparse([Partials("sparse", fp.acc, ck, fp.hll)], prog.slots) if g.numel() else \
            Partials("sparse", fp.acc, ck, fp.hll)
        sh = _shell(engine, qs, ds)
        sh._full_prog = coarse
        cols = finalize(coarse, cp, out_types[i] if out_types else None)
        res = sh._post(coarse, cols)
        res.stats.update(fused_sets=len(specs), exec_ms=(time.perf_counter() - t0) * 1e3)
        out.append(res)
    return out


# ---------------------------------------------------------------------------------------------
# Key-range passes: dense group tables far larger than the Infinity Cache
class KeyRangePasses:
    """A groupBy whose dense HBM table is far larger than the 256 MB Infinity Cache (TPC-H Q18:
    150M orders) runs as P scans, each restricted to 1/P of the largest key's dictionary ids
    (``IdRangeFilterSpec``); the filter-implied key compaction of the lowering (engine/lower.py
    compact_key) gives every pass a cache-resident table.  Group keys are disjoint across passes,
    so HAVING applies per pass and the results concatenate; ORDER BY ... LIMIT k keeps each pass's
    top k (a superset) and re-orders the union.  Planned by planner/cost.py plan_key_passes."""

    def __init__(self, engine, qs, ds, key, passes: int):
        self.engine, self.qs, self.ds = engine, qs, ds
        self.key = key
        card = max(1, int(key.card))
        step = -(-card // passes)
        self.ranges = [(lo, min(card, lo + step)) for lo in range(0, card, step)]
        self.subs = []
        for lo, hi in self.ranges:
            f = S.IdRangeFilterSpec(key.col, lo, hi)
            filt = f if qs.filter is None else S.LogicalFilterSpec("and", [qs.filter, f])
            self.subs.append(PreparedQuery(engine, qs.copy(filter=filt), ds))
        self.deterministic = bool(self.subs[0].deterministic) if self.subs else False
        self.scans = self.subs[0].scans if self.subs else []

    @property
    def out_types(self):
        return getattr(self.subs[0], "out_types", None)

    @out_types.setter
    def out_types(self, v):
        for p in self.subs:
            p.out_types = v

    def run(self) -> QueryResult:
        t0 = time.perf_counter()
        res = [p.run() for p in self.subs]
        cols = list(res[0].columns)
        data: Dict[str, Any] = {}
        for c in cols:
            parts = [r.data[c] for r in res]
            if isinstance(parts[0], DictColumn):
                data[c] = DictColumn(np.concatenate([np.asarray(x.codes, dtype=np.int64) for x in parts]),
                                     parts[0].dictionary)
            else:
                data[c] = np.concatenate([np.asarray(x) for x in parts])
        n = len(data[cols[0]]) if cols else 0
        ls = getattr(self.qs, "limitSpec", None)
        if ls is not None and n:
            idx = order_and_limit(data, np.arange(n), ls.columns, ls.limit)
            data = {c: take(v, idx) for c, v in data.items()}
        out = QueryResult(cols, data, res[0].query_type, {"groups": sum(r.stats.get("groups", 0) for r in res)})
        out.stats.update(passes=len(self.subs), exec_ms=(time.perf_counter() - t0) * 1e3)
        self.last_stats = out.stats
        return out


def _pass_key(prog, min_card: int = 1 << 20):
    """The key to split on: the widest plain dictionary-id key (not already compacted)."""
    best = None
    for kc in prog.keys:
        if kc.kind == D.K_ID and kc.orig is None and kc.base == 0 and kc.card >= min_card and \
                (best is None or kc.card > best.card):
            best = kc
    return best
