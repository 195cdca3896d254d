"""Partial aggregates of one shard, their cross-GPU merge representation, and finalization
into host result columns (the role of the reference's result iterators + DruidValTransform,
``asd/DruidQueryResultIterator.scala``, ``sd/DruidRDD.scala:285-418``)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from ..ops import desc as D
from .lower import fixed_value, ord2f


@dataclass
class Partials:
    kind: str                        # dense | sparse
    acc: torch.Tensor                # [R, nslots] int64 (f64 slots hold bit patterns)
    keys: Optional[torch.Tensor]     # [R] int64 (sparse)
    hll: List[torch.Tensor] = field(default_factory=list)  # [R, m] uint8 byte registers each
    # multi-rank: this rank holds a DISJOINT slice of the final groups (after the shuffle, or when
    # grouped on the shard key); parallel/merge.py gather_groups concatenates the slices, carrying
    # ``status`` (this rank's failure word, parallel/fault.py) in that collective
    scattered: bool = False
    status: int = 0
    # peer-to-peer merge (parallel/p2p.py): every rank's status word, still on the device -- read
    # with the result's device-to-host copy (finalize) instead of a separate host synchronisation
    status_dev: Optional[torch.Tensor] = None
    status_rank: int = 0

    @property
    def rows(self) -> int:
        return int(self.acc.shape[0])

    def compact(self) -> "Partials":
        """dense -> sparse keeping groups with a non-zero presence count (slot 0).  A P2P-merged
        state's status words are checked first: the compacted state no longer carries them."""
        if self.kind == "sparse":
            return self
        if self.status_dev is not None:
            from ..parallel.p2p import check_status

            check_status(self)
        if self.acc.is_cuda:
            from ..ops import native

            idx = native.nonzero_rows(self.acc[:, 0])  # ballot mask + compact_rows kernels
        else:
            idx = torch.nonzero(self.acc[:, 0] > 0).flatten()
        return Partials("sparse", self.acc.index_select(0, idx), idx, [h.index_select(0, idx) for h in self.hll],
                        self.scattered, self.status)


class DeferredSparse(Partials):
    """Sparse partials of a first-touch scan (engine/device_exec.py) whose groups are counted but
    still lie in the scan's accumulator table: ``finalize`` turns them into host columns in one
    kernel (``_native_sparse``: post_scan.hip touch_decode_kernel); any other consumer reads
    ``keys`` / ``acc``, which gathers them first (ops/native.py touch_gather) -- from then on this is
    an ordinary sparse state.  Either way the table's touched rows are re-initialised and the slot's
    buffers marked clean (``bufs``: the scan's _Bufs, whose ``pending`` names this state meanwhile)."""

    def __init__(self, count, bufs):
        Partials.__init__(self, "sparse", None, None)
        self.count, self.bufs, self.lost, self.n = count, bufs, False, count.n

    @property
    def pending(self) -> bool:
        return self.count is not None

    def take(self):
        """The counted table (ops/native.py TouchCount) for whoever empties it now."""
        if self.lost:
            raise RuntimeError("deferred sparse partials read after their scan's buffers were re-used")
        c, b = self.count, self.bufs
        self.count = self.bufs = None
        b.clean, b.pending = True, None
        return c

    def gather(self) -> None:
        """Materialise ``keys`` / ``acc`` (no-op once done)."""
        if self.pending:
            from ..ops import native

            self._keys, self._acc = native.touch_gather(self.take())

    def __repr__(self) -> str:  # (the dataclass's would read -- and so gather -- keys / acc)
        return f"DeferredSparse(rows={self.rows}, pending={self.pending})"

    @property
    def rows(self) -> int:
        return self.n if self._acc is None else int(self._acc.shape[0])

    @property
    def keys(self):
        self.gather()
        return self._keys

    @keys.setter
    def keys(self, v):
        self._keys = v

    @property
    def acc(self):
        self.gather()
        return self._acc

    @acc.setter
    def acc(self, v):
        self._acc = v


def merge_sparse(parts: List[Partials], slots) -> Partials:
    """Merge sparse partials by key (sum / min / max per slot op, max for HLL registers)."""
    parts = [p.compact() for p in parts]
    keys = torch.cat([p.keys for p in parts])
    acc = torch.cat([p.acc for p in parts])
    uk, inv = torch.unique(keys, return_inverse=True)
    R = uk.numel()
    out = torch.empty((R, acc.shape[1]), dtype=torch.int64, device=acc.device)
    for s, (op, init) in enumerate(slots):
        col = torch.full((R,), init, dtype=torch.int64, device=acc.device)
        src = acc[:, s]
        if op == D.S_SUM_I:
            col.zero_().index_add_(0, inv, src)
        elif op == D.S_SUM_F:
            cf = torch.zeros(R, dtype=torch.float64, device=acc.device)
            cf.index_add_(0, inv, src.view(torch.float64))
            col = cf.view(torch.int64)
        elif op == D.S_MIN_I:
            col.scatter_reduce_(0, inv, src, reduce="amin", include_self=True)
        else:
            col.scatter_reduce_(0, inv, src, reduce="amax", include_self=True)
        out[:, s] = col
    hll = []
    for i in range(len(parts[0].hll)):
        h = torch.cat([p.hll[i] for p in parts])
        m = h.shape[1]
        o = torch.zeros((R, m), dtype=h.dtype, device=acc.device)
        o.scatter_reduce_(0, inv.unsqueeze(1).expand(-1, m), h, reduce="amax", include_self=True)
        hll.append(o)
    return Partials("sparse", out, uk, hll)


def hll_estimates(regs: torch.Tensor, p: int) -> np.ndarray:
    """Estimate per group: native MFMA kernel on GPU, torch on CPU."""
    G = regs.shape[0]
    if G == 0:
        return np.zeros(0, dtype=np.float64)
    if regs.is_cuda:
        from ..ops import native

        est = torch.empty(G, dtype=torch.float64, device=regs.device)
        native.hll_estimate(regs.contiguous(), G, p, est)
        return est.cpu().numpy()
    from ..ops.reference import hll_estimate_torch

    return hll_estimate_torch(regs, p).numpy()


def d2h(ts: List[torch.Tensor]) -> List[np.ndarray]:
    """Device -> host through pinned (cached) staging buffers with one stream sync."""
    outs = []
    dev = None
    for t in ts:
        if t.is_cuda:
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            outs.append(h)
            dev = t.device
        else:
            outs.append(t)
    if dev is not None:
        from ..ops import native

        native.stream_sync(dev)  # this thread's stream only, GIL released while waiting
    return [o.numpy() for o in outs]


_STAGE = __import__("threading").local()
_NATIVE: list = []


def _native():
    if not _NATIVE:
        from ..ops import native

        _NATIVE.append(native)
    return _NATIVE[0]


def _fetch_small(acc: torch.Tensor, hll: List[torch.Tensor], G: int, p: int,
                 status: Optional[torch.Tensor] = None, reset_args: Optional[tuple] = None) -> List[np.ndarray]:
    """[acc as host int64 [G, ns], estimates per register block...] of a small dense state,
    read back through per-thread pinned / device scratch buffers (reused across executions).
    ``status``: a P2P merge's status words, copied in the same stream before the one sync and
    returned last.  ``reset_args``: re-initialise the scan's buffers behind the copies (the next
    run then launches the scan alone, engine/executor.py _SmallDenseRunner)."""
    native = _native()

    nb = acc.numel() * 8
    need = nb + len(hll) * G * 8
    ns = 0 if status is None else status.numel() * 8
    host = getattr(_STAGE, "host", None)
    if host is None or host.numel() < need + ns:
        host = _STAGE.host = torch.empty(max(need + ns, 1 << 16), dtype=torch.uint8, pin_memory=True)
    if status is not None:
        host[need: need + ns].copy_(status.view(torch.uint8), non_blocking=True)
    est = getattr(_STAGE, "est", None)
    if hll and (est is None or est.numel() < len(hll) * G or est.device != acc.device):
        est = _STAGE.est = torch.empty(max(len(hll) * G, 4096), dtype=torch.float64, device=acc.device)
    if reset_args is not None:
        native.fetch_small_reset(acc, hll, G, p, est if hll else acc, host, reset_args)
    else:
        native.fetch_small(acc, [h.contiguous() for h in hll], G, p, est if hll else acc, host)
    buf = host.numpy()
    out = [buf[:nb].view(np.int64).reshape(acc.shape)]
    for i in range(len(hll)):
        out.append(buf[nb + i * G * 8: nb + (i + 1) * G * 8].view(np.float64))
    if status is not None:
        out.append(buf[need: need + ns].view(np.int64).copy())
    return out


_INT_T = ("tinyint", "smallint", "int", "bigint")
_NO_DEVICE_DECODE = False  # (tests / tools: decode every result column on the host)
_I32 = (-(1 << 31), (1 << 31) - 1)


class _Const:
    """A key whose every value is the same (a one-entry dictionary): nothing crosses the link."""

    def __init__(self, value, dtype):
        self.value, self.dtype = value, dtype


def _const_column(R: int, v: "_Const") -> np.ndarray:
    """A read-only length-R view of one value (stride 0): a constant key of a million-row result
    (TPC-H Q3's o_shippriority) costs nothing instead of a 4 MB fill."""
    return np.broadcast_to(np.asarray(v.value, dtype=v.dtype), (R,))


def _typed_plan(kc, sqlt: Optional[str], device):
    """How a dictionary-id key becomes its final numeric SQL-typed values ON THE DEVICE (the same
    values ``sql/execute.py:_dict_series`` would produce on the host): integer range dictionaries
    are ``start + id`` -> ("range", start, torch dtype); other dictionaries of up to 4M entries gather
    from a cached device table of their typed values -> ("table", table); a one-entry dictionary is
    a ``_Const``.  ``int`` and narrower SQL types travel as int32.  A million-group result (TPC-H
    Q3: o_orderkey, o_shippriority) then ships final values at their SQL width and the host does no
    per-row decode pass.  None when not applicable (strings, NULL-bearing dictionaries, huge
    non-range dictionaries)."""
    d = getattr(kc, "dictionary", None)
    if d is None or sqlt is None or kc.orig is not None:
        return None
    from ..sql.types import base

    bt = base(sqlt)
    if bt not in _INT_T and bt not in ("double", "float"):
        return None
    narrow = bt in ("tinyint", "smallint", "int")
    if hasattr(d, "start") and not getattr(d, "has_null", False) and not hasattr(d, "prefix"):
        lo, hi = int(d.start), int(d.start) + len(d) - 1
        if narrow and _I32[0] <= lo and hi <= _I32[1]:
            return ("range", lo, torch.int32)
        return ("range", lo, torch.int64 if bt in _INT_T else torch.float64)
    if len(d) > (1 << 22):
        return None
    cache = d.__dict__.setdefault("_dev_typed", {})
    key = (bt, str(device))
    tab = cache.get(key)
    if tab is None:
        from ..sql.execute import _raw
        from ..sql.types import to_series

        typed = to_series(_raw(d.all_values()), sqlt)
        if typed.isna().any() or len(typed) == 0:
            tab = False
        else:
            arr = typed.to_numpy(dtype=np.int64 if bt in _INT_T else np.float64)
            if len(arr) == 1:
                tab = _Const(arr[0], arr.dtype)
            else:
                if narrow and _I32[0] <= int(arr.min()) and int(arr.max()) <= _I32[1]:
                    arr = arr.astype(np.int32)
                tab = torch.from_numpy(np.ascontiguousarray(arr)).to(device)
        cache[key] = tab
    if tab is False:
        return None
    if isinstance(tab, _Const):
        return tab
    return ("table", tab)


def _device_typed(kc, ids: torch.Tensor, sqlt: Optional[str]):
    """Typed values of a dictionary-id key computed on the device with torch ops (``_typed_plan``)."""
    plan = _typed_plan(kc, sqlt, ids.device)
    if plan is None or isinstance(plan, _Const):
        return plan
    if plan[0] == "range":
        lo, dt = plan[1], plan[2]
        if dt == torch.int32:
            return ids.to(torch.int32) + lo
        v = ids.to(torch.int64) + lo
        return v if dt == torch.int64 else v.to(torch.float64)
    return plan[1].index_select(0, ids.to(torch.int64))


def _narrow_ids(kc, ids: torch.Tensor) -> torch.Tensor:
    """Dictionary ids at the narrowest width their cardinality allows (fewer D2H bytes)."""
    if kc.card <= (1 << 15) and getattr(kc, "dictionary", None) is not None:
        return ids.to(torch.int16)
    return ids.to(torch.int32) if kc.card < 2 ** 31 else ids


def _agg_outputs_dev(prog, acc: torch.Tensor, skip) -> Dict[str, torch.Tensor]:
    """Final aggregator columns on the device (same values as finalize's host conversions)."""
    out = {}
    for a in prog.aggs:
        if a.name in skip or a.slot < 0 or a.kind in ("hll", "theta", "quantile", "distinct", "moment"):
            continue
        col = acc[:, a.slot]
        if a.kind == "count":
            v = col
        elif a.kind in ("sum_i", "min_i", "max_i"):
            if a.scale:
                v = col.to(torch.float64) / (10.0 ** a.scale)
            elif a.out_type == "long":
                v = col
            else:
                v = col.to(torch.float64)
        elif a.kind == "sum_f":
            v = col.contiguous().view(torch.float64)
        elif a.kind == "sum_fx":
            v = fixed_value(col, acc[:, a.slot2])
        elif a.kind in ("min_f", "max_f"):
            v = torch.where(col >= 0, col, col ^ 0x7FFFFFFFFFFFFFFF).view(torch.float64)
            if a.out_type == "long":
                v = torch.where(torch.isfinite(v), v, torch.zeros_like(v)).to(torch.int64)
        else:
            continue
        out[a.name] = v.contiguous()
    return out


SMALL_DENSE_WORDS = 1 << 20  # dense states up to this many accumulator words are fetched whole
NATIVE_DECODE = True  # sparse finalize through post_scan.hip sparse_decode_kernel (tests compare both)
# first-touch scans hand finalize their counted table (DeferredSparse): gather + decode in one
# kernel (post_scan.hip touch_decode_kernel); False gathers in the scan as before (tests compare both)
FUSED_TOUCH_DECODE = True
_LUT_T = {torch.int32: 1, torch.int64: 2, torch.float64: 3}
_OUT_NP = {0: np.int16, 1: np.int32, 2: np.int64, 3: np.float64, 4: np.float64, 5: np.int64}
_OUT_W = {0: 2, 1: 4, 2: 8, 3: 8, 4: 8, 5: 8}
_DT_OUT = {torch.int32: 1, torch.int64: 2, torch.float64: 3}


def _dev_table(holder, key, t, device) -> torch.Tensor:
    """A decode table (FD map, typed dictionary values) on the device as int32 / int64 / f64,
    cached on ``holder`` (the prepared program or key) -- not re-uploaded per execution."""
    cache = holder.__dict__.setdefault("_dec_tabs", {})
    ck = (key, str(device))
    v = cache.get(ck)
    if v is None:
        t = torch.as_tensor(t)
        if t.dtype not in _LUT_T:
            t = t.to(torch.float64 if t.is_floating_point() else torch.int64)
        v = cache[ck] = t.to(device).contiguous()
    return v


def _native_sparse(prog, parts: Partials, out_types, want_gid: bool):
    """Sparse finalize through ONE kernel and ONE device-to-host copy (ops/csrc/post_scan.hip
    sparse_decode_kernel): every key component, functionally dependent key, derived aggregate and
    aggregator output is computed at its final width into one device buffer.  Returns
    (key_ids, derived_ids, derived_agg_vals, agg_host, gid, typed) or None when a column needs the
    general torch path (fixed-point float sums, float FD aggregate tables, > 16 columns)."""
    deferred = isinstance(parts, DeferredSparse) and parts.pending
    if deferred:  # (still in the scan's table: on the device, R counted)
        if _NO_DEVICE_DECODE:
            return None
        dev, R = parts.count.acc.device, parts.count.n
    else:
        g = parts.keys
        if not g.is_cuda or _NO_DEVICE_DECODE:
            return None
        if not g.is_contiguous():  # (the kernel reads the ids as one contiguous int64 array)
            g = g.contiguous()
        dev = g.device
        R = int(g.numel())
    specs, consts, typed = [], {}, {}

    def key_base(det):
        kd = prog.keys[det]
        orig = 0
        if kd.orig is not None:
            orig = _dev_table(kd, "orig", torch.from_numpy(np.asarray(kd.orig, dtype=np.int64)), dev).data_ptr()
        return int(kd.stride), max(1, int(kd.card)), orig

    def typed_spec(i, kc, stride, card, orig, lut, lut_key):
        """(key i's spec) through its SQL-typed plan, or as narrow ids."""
        plan = _typed_plan(kc, out_types.get(kc.name), dev) if out_types else None
        lut_ptr = lut.data_ptr() if lut is not None else 0
        lut_t = _LUT_T[lut.dtype] if lut is not None else 0
        if isinstance(plan, _Const):
            typed[i] = plan
            consts[i] = plan
            return None
        if plan is not None and plan[0] == "range":
            typed[i] = "dev"
            return (0, _DT_OUT[plan[2]], lut_t, 0, stride, card, int(plan[1]), orig, lut_ptr, 0.0)
        if plan is not None:  # typed table (composed with the FD map for a derived key)
            tab = plan[1]
            if lut is not None:
                tab = _dev_table(prog, ("typed", lut_key, kc.name), tab.index_select(0, lut.to(torch.int64)), dev)
            typed[i] = "dev"
            return (0, 4 if tab.dtype == torch.float64 else _DT_OUT[tab.dtype], _LUT_T[tab.dtype], 0, stride, card, 0,
                    orig, tab.data_ptr(), 0.0)
        out = 0 if (kc.card <= (1 << 15) and getattr(kc, "dictionary", None) is not None) else \
            (1 if kc.card < 2 ** 31 else 2)
        return (0, out, lut_t, 0, stride, card, 0, orig, lut_ptr, 0.0)

    order = []  # (role, index) per spec
    nk = len(prog.keys)
    for i, kc in enumerate(prog.keys):
        sp = typed_spec(i, kc, int(kc.stride), max(1, int(kc.card)), 0, None, None)
        if sp is not None:
            specs.append(sp)
            order.append(("key", i))
    for j, (kc, det, lut) in enumerate(getattr(prog, "derived", ())):
        stride, card, orig = key_base(det)
        lut_d = _dev_table(prog, ("fd", j), lut, dev)
        if lut_d.dtype == torch.float64:
            return None
        sp = typed_spec(nk + j, kc, stride, card, orig, lut_d, ("fd", j))
        if sp is not None:
            specs.append(sp)
            order.append(("key", nk + j))
    for j, (a, det, lut) in enumerate(getattr(prog, "derived_aggs", ())):
        stride, card, orig = key_base(det)
        lut_d = _dev_table(prog, ("dag", j), lut, dev)
        if lut_d.dtype == torch.float64:
            return None
        specs.append((0, 2, _LUT_T[lut_d.dtype], 0, stride, card, 0, orig, lut_d.data_ptr(), 0.0))
        order.append(("dag", j))
    derived_names = {a.name for a, _, _ in getattr(prog, "derived_aggs", ())}
    for a in prog.aggs:
        if a.name in derived_names or a.slot < 0 or a.kind in ("hll", "theta", "quantile", "distinct", "moment"):
            continue
        if a.kind == "count":
            sp = (1, 2, 0, a.slot, 1, 1, 0, 0, 0, 0.0)
        elif a.kind in ("sum_i", "min_i", "max_i"):
            if a.scale:
                sp = (1, 3, 0, a.slot, 1, 1, 0, 0, 0, float(10.0 ** a.scale))
            else:
                sp = (1, 2 if a.out_type == "long" else 3, 0, a.slot, 1, 1, 0, 0, 0, 0.0)
        elif a.kind == "sum_f":
            sp = (3, 4, 0, a.slot, 1, 1, 0, 0, 0, 0.0)
        elif a.kind in ("min_f", "max_f"):
            sp = (2, 5 if a.out_type == "long" else 4, 0, a.slot, 1, 1, 0, 0, 0, 0.0)
        elif a.kind == "sum_fx":
            return None
        else:
            continue
        specs.append(sp)
        order.append(("agg", a.name))
    if want_gid:
        specs.append((4, 2, 0, 0, 1, 1, 0, 0, 0, 0.0))
        order.append(("gid", 0))
    if len(specs) > 16:
        return None
    offs, off = [], 0
    for sp in specs:
        offs.append(off)
        off = (off + R * _OUT_W[sp[1]] + 15) // 16 * 16
    nbytes = off
    host = torch.empty(max(nbytes, 16), dtype=torch.uint8, pin_memory=True)
    from ..ops import native

    cols = [sp + (o,) for sp, o in zip(specs, offs)]
    if deferred:
        native.touch_decode(parts.count, cols, nbytes, host)
        parts.take()  # (emptied into ``host``: keys / acc stay None)
    else:
        acc = parts.acc if parts.acc.is_contiguous() else parts.acc.contiguous()
        out = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        native.load().sparse_decode(g.data_ptr(), acc.data_ptr(), R, int(acc.shape[1]) if acc.dim() == 2 else 1, cols,
                                    out.data_ptr(), nbytes, host.data_ptr(), native._stream(dev))
    hb = host.numpy()
    key_all = [None] * (nk + len(getattr(prog, "derived", ())))
    dag_vals = [None] * len(getattr(prog, "derived_aggs", ()))
    agg_host, gid = {}, None
    for (role, i), sp, o in zip(order, specs, offs):
        arr = hb[o: o + R * _OUT_W[sp[1]]].view(_OUT_NP[sp[1]])
        if role == "key":
            key_all[i] = arr
        elif role == "dag":
            dag_vals[i] = arr
        elif role == "agg":
            agg_host[i] = arr
        else:
            gid = arr
    for i, c in consts.items():
        key_all[i] = _const_column(R, c)
    return R, key_all[:nk], key_all[nk:], dag_vals, agg_host, gid, typed


_DECODE_TABLE_MAX = 1 << 16


def _decode_key_int(kc, ids, sqlt: Optional[str]):
    """An integer-typed output of a key whose decoder yields digit strings (a numeric time format:
    ``year(dateTime(...))`` -> 'yyyy'), decoded straight to the int64 values the SQL layer would
    parse from those strings (sql/execute.py druid_value_series): one table of the key's domain,
    built once.  None when not applicable."""
    if sqlt not in _INT_T:
        return None
    tab = kc.__dict__.get("_int_table")
    if tab is None:
        tab = False
        if 0 < kc.card <= _DECODE_TABLE_MAX:
            full = kc.decoder(np.arange(kc.card, dtype=np.int64))
            if isinstance(full, np.ndarray) and full.dtype == object and len(full) == kc.card:
                try:
                    tab = full.astype(np.int64)
                except (TypeError, ValueError):
                    tab = False
        kc._int_table = tab
    if tab is False:
        return None
    return tab[np.asarray(ids, dtype=np.int64)]


def _decode_key(kc, ids):
    """``kc.decoder(ids)`` through a table of the whole key domain, built once per key: a prepared
    query re-run many times (dashboards, the benchmark) then decodes by one numpy gather instead of
    a Python loop per group (time-format keys: year / month / date strings).  Decoders returning
    dictionary-coded columns are already a view and are called directly."""
    tab = kc.__dict__.get("_decode_table")
    if tab is None:
        tab = False
        if 0 < kc.card <= _DECODE_TABLE_MAX and len(ids) * 4 >= min(kc.card, 64):
            full = kc.decoder(np.arange(kc.card, dtype=np.int64))
            if isinstance(full, np.ndarray) and len(full) == kc.card:
                tab = full
        if tab is not False or len(ids) * 4 >= min(kc.card, 64):
            kc._decode_table = tab
    if tab is False:
        return kc.decoder(ids)
    return tab[np.asarray(ids, dtype=np.int64)]


def finalize(prog, parts: Partials, out_types: Optional[Dict[str, str]] = None,
             prefetched: Optional[List[np.ndarray]] = None) -> Dict[str, np.ndarray]:
    """Decode groups into host columns: key outputs then aggregator outputs (Druid types).
    A P2P-merged state's status words are read with its result copy; any other consumer checks
    them first (parallel/p2p.py check_status).

    Large (sparse) results are decoded on the device and cross the host link narrow: key ids at
    their dictionary's width, numeric dictionary keys as final SQL-typed values when ``out_types``
    (output name -> SQL type, from the SQL layer) asks for them, constant keys not at all, and only
    the accumulator slots an output reads."""
    want_gid = bool(getattr(prog, "needs_rows", False))
    collapse = any(kc.collapse for kc in prog.keys)
    typed: Dict[int, object] = {}
    est_host: List[np.ndarray] = []
    if parts.kind == "dense":
        small = parts.rows * parts.acc.shape[1] <= SMALL_DENSE_WORDS
        if small:
            # HLL estimates of every group computed before the one D2H (one sync, not two)
            est_dev = []
            G = parts.rows
            want_est = bool(parts.hll) and G * (1 << prog.hll_p) <= (1 << 26) and not collapse
            if prefetched is not None:
                host = prefetched  # (the caller's _fetch_small of exactly this state)
            elif parts.acc.is_cuda and parts.acc.is_contiguous():
                # estimates + both copies + the sync in one native call (bindings.cpp fetch_small),
                # through this thread's pinned staging buffer; the fancy indexing below copies out
                host = _fetch_small(parts.acc, list(parts.hll) if want_est else [], G, prog.hll_p,
                                    parts.status_dev)
                if parts.status_dev is not None:
                    sts = host.pop()
                    parts.status_dev = None
                    from ..parallel.p2p import note_ok, raise_status

                    if sts.any():
                        raise_status(sts.tolist(), parts.status_rank)
                    note_ok(parts.status_rank)
            else:
                if want_est and parts.acc.is_cuda:
                    from ..ops import native

                    for h in parts.hll:
                        e = torch.empty(G, dtype=torch.float64, device=h.device)
                        native.hll_estimate(h.contiguous(), G, prog.hll_p, e)
                        est_dev.append(e)
                host = d2h([parts.acc] + est_dev)
            if parts.status_dev is not None:  # (not fetched with the copy above)
                from ..parallel.p2p import check_status

                check_status(parts)
            acc_h = host[0]
            gid = np.flatnonzero(acc_h[:, 0] > 0)
            acc_h = acc_h[gid]
            acc_cols = {s: acc_h[:, s] for s in range(acc_h.shape[1])}
            R = len(gid)
            est_host = [e[gid] for e in host[1:]]
            hll_d = [] if est_host else [h.index_select(0, torch.from_numpy(gid).to(h.device)) for h in parts.hll]
            key_ids = [(gid // kc.stride) % max(1, kc.card) for kc in prog.keys]
            derived_ids = None
            derived_agg_vals = []
            for a, det, lut in getattr(prog, "derived_aggs", ()):
                did = np.asarray(key_ids[det], dtype=np.int64)
                orig = prog.keys[det].orig
                if orig is not None:
                    did = orig[did]
                derived_agg_vals.append(lut[torch.from_numpy(did).to(lut.device)].cpu().numpy())
        else:
            if parts.status_dev is not None:
                from ..parallel.p2p import check_status

                check_status(parts)
            parts = parts.compact()
    nat = _native_sparse(prog, parts, out_types, want_gid) \
        if parts.kind == "sparse" and not collapse and NATIVE_DECODE else None
    if nat is not None:
        R, key_ids, derived_ids, derived_agg_vals, agg_host, gid, typed_n = nat
        typed.update(typed_n)
        acc_cols = {}
        hll_d = parts.hll
    elif parts.kind == "sparse":
        # decode key components on the device, then one pinned D2H of every array
        g = parts.keys
        R = int(g.numel())
        full_ids = []
        for kc in prog.keys:
            ids = torch.remainder(torch.div(g, kc.stride, rounding_mode="floor"), max(1, kc.card))
            full_ids.append(ids)
        nk = len(full_ids)
        dag = []
        for a, det, lut in getattr(prog, "derived_aggs", ()):
            # min/max of a metric constant per key: gathered from its FD table, no accumulator
            did = full_ids[det]
            orig = prog.keys[det].orig
            if orig is not None:
                did = torch.from_numpy(orig).to(did.device)[did]
            dag.append(lut.to(did.device)[did])
        all_kcs = list(prog.keys)
        for kc, det, lut in getattr(prog, "derived", ()):
            # functionally dependent keys: gather their ids on the device
            did = full_ids[det]
            orig = prog.keys[det].orig
            if orig is not None:
                did = torch.from_numpy(orig).to(did.device)[did]
            full_ids.append(lut.to(did.device)[did].to(torch.int64))
            all_kcs.append(kc)
        dev_ids = []
        for i, (kc, ids) in enumerate(zip(all_kcs, full_ids)):
            v = None
            if out_types and g.is_cuda and not _NO_DEVICE_DECODE and not collapse:
                v = _device_typed(kc, ids, out_types.get(kc.name))
            if v is not None:
                typed[i] = v
                dev_ids.append(None if isinstance(v, _Const) else v)
            else:
                dev_ids.append(_narrow_ids(kc, ids) if g.is_cuda else (ids.to(torch.int32) if kc.card < 2 ** 31 else ids))
        # aggregator outputs finished on the device (decimal scaling, float views, ordered-float
        # decode) so the host receives final columns; with non-injective key formatting the raw
        # slots travel instead (the host re-aggregates)
        nslots = parts.acc.shape[1]
        derived_names = {a.name for a, _, _ in getattr(prog, "derived_aggs", ())}
        agg_dev = {} if collapse else _agg_outputs_dev(prog, parts.acc, derived_names)
        need = list(range(nslots)) if collapse else []
        acc_dev = parts.acc[:, need].t().contiguous() if need else None
        agg_names = list(agg_dev)
        ship = [t for t in dev_ids if t is not None] + dag + ([acc_dev] if acc_dev is not None else []) + \
            [agg_dev[n] for n in agg_names] + ([g] if want_gid else [])
        host = d2h(ship)
        it = iter(host)
        hid = [None if t is None else next(it) for t in dev_ids]
        key_ids = hid[:nk]
        derived_ids = hid[nk:]
        derived_agg_vals = [next(it) for _ in dag]
        acc_rows = next(it) if acc_dev is not None else None
        acc_cols = {s: acc_rows[k] for k, s in enumerate(need)}
        agg_host = {n: next(it) for n in agg_names}
        gid = next(it) if want_gid else None
        hll_d = parts.hll
        for i, v in typed.items():
            if isinstance(v, _Const):
                (key_ids if i < nk else derived_ids)[i if i < nk else i - nk] = _const_column(R, v)
    if parts.kind != "sparse":
        agg_host = {}
    cols: Dict[str, np.ndarray] = {}
    key_vals = []
    for i, (kc, ids) in enumerate(zip(prog.keys, key_ids)):
        vals = None
        if not (i in typed or kc.decoder is None) and out_types and not collapse:
            vals = _decode_key_int(kc, ids, out_types.get(kc.name))
        if vals is None:
            vals = ids if (i in typed or kc.decoder is None) else _decode_key(kc, ids)
        key_vals.append(vals)
        cols[kc.name] = vals
    for j, (kc, det, lut) in enumerate(getattr(prog, "derived", ())):
        # functionally dependent key: its id through the FD table of the determinant's original id
        if derived_ids is not None:
            ids = derived_ids[j]
        else:
            did = np.asarray(key_ids[det], dtype=np.int64)
            orig = prog.keys[det].orig
            if orig is not None:
                did = orig[did]
            ids = lut[torch.from_numpy(did).to(lut.device)].cpu().numpy()
        done = (len(prog.keys) + j) in typed
        vals = ids if (done or kc.decoder is None) else kc.decoder(ids)
        key_vals.append(vals)
        cols[kc.name] = vals
    key_names = [kc.name for kc in prog.keys] + [kc.name for kc, _, _ in getattr(prog, "derived", ())]
    if collapse and R:
        # non-injective key formatting: re-aggregate groups that format identically
        tup = list(zip(*[v.tolist() for v in key_vals]))
        uniq = {}
        inv = np.empty(len(tup), dtype=np.int64)
        for i, t in enumerate(tup):
            inv[i] = uniq.setdefault(t, len(uniq))
        R = len(uniq)
        new_cols = {}
        for s, (op, init) in enumerate(prog.slots):
            col = np.full(R, init, dtype=np.int64)
            src = acc_cols[s]
            if op == D.S_SUM_I:
                col[:] = 0
                np.add.at(col, inv, src)
            elif op == D.S_SUM_F:
                cf = np.zeros(R, dtype=np.float64)
                np.add.at(cf, inv, src.view(np.float64) if src.flags.c_contiguous else src.copy().view(np.float64))
                col = cf.view(np.int64)
            elif op == D.S_MIN_I:
                np.minimum.at(col, inv, src)
            else:
                np.maximum.at(col, inv, src)
            new_cols[s] = col
        inv_t = torch.from_numpy(inv)
        new_hll = []
        for h in hll_d:
            hc = h.cpu()
            o = torch.zeros((R, hc.shape[1]), dtype=hc.dtype)
            o.scatter_reduce_(0, inv_t.unsqueeze(1).expand(-1, hc.shape[1]), hc, reduce="amax", include_self=True)
            new_hll.append(o)
        keys_first = [None] * R
        for t, i in uniq.items():
            keys_first[i] = t
        for j, name in enumerate(key_names):
            cols[name] = np.array([t[j] for t in keys_first], dtype=object)
        acc_cols, hll_d = new_cols, new_hll
    derived_names = {}
    for (a, _, _), v in zip(getattr(prog, "derived_aggs", ()), derived_agg_vals):
        v = np.asarray(v, dtype=np.int64)
        derived_names[a.name] = v.astype(np.float64) / (10.0 ** a.scale) if a.scale else \
            (v if a.out_type == "long" else v.astype(np.float64))
    for a in prog.aggs:
        if a.name in derived_names:
            cols[a.name] = derived_names[a.name]
        elif parts.kind == "sparse" and a.name in agg_host:
            cols[a.name] = agg_host[a.name]
        elif a.kind in ("count",):
            cols[a.name] = acc_cols[a.slot]
        elif a.kind in ("sum_i", "min_i", "max_i"):
            v = acc_cols[a.slot]
            if a.scale:
                cols[a.name] = v.astype(np.float64) / (10.0 ** a.scale)
            elif a.out_type == "long":
                cols[a.name] = v
            else:
                cols[a.name] = v.astype(np.float64)
        elif a.kind == "sum_f":
            col = acc_cols[a.slot]
            cols[a.name] = col.view(np.float64) if col.flags.c_contiguous else col.copy().view(np.float64)
        elif a.kind == "sum_fx":
            cols[a.name] = fixed_value(np.asarray(acc_cols[a.slot]), np.asarray(acc_cols[a.slot2]))
        elif a.kind in ("min_f", "max_f"):
            v = ord2f(acc_cols[a.slot]).copy()
            if a.out_type == "long":
                # longMin/longMax over __time: empty groups keep the +-inf identity
                v = np.where(np.isfinite(v), v, 0).astype(np.int64)
            cols[a.name] = v
        elif a.kind == "hll":
            if est_host:
                cols[a.name] = est_host[a.hll_index]
            else:
                cols[a.name] = hll_estimates(hll_d[a.hll_index], prog.hll_p) if R else np.zeros(0)
        elif a.kind in ("theta", "quantile", "distinct", "moment"):
            pass  # filled by the executor
    # group count of the result (only its length is read downstream)
    cols["__rows__"] = acc_cols[0] if 0 in acc_cols else np.zeros(R, dtype=np.int8)
    cols["__gid__"] = gid if not collapse else np.arange(R)
    return cols
