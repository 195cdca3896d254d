"""Device text heap of a materialized string dictionary.

The UTF-8 bytes of all (non-NULL) entries back to back in id order plus ``n + 1`` u32 byte offsets,
uploaded once per (dictionary, device) on first use: what the matcher kernel (ops/csrc/dict_match.hip)
reads to answer LIKE / contains / fragment predicates per entry.  The NULL id has no bytes -- the
heap starts at the first real value and the caller shifts the verdicts by ``has_null``.

Declined (``None``: the caller's host path answers) for lazy dictionaries -- Range / Formatted /
Words keep their own ``id_range`` / ``like_mask`` paths -- non-string dictionaries, entries that are
not valid UTF-8 strings, heaps of 4 GiB or more (u32 offsets) and heaps over the budget share below.
"""
from __future__ import annotations

import threading
import weakref
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ..utils.memory import RUNTIME_RESERVE, dict_cache_bytes, note_dict_cache_bytes
from ..utils.streams import publish
from .dictionary import STRING, Dictionary

HEAP_MAX_BYTES = (1 << 32) - 64   # u32 offsets, with room for the 16-byte padding
# All text heaps of a device together stay under this share of its budget (device memory less the
# runtime reserve of utils/memory.py).  The heaps are a lowering-time convenience next to what the
# scans need -- the columns themselves, the slot arenas, partition scratch, cached scan buffers --
# and, unlike the scan buffers, nothing evicts them (device_exec.release_device_memory does not
# know them): an eighth bounds what an out-of-memory retry cannot win back, and on a 288 GB device
# still admits eight 4 GiB dictionaries.
HEAP_BUDGET_SHARE = 1.0 / 8.0

_lock = threading.Lock()


@dataclass
class TextHeap:
    heap: torch.Tensor      # uint8 [padded], 16-byte aligned, zero padded to a multiple of 16
    offsets: torch.Tensor   # int32 view of the u32 byte offsets [n + 1]
    n: int                  # non-NULL entries
    text_bytes: int

    @property
    def nbytes(self) -> int:
        return self.heap.numel() + self.offsets.numel() * 4


def encode(values: np.ndarray):
    """(uint8 bytes, int64 offsets [n + 1]) of an object array of str, or None when an entry is not
    a str or has no UTF-8 encoding (a lone surrogate)."""
    n = len(values)
    try:
        import pyarrow as pa
    except ImportError:
        pa = None
    try:
        if pa is not None:
            # (the string array's own buffers: no per-entry Python work)
            arr = pa.array(values, type=pa.large_string(), from_pandas=False)
            if arr.null_count:
                return None
            bufs = arr.buffers()
            off = np.frombuffer(bufs[1], dtype=np.int64, count=n + 1) if n else np.zeros(1, dtype=np.int64)
            data = np.frombuffer(bufs[2], dtype=np.uint8, count=int(off[-1])) if int(off[-1]) else np.zeros(0, np.uint8)
            return data, off
        enc = [v.encode("utf-8") for v in values.tolist()]
    except Exception:  # ArrowTypeError / ArrowInvalid / AttributeError / UnicodeEncodeError
        return None
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.fromiter((len(b) for b in enc), dtype=np.int64, count=n), out=off[1:])
    return np.frombuffer(b"".join(enc), dtype=np.uint8), off


def _budget(dev: torch.device) -> int:
    total = torch.cuda.get_device_properties(dev).total_memory
    return int(max(0, total - RUNTIME_RESERVE) * HEAP_BUDGET_SHARE)


def text_heap(d: Dictionary, dev) -> Optional[TextHeap]:
    """The dictionary's heap on ``dev`` (built and uploaded on first use), or None when declined."""
    if getattr(d, "lazy", False) or d.vtype != STRING:
        return None
    dev = torch.device(dev)
    cache = d.__dict__.setdefault("_text_heaps", {})
    key = str(dev)
    if key in cache:
        return cache[key]
    with _lock:
        if key in cache:
            return cache[key]
        cache[key] = _build(d, dev)
        return cache[key]


def _build(d: Dictionary, dev: torch.device) -> Optional[TextHeap]:
    enc = encode(d.values)
    if enc is None:
        return None
    data, off = enc
    nbytes = int(off[-1])
    n = len(off) - 1
    if n == 0 or nbytes > HEAP_MAX_BYTES:
        return None
    padded = (nbytes + 15) // 16 * 16 + 16
    if dev.type == "cuda" and dict_cache_bytes(dev) + padded + 4 * (n + 1) > _budget(dev):
        return None
    host = np.zeros(padded, dtype=np.uint8)
    host[:nbytes] = data
    heap = torch.from_numpy(host).to(dev)
    offsets = torch.from_numpy(off.astype(np.uint32).view(np.int32)).to(dev)
    assert heap.data_ptr() % 16 == 0
    th = TextHeap(heap, offsets, n, nbytes)
    note_dict_cache_bytes(dev, th.nbytes)
    weakref.finalize(d, note_dict_cache_bytes, dev, -th.nbytes)
    # (every slot's stream reads it: complete before it is visible)
    return publish(th, dev)
