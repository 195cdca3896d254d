"""LIKE / contains / fragment over a materialized string dictionary, matched on the device.

The predicate is compiled into the matcher kernel's fixed-size pattern program
(ops/csrc/dict_match.h ``DmProgram``), the kernel answers one bit per dictionary entry from the
dictionary's device text heap (segment/textheap.py), and the host unpacks the bits into the bool
mask an ``("ids", dim, mask)`` leaf carries -- constant folding, mask statistics and the bitset
upload downstream are unchanged.  Anything the program cannot hold (more than 8 segments, a
segment over 256 positions) and every dictionary the heap declines returns None: the caller's host
path answers, as before.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from ..segment.dictionary import Dictionary
from ..segment.textheap import text_heap

MAX_SEGS = 8
MAX_SEG_LEN = 256
ANCHOR_START, ANCHOR_END, FOLD, ALL = 1, 2, 4, 8

PROGRAM = np.dtype([("nseg", "<i4"), ("flags", "<i4"), ("len", "<u2", (MAX_SEGS,)),
                    ("lit", "u1", (MAX_SEGS, MAX_SEG_LEN)), ("any", "<u4", (MAX_SEGS, MAX_SEG_LEN // 32))])

# Dictionary cardinality from which the device answers: the smallest measured cardinality at which
# the device path -- program compile, launch, the copy back, unpack, recheck -- beats the host for
# LIKE '%abc%', LIKE 'abc%' and insensitive_contains alike, at mean entry lengths of ~24 and ~96
# bytes (profiles/dict_match_probe.json, one MI355X, tools/dict_match_probe.py).  At 1,000 entries:
# host 0.15-0.22 ms, device 0.03-0.09 ms; at 100 the host's 0.02 ms insensitive_contains loop still
# wins against 0.04-0.08 ms.  The one-time heap build and upload (0.3-6 ms at 1,000 entries, ~140 ms at
# 10^6) is not part of the comparison.
DEVICE_MIN_CARD = 1000

_ANY = None  # a '_' position in a segment (literal positions are ints 0..255)


def _pack(segs: Sequence[list], flags: int) -> Optional[np.ndarray]:
    if len(segs) > MAX_SEGS or any(len(s) > MAX_SEG_LEN for s in segs):
        return None
    p = np.zeros((), dtype=PROGRAM)
    p["nseg"], p["flags"] = len(segs), flags
    for i, s in enumerate(segs):
        p["len"][i] = len(s)
        for j, c in enumerate(s):
            if c is _ANY:
                p["any"][i, j >> 5] |= np.uint32(1 << (j & 31))
            else:
                p["lit"][i, j] = c
    return p


def compile_like(pattern: str) -> Optional[np.ndarray]:
    """SQL LIKE -> program, with the escapes of sql/functions.py like_to_regex: split at unescaped
    '%', '_' is one code point, backslash-x is the literal x.  None: does not fit."""
    try:
        pattern.encode("utf-8")
    except UnicodeEncodeError:
        return None
    pieces: List[list] = [[]]
    i = 0
    while i < len(pattern):
        c = pattern[i]
        if c == "\\" and i + 1 < len(pattern):
            pieces[-1].extend(pattern[i + 1].encode("utf-8"))
            i += 2
            continue
        if c == "%":
            pieces.append([])
        elif c == "_":
            pieces[-1].append(_ANY)
        else:
            pieces[-1].extend(c.encode("utf-8"))
        i += 1
    if len(pieces) == 1:  # no '%': the whole entry
        return _pack(pieces, ANCHOR_START | ANCHOR_END)
    flags = (ANCHOR_START if pieces[0] else 0) | (ANCHOR_END if pieces[-1] else 0)
    return _pack([p for p in pieces if p], flags)


def compile_needles(needles: Sequence[str], fold: bool) -> Optional[np.ndarray]:
    """contains (one needle) / fragment (all needles present), case-folded or not.  Folded needles
    arrive already lowered (``str.lower``), as the host predicates compare them."""
    try:
        segs = [list(s.encode("utf-8")) for s in needles]
    except UnicodeEncodeError:
        return None
    return _pack(segs, (FOLD if fold else 0) | (ALL if len(segs) != 1 else 0))


def match_mask(d: Dictionary, dev, program: Optional[np.ndarray],
               recheck: Optional[Callable[[object], bool]] = None) -> Optional[np.ndarray]:
    """bool[len(d)]: the entries ``program`` matches (the NULL id never does), or None when the
    device path declines.  ``recheck``: the exact host predicate of a case-folding program, applied
    to the entries the kernel flags as non-ASCII."""
    from ..ops import native

    if program is None:
        return None
    th = text_heap(d, dev)
    if th is None:
        return None
    fold = bool(int(program["flags"]) & FOLD)
    assert recheck is not None or not fold
    n, nw = th.n, (th.n + 63) // 64
    words = torch.empty(nw * (2 if fold else 1), dtype=torch.int64, device=th.heap.device)
    native.dict_match(th.heap, th.offsets, n, th.text_bytes, program.tobytes(), words, nw if fold else 0)
    host = words.cpu().numpy().view(np.uint8)  # the one copy back (both bitsets); waits for the kernel
    bits = np.unpackbits(host, bitorder="little").view(np.bool_)
    off = 1 if d.has_null else 0
    out = np.zeros(len(d), dtype=bool)
    out[off:] = bits[:n]
    if fold:
        vals = d.values
        for i in np.flatnonzero(bits[nw * 64: nw * 64 + n]).tolist():
            out[i + off] = bool(recheck(vals[i]))
    return out
