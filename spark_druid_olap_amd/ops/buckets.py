"""Fixed-bucket histograms: bucket edges as exact rationals and their thresholds in a column's
ordered-u64 domain.  Pure host arithmetic that the engine (ops/csrc/histogram.hip), its torch
fallback and the SQL host path share, so every path bins a value the same way.

A histogram of B buckets has edges e_0 < ... < e_B; a value v belongs to bucket i iff
e_i <= v < e_{i+1}, is "below" if v < e_0 and "above" if v >= e_B.  Limits and breaks are read as
the exact decimal value of their shortest round-trip text (0.1 is 1/10), edges are Fractions and
nothing is rounded before the comparison: threshold t_i is the smallest STORED value whose value is
>= e_i, so v >= e_i iff stored(v) >= t_i, and a value's index in [below, c_0 .. c_{B-1}, above] is
the number of thresholds <= it.  NaN (of either sign) counts as "above"."""
from __future__ import annotations

import math
from fractions import Fraction
from typing import List, Optional, Sequence

import numpy as np

MAX_BUCKETS = 1022  # ops/csrc/histogram.h FBH_MAX_BUCKETS
MODES = ("ignore", "overflow")
_SIGN = 1 << 63
_I64_MIN, _I64_MAX = -(1 << 63), (1 << 63) - 1


def exact(v) -> Fraction:
    """The exact decimal value of a limit's shortest round-trip text."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating, Fraction)):
        raise ValueError(f"histogram limit {v!r} is not a number")
    if isinstance(v, (float, np.floating)):
        if not math.isfinite(v):
            raise ValueError(f"histogram limit {v!r} is not finite")
        return Fraction(repr(float(v)))
    return Fraction(v) if isinstance(v, Fraction) else Fraction(int(v))


def bucket_edges(lower=None, upper=None, num_buckets=None, breaks: Optional[Sequence] = None) -> List[Fraction]:
    """The B + 1 edges of ``breaks`` (strictly ascending) when given, else of ``num_buckets`` equal
    buckets over [lower, upper): e_i = lo + i (hi - lo) / B.  ValueError for anything else."""
    if breaks is not None:
        edges = [exact(b) for b in breaks]
        if len(edges) < 2 or any(a >= b for a, b in zip(edges, edges[1:])):
            raise ValueError("histogram breaks must be at least two strictly ascending numbers")
    else:
        if isinstance(num_buckets, bool) or not isinstance(num_buckets, (int, np.integer)):
            raise ValueError(f"histogram numBuckets {num_buckets!r} is not an integer")
        if lower is None or upper is None:
            raise ValueError("histogram needs lowerLimit and upperLimit, or breaks")
        lo, hi, n = exact(lower), exact(upper), int(num_buckets)
        if n < 1 or lo >= hi:
            raise ValueError("histogram needs numBuckets >= 1 and lowerLimit < upperLimit")
        edges = [lo + i * (hi - lo) / n for i in range(n + 1)]
    if len(edges) - 1 > MAX_BUCKETS:
        raise ValueError(f"histogram of {len(edges) - 1} buckets: at most {MAX_BUCKETS}")
    return edges


def f2ord(f: float) -> int:
    """The signed order of a double's bits (ops/csrc/sdo_device.h f2ord): -0.0 is -1, +0.0 is 0."""
    b = int(np.array([f], dtype=np.float64).view(np.int64)[0])
    return b if b >= 0 else b ^ 0x7FFFFFFFFFFFFFFF


# ordered values below this are NaNs with the sign bit set (they order below -inf)
NAN_LO = (f2ord(-math.inf) + _SIGN) & (2 * _SIGN - 1)


def bucket_thresholds(edges: Sequence[Fraction], kind: str, scale: int = 0) -> np.ndarray:
    """Per edge the smallest stored value of a ``kind`` ("long" | "decimal" of ``scale`` digits |
    "double") column whose value is >= the edge, under the producer's order-preserving u64 map
    (int64 with the sign bit flipped, doubles through f2ord first): uint64 [B + 1], ascending.  An
    edge at zero takes the ordered value of -0.0, which f2ord orders below +0.0 but equals it."""
    out = []
    for e in edges:
        if kind == "double":
            try:
                t = float(e)  # (correctly rounded)
            except OverflowError:
                t = math.copysign(math.inf, e)
            if t == math.inf:
                raise ValueError("histogram edge beyond the largest double")
            if t != -math.inf and Fraction(t) < e:
                t = math.nextafter(t, math.inf)
            s = f2ord(-0.0 if t == 0.0 else t)
        else:
            s = max(math.ceil(e * 10 ** int(scale) if kind == "decimal" else e), _I64_MIN)
            if s > _I64_MAX:
                raise ValueError("histogram edge beyond the column's int64 range")
        out.append((s + _SIGN) & (2 * _SIGN - 1))
    return np.asarray(out, dtype=np.uint64)


def ordered(values: np.ndarray, kind: str) -> np.ndarray:
    """Stored values (int64 digits for long / decimal, float64 for double) under the same u64 map;
    NaNs of either sign map to the largest u64."""
    if kind == "double":
        v = np.ascontiguousarray(values, dtype=np.float64)
        b = v.view(np.int64)
        o = np.where(b >= 0, b, b ^ np.int64(0x7FFFFFFFFFFFFFFF)).view(np.uint64) ^ np.uint64(_SIGN)
        return np.where(np.isnan(v), np.uint64(2 * _SIGN - 1), o)
    return np.ascontiguousarray(values, dtype=np.int64).view(np.uint64) ^ np.uint64(_SIGN)


def slots(values: np.ndarray, thresholds: np.ndarray, kind: str) -> np.ndarray:
    """Per stored value its index in [below, c_0 .. c_{B-1}, above]: the thresholds <= it."""
    return np.searchsorted(thresholds, ordered(values, kind), side="right")


def apply_mode(counts: np.ndarray, mode: str) -> np.ndarray:
    """``counts`` [..., B + 2] under the outlier mode: "ignore" as is; "overflow" adds below into
    c_0 and above into c_{B-1} and reports 0 in the two end slots."""
    if mode == "ignore":
        return counts
    if mode != "overflow":
        raise ValueError(f"histogram: unknown outlierHandlingMode {mode!r}")
    out = counts.copy()
    out[..., 1] += out[..., 0]
    out[..., -2] += out[..., -1]
    out[..., 0] = out[..., -1] = 0
    return out
