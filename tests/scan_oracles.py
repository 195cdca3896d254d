"""Synthetic shards and plain oracles for the scan kernels' time fields, expressions and filters.

Everything expected here is computed with ``datetime`` / ``calendar`` / ``math`` and numpy on the
host arrays.  The oracles deliberately import nothing from ``ops.reference``, ``query.granularity``,
``query.intervals`` or ``query.joda``: the engine's reference executor, its host bucket arithmetic
and the device kernels all share one civil-from-days algorithm, and a mistake common to them is
only visible from outside.

Shards (``shard(name)`` builds them on the CPU, ``.to("cuda")`` moves them):

* ``cal_minutes`` -- minute unit, 1899..2101, 3 264 rows, no time lookup table (span > 65 536 units)
* ``epoch_ms``    -- millisecond unit, +-20 days around the epoch, 4 197 rows
* ``secs_wide``   -- second unit, 30 days across 2024-02-29, 4 197 rows, arithmetic path
* ``secs_lut``    -- second unit, 12 hours across 2023-12-31/2024-01-01, 4 197 rows, table path
* ``values``      -- one day, 4 197 rows, one metric per storage type the kernels read

4 197 = 4 096 + 64 + 37 rows: a full chunk, a full 64-row word and a partial last word.  Every shard
has a ``row`` dimension (one id per row, so one query reports per-row results) and a small ``grp``
dimension.

``epoch_ms`` cannot hold +-1 ms around *every* second boundary of two days (172 800 boundaries) in
4 197 rows.  It holds b-1, b, b+1 for every day and hour boundary of 1969-12-31 and 1970-01-01,
for the first and last minute and second boundaries of each of their 48 hours, and for every
minute boundary within ten minutes and every second boundary within twenty seconds of the epoch;
the rest is seeded uniform.
"""
import calendar
import collections
import datetime as dt
import math

import numpy as np
import torch

N = 4096 + 64 + 37
EPOCH = dt.datetime(1970, 1, 1)
MS = dt.timedelta(milliseconds=1)
INTERVAL = ["1800-01-01/2200-01-01"]

# (spelling accepted by engine.lower.tz_offset_ms, offset in ms): a positive offset with a half
# hour, and a negative one
ZONES = [("+05:30", (5 * 60 + 30) * 60_000), ("-08:00", -8 * 3_600_000)]
TIME_SHARDS = ["cal_minutes", "epoch_ms", "secs_wide", "secs_lut"]
T_QOY = 16  # scan_desc.h TField (the oracles import no engine calendar code; the CPU test checks the value)


# --------------------------------------------------------------------------------------- shards
class Shard:
    def __init__(self, ds, ms, cols):
        self.ds = ds
        self.ms = ms          # int64 epoch ms per row (python ints via .tolist() for datetime)
        self.cols = cols      # host numpy columns, first N rows only
        self.n = len(ms)

    def to(self, device):
        return Shard(self.ds.to(device), self.ms, self.cols)


def _ms_of(y, m, d, minutes=0):
    return ((dt.datetime(y, m, d) - EPOCH) // MS) + minutes * 60_000


def _time_values(name):
    rng = np.random.default_rng({"cal_minutes": 11, "epoch_ms": 12, "secs_wide": 13, "secs_lut": 14}[name])
    if name == "cal_minutes":
        v = []
        for y in (1899, 1900, 1903, 1904, 1969, 1970, 1999, 2000, 2001, 2099, 2100):
            for m, d in ((1, 1), (2, 28), (3, 1), (6, 30), (7, 1), (12, 31)):
                for off in (-1, 0, 1, 1439):
                    v.append(_ms_of(y, m, d, off) // 60_000)
        lo, hi = _ms_of(1899, 12, 25) // 60_000, _ms_of(2101, 3, 5) // 60_000
        v += rng.integers(lo, hi, 3000).tolist()
        assert len(v) == 3264
        return np.sort(np.asarray(v, dtype=np.int64)), 60_000
    if name == "epoch_ms":
        day, hour = 86_400_000, 3_600_000
        b = {k * hour for k in range(-24, 25)}  # every hour and day boundary of both days
        for h in range(-24, 24):  # each hour's first and last minute and second boundaries
            b |= {h * hour + k * 60_000 for k in (1, 2, 58, 59)} | {h * hour + k * 1000 for k in (1, 2, 59, 61, 3541, 3599)}
        b |= {k * 60_000 for k in range(-10, 11)} | {k * 1000 for k in range(-20, 21)}  # and around the epoch
        v = sorted({x + e for x in b for e in (-1, 0, 1)})
        fill = N - len(v)
        assert fill > 2000
        v += rng.integers(-20 * day, 0, fill // 2).tolist() + rng.integers(0, 20 * day + 1, fill - fill // 2).tolist()
        v = np.sort(np.asarray(v, dtype=np.int64))
        assert len(v) == N and (v < 0).sum() >= 1000 and {-1, 0, 1} <= set(v.tolist())
        return v, 1
    if name == "secs_wide":
        lo, hi = _ms_of(2024, 2, 14) // 1000, _ms_of(2024, 3, 15) // 1000
        edges = [_ms_of(2024, 2, 29) // 1000 + e for e in (-1, 0, 1)] + \
                [_ms_of(2024, 3, 1) // 1000 + e for e in (-1, 0, 1)] + [lo, hi - 1]
        v = edges + rng.integers(lo, hi, N - len(edges)).tolist()
        return np.sort(np.asarray(v, dtype=np.int64)), 1000
    if name == "secs_lut":
        mid = _ms_of(2024, 1, 1) // 1000
        lo, hi = mid - 6 * 3600, mid + 6 * 3600
        edges = [mid + e for e in (-3601, -3600, -61, -60, -2, -1, 0, 1, 59, 60, 3599, 3600)] + [lo, hi - 1]
        v = edges + rng.integers(lo, hi, N - len(edges)).tolist()
        return np.sort(np.asarray(v, dtype=np.int64)), 1000
    raise KeyError(name)


F64_SPECIAL = [0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 1e-300, 1e300, math.inf, -math.inf, math.nan,
               1.0, -1.0, 2.0, -2.0, 7.25, -7.25, 100.0]
F64_Y = [3.0, -3.0, 0.0, 2.5, -2.5, 0.5, 2.0, -2.0, math.nan, 1.0, -0.0, math.inf]


def _value_columns(n):
    """Host columns of the ``values`` shard.  Rows [0, len(F64_SPECIAL) * len(F64_Y)) pair every
    special ``f64`` with every ``y``; the integer extremes sit in the first rows and again in the
    last partial word, and 0 occurs in real rows of every column."""
    rng = np.random.default_rng(5)
    c = {}

    def ints(dtype, lo, hi, edge):
        v = rng.integers(lo, hi, n, dtype=np.int64)
        e = np.asarray(edge, dtype=np.int64)
        v[:len(e)] = e
        v[n - len(e):] = e[::-1]
        return v.astype(dtype)

    c["u8"] = ints(np.uint8, 0, 256, [0, 255, 1, 0])
    c["i16"] = ints(np.int16, -300, 300, [-32768, 32767, -1, 0, 1])
    c["i32"] = ints(np.int32, -10**6, 10**6, [-2**31, 2**31 - 1, -1, 0, 1])
    c["i64"] = ints(np.int64, -10**12, 10**12, [-2**62, 2**62, -1, 0, 1])
    c["i64"][n - 2:] = [2**61, -2**61]  # +-2^62 once each: no group's sum can wrap
    c["dec"] = ints(np.int32, -10**6, 10**6, [0, 1, -1, 999_999_99, -999_999_99, 5, 15, 25])  # cents
    ns, ny = len(F64_SPECIAL), len(F64_Y)
    x = np.round(rng.uniform(-100, 100, n) * 4) / 4  # quarters: halves and integers occur
    y = np.asarray(F64_Y)[rng.integers(0, 8, n)]
    k = np.arange(ns * ny)
    x[:ns * ny] = np.asarray(F64_SPECIAL)[k % ns]
    y[:ns * ny] = np.asarray(F64_Y)[k // ns]
    x[n - ns:] = np.asarray(F64_SPECIAL)  # specials in the partial last word too
    c["f64"], c["y"] = x, y
    with np.errstate(over="ignore"):
        f = x.astype(np.float32)  # 1e-300 -> 0, 1e300 -> inf: float32 keeps its own extremes below
    f[ns * ny: ns * ny + 4] = [np.float32(1e-38), np.float32(3e38), np.float32(0.1), np.float32(-0.1)]
    c["f32"] = f
    return c


_CACHE = {}


def shard(name):
    """The named shard on the CPU (built once per process)."""
    if name in _CACHE:
        return _CACHE[name]
    from spark_druid_olap_amd.segment.datasource import make_datasource
    from spark_druid_olap_amd.segment.dictionary import Dictionary, RangeDictionary

    if name == "values":
        n, unit = N, 86_400_000
        t = np.full(n, _ms_of(2020, 2, 29) // unit, dtype=np.int64)
        cols = _value_columns(n)
    else:
        t, unit = _time_values(name)
        n = len(t)
        cols = {}
    row = np.arange(n, dtype=np.int64)
    grp = (row * 7919 + 3) % 7
    grp[:3] = [0, 6, 0]
    dnum = (row * 31) % 11  # numeric dimension: ids 0..10 are the values -5 .. 5
    cols.update(row=row, grp=grp, dnum=dnum)
    dims = {k: torch.from_numpy(cols[k]) for k in ("row", "grp", "dnum")}
    dicts = {"row": RangeDictionary(0, n), "grp": Dictionary([f"g{i}" for i in range(7)]),
             "dnum": Dictionary(list(range(-5, 6)), "long")}
    mcols = [k for k in cols if k not in dims]
    kinds = {k: ("decimal" if k == "dec" else "double" if cols[k].dtype.kind == "f" else "long") for k in mcols}
    ds = make_datasource(name, n, torch.from_numpy(t), unit, dims, dicts,
                         {k: torch.from_numpy(cols[k]) for k in mcols}, kinds, {"dec": 2},
                         segment_granularity="year")
    ds.build_indexes()
    out = _CACHE[name] = Shard(ds, t * unit, cols)
    return out


# ------------------------------------------------------------------------------- time oracles
def local(ms, tz_ms=0):
    """Wall-clock datetime of an epoch-ms instant at a fixed offset."""
    return EPOCH + dt.timedelta(milliseconds=int(ms) + tz_ms)


def instant(d, tz_ms=0):
    """UTC epoch ms of a wall-clock datetime at a fixed offset."""
    return (d - EPOCH) // MS - tz_ms


_FMT = {
    "yyyy": lambda d: f"{d.year:04d}", "YYYY": lambda d: f"{d.year:04d}",
    "yyyy-MM": lambda d: f"{d.year:04d}-{d.month:02d}",
    "yyyy-MM-dd": lambda d: f"{d.year:04d}-{d.month:02d}-{d.day:02d}",
    "YYYY-MM-dd": lambda d: f"{d.year:04d}-{d.month:02d}-{d.day:02d}",
    "MM": lambda d: f"{d.month:02d}", "M": lambda d: str(d.month),
    "MMM": lambda d: calendar.month_abbr[d.month], "MMMM": lambda d: calendar.month_name[d.month],
    "dd": lambda d: f"{d.day:02d}", "d": lambda d: str(d.day),
    "EEEE": lambda d: calendar.day_name[d.weekday()], "EEE": lambda d: calendar.day_abbr[d.weekday()],
    "E": lambda d: calendar.day_abbr[d.weekday()], "e": lambda d: str(d.isoweekday()),
    "HH": lambda d: f"{d.hour:02d}", "H": lambda d: str(d.hour), "mm": lambda d: f"{d.minute:02d}",
    "ss": lambda d: f"{d.second:02d}", "D": lambda d: str(d.timetuple().tm_yday),
    "DDD": lambda d: f"{d.timetuple().tm_yday:03d}",
    "yyyy-MM-dd HH": lambda d: d.strftime("%Y-%m-%d %H").zfill(13),
    "yyyy-MM-dd'T'HH": lambda d: d.strftime("%Y-%m-%dT%H").zfill(13),
    "yyyy-MM-dd HH:mm": lambda d: d.strftime("%Y-%m-%d %H:%M").zfill(16),
    "yyyy-MM-dd HH:mm:ss": lambda d: d.strftime("%Y-%m-%d %H:%M:%S").zfill(19),
    "yyyy-MM-dd'T'HH:mm:ss": lambda d: d.strftime("%Y-%m-%dT%H:%M:%S").zfill(19),
}
FORMATS = sorted(_FMT)


def format_labels(ms, fmt, tz_ms=0):
    f = _FMT[fmt]
    return [f(local(m, tz_ms)) for m in ms.tolist()]


def _trunc(d, name):
    if name == "second":
        return d.replace(microsecond=0)
    if name == "minute":
        return d.replace(second=0, microsecond=0)
    if name == "hour":
        return d.replace(minute=0, second=0, microsecond=0)
    day = d.replace(hour=0, minute=0, second=0, microsecond=0)
    if name == "day":
        return day
    if name == "week":  # ISO weeks start on Monday
        return day - dt.timedelta(days=d.isoweekday() - 1)
    if name == "month":
        return day.replace(day=1)
    if name == "quarter":
        return day.replace(month=(d.month - 1) // 3 * 3 + 1, day=1)
    if name == "year":
        return day.replace(month=1, day=1)
    raise KeyError(name)


# name -> (granularity JSON the engine parses, calendar truncation or (period ms, origin ms))
DURATION_ORIGIN = 1_234_567  # 00:20:34.567 after the epoch: not a multiple of any unit
GRANULARITIES = {
    "none": ("none", (1, 0)),
    **{g: (g, g) for g in ("second", "minute", "hour", "day", "week", "month", "quarter", "year")},
    "fifteen_minute": ("fifteen_minute", (900_000, 0)),
    "duration": ({"type": "duration", "duration": 7_200_000, "origin": DURATION_ORIGIN}, (7_200_000, DURATION_ORIGIN)),
    "PT6H": ({"type": "period", "period": "PT6H"}, (6 * 3_600_000, 0)),
    "P1M": ({"type": "period", "period": "P1M"}, "month"),
    "P3M": ({"type": "period", "period": "P3M"}, "quarter"),
    "P1Y": ({"type": "period", "period": "P1Y"}, "year"),
}


def bucket_starts(ms, gname, tz_ms=0):
    """UTC epoch ms of the start of each row's granularity bucket, in wall-clock time at tz_ms.
    Calendar buckets (second .. year, P1M / P3M / P1Y) are what ``datetime`` truncation gives.
    For fixed-length buckets with a zone (none, fifteen_minute, duration, PT6H) there is no outside
    authority: "count whole periods from the origin on the wall clock" is the engine's own
    convention (KOp.tz_ms is added before T_PERIOD divides), written here with timedelta
    arithmetic; what the oracle adds for them is the floor division on negative instants."""
    how = GRANULARITIES[gname][1]
    out = []
    for m in ms.tolist():
        d = local(m, tz_ms)
        if isinstance(how, str):
            out.append(instant(_trunc(d, how), tz_ms))
        else:
            period, origin = dt.timedelta(milliseconds=how[0]), local(how[1])
            out.append(instant(origin + ((d - origin) // period) * period, tz_ms))
    return out


def counts(labels):
    return dict(collections.Counter(labels))


# ------------------------------------------------------------------------- expression oracles
def _fmod(a, b):
    try:
        return math.fmod(a, b)
    except ValueError:  # fmod(x, 0), fmod(inf, y): IEEE 754 invalid -> NaN
        return math.nan


def _pmod(a, b):
    """Spark's Pmod on doubles: r = fmod(a, b); r < 0 -> fmod(r + b, b)."""
    r = _fmod(a, b)
    return _fmod(r + b, b) if r < 0 else r


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(a):
    return math.sqrt(a) if a >= 0 else math.nan if a == a else a


def _log(a):
    if a != a or a < 0:
        return math.nan
    return -math.inf if a == 0 else math.log(a)


def _exp(a):
    try:
        return math.exp(a)
    except OverflowError:
        return math.inf


def _pow(a, b):
    """IEEE 754 / C pow (python's ** raises or goes complex where C returns inf or NaN)."""
    try:
        return math.pow(a, b)
    except OverflowError:
        return -math.inf if a < 0 and float(b).is_integer() and int(b) % 2 else math.inf
    except ValueError:  # negative base with a non-integer exponent -> NaN; 0 ** negative -> inf
        if a == 0:
            return -math.inf if math.copysign(1, a) < 0 and float(b).is_integer() and int(b) % 2 else math.inf
        return math.nan


def _fminmax(pick):
    """C fmin / fmax: a NaN operand is ignored (the rule the kernels and the reference follow,
    see E_MIN in scan_desc.h); NaN only when both are."""
    def f(a, b):
        if a != a:
            return b
        if b != b:
            return a
        return pick(a, b)
    return f


EXPR_ORACLE = {
    "add": lambda a, b: a + b, "sub": lambda a, b: a - b, "mul": lambda a, b: a * b, "div": _div,
    "neg": lambda a: -a, "abs": abs, "floor": lambda a: float(np.floor(a)), "ceil": lambda a: float(np.ceil(a)),
    "sqrt": _sqrt, "log": _log, "exp": _exp, "mod": _fmod, "pmod": _pmod, "pow": _pow,
    "min": _fminmax(min), "max": _fminmax(max),
}
# javascript text of each operation over two operands
EXPR_JS = {
    "add": "{a} + {b}", "sub": "{a} - {b}", "mul": "{a} * {b}", "div": "{a} / {b}", "neg": "-{a}",
    "abs": "Math.abs({a})", "floor": "Math.floor({a})", "ceil": "Math.ceil({a})", "sqrt": "Math.sqrt({a})",
    "log": "Math.log({a})", "exp": "Math.exp({a})", "mod": "{a} % {b}", "pmod": "Math.pmod({a}, {b})",
    "pow": "Math.pow({a}, {b})", "min": "Math.min({a}, {b})", "max": "Math.max({a}, {b})",
}
EXACT_OPS = ("add", "sub", "mul", "div", "neg", "abs", "floor", "ceil", "sqrt", "mod", "pmod", "min", "max")
ULP_OPS = ("log", "exp", "pow")  # within 4 ulp: host libm and the device math library are each <= 2 ulp


def expr_expected(op, a, b):
    f = EXPR_ORACLE[op]
    if op in ("neg", "abs", "floor", "ceil", "sqrt", "log", "exp"):
        return np.asarray([f(x) for x in a.tolist()], dtype=np.float64)
    return np.asarray([f(x, y) for x, y in zip(a.tolist(), b.tolist())], dtype=np.float64)


def _ordered(x):
    """float64 -> int64 whose integer order is the numeric order (adjacent values differ by 1)."""
    b = np.asarray(x, dtype=np.float64).view(np.int64)
    return np.where(b >= 0, b, np.int64(-2**63) - b)


def assert_float_rows(got, want, ulp=0, what=""):
    """NaN equals NaN; ulp == 0 compares bit patterns (so -0.0 != 0.0), else at most ulp steps."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = gn != wn
    ok = ~(gn | wn)
    if ulp == 0:
        bad |= ok & (got.view(np.int64) != want.view(np.int64))
    else:
        d = np.abs(_ordered(np.where(ok, got, 0.0)).astype(object) - _ordered(np.where(ok, want, 0.0)).astype(object))
        bad |= ok & (d > ulp).astype(bool)
    idx = np.nonzero(bad)[0]
    assert len(idx) == 0, f"{what}: {len(idx)} rows differ, first {[(int(i), got[i], want[i]) for i in idx[:6]]}"


def per_row(result, name, n):
    """Column ``name`` of a result grouped by ``row``, as an array indexed by row (every row must
    be present exactly once)."""
    rows = np.asarray([int(r) for r in result.data["row"]])
    assert len(rows) == n and len(set(rows.tolist())) == n, (len(rows), n)
    out = np.empty(n, dtype=np.asarray(result.data[name]).dtype)
    out[rows] = np.asarray(result.data[name])
    return out


def single_row_value(mx, mn, what=""):
    """The value of a one-row group from its ``Math.max`` and ``Math.min`` aggregates.  Both keep
    the row's exact bits (a sum would turn -0.0 into 0.0).  A NaN orders above +inf or below -inf
    depending on its sign bit, so exactly one of the two aggregates sees it and the other stays
    at its reset value."""
    mx, mn = np.asarray(mx, dtype=np.float64), np.asarray(mn, dtype=np.float64)
    nan = np.isnan(mx) | np.isnan(mn)
    other = np.where(np.isnan(mx), mn == np.inf, mx == -np.inf)
    assert bool((other | ~nan).all()), what
    same = mx.view(np.int64) == mn.view(np.int64)
    assert bool((same | nan).all()), (what, np.nonzero(~(same | nan))[0][:6])
    return np.where(nan, np.nan, mx)


# ------------------------------------------------------------------------------ query checks
# timeFormat patterns run together: field extracts whose domains multiply to <= 2^16 share one
# query (and one JIT compile); patterns over absolute buckets run alone
FORMAT_GROUPS = {
    "date_fields": [["MM", "dd", "e", "HH"], ["MMM", "EEE", "mm"], ["D"]],
    "name_fields": [["M", "d", "E", "H"], ["MMMM", "EEEE", "ss"], ["DDD"]],
    "dates": [["yyyy", "YYYY"], ["yyyy-MM"], ["yyyy-MM-dd"], ["YYYY-MM-dd"]],
    "datetimes": [["yyyy-MM-dd HH"], ["yyyy-MM-dd'T'HH"], ["yyyy-MM-dd HH:mm"], ["yyyy-MM-dd HH:mm:ss"],
                  ["yyyy-MM-dd'T'HH:mm:ss"]],
}
assert sorted(f for gs in FORMAT_GROUPS.values() for g in gs for f in g) == FORMATS


def _same_counts(got, want, what):
    if got != want:
        miss = [(k, want[k], got.get(k)) for k in want if got.get(k) != want[k]][:5]
        extra = [(k, got[k]) for k in got if k not in want][:5]
        raise AssertionError(f"{what}: {len(got)} groups, oracle {len(want)}; wrong/missing (key, oracle, got) "
                             f"{miss}; not in oracle {extra}")


def format_query(sh, formats, zone):
    from spark_druid_olap_amd.query import spec as S

    dims = [S.ExtractionDimensionSpec("__time", f"t{i}", S.TimeFormatExtractionFunctionSpec(f, zone))
            for i, f in enumerate(formats)]
    return S.GroupByQuerySpec(sh.ds.name, dims, aggregations=[S.FunctionAggregationSpec("count", "c")],
                              intervals=INTERVAL)


def check_formats(engine, sh, zone, groups):
    """Group by timeFormat labels; labels and per-label counts equal the datetime oracle's."""
    tz_ms = dict(ZONES)[zone]
    for formats in groups:
        r = engine.execute(format_query(sh, formats, zone), sh.ds)
        got = {tuple(r.data[f"t{i}"][j] for i in range(len(formats))): int(r.data["c"][j]) for j in range(r.num_rows)}
        assert len(got) == r.num_rows, f"{formats}: duplicate labels"
        want = counts(zip(*[format_labels(sh.ms, f, tz_ms) for f in formats]))
        _same_counts(got, want, f"{sh.ds.name} timeFormat {formats} {zone}")


def granularity_query(sh, gname, zone):
    """Period granularities take the zone the way a query spells it (``timeZone``).  The simple
    names and ``duration`` have no zone in the query language: for them ``tz_ms`` is set on the
    parsed spec, which the engine supports but no JSON can express."""
    import dataclasses

    from spark_druid_olap_amd.query import spec as S
    from spark_druid_olap_amd.query.granularity import Granularity

    j = GRANULARITIES[gname][0]
    if isinstance(j, dict) and j["type"] == "period":
        g = Granularity.parse(dict(j, timeZone=zone))
        assert g.tz_ms == dict(ZONES)[zone]
    else:
        g = dataclasses.replace(Granularity.parse(j), tz_ms=dict(ZONES)[zone])
    return S.GroupByQuerySpec(sh.ds.name, [], granularity=g, aggregations=[S.FunctionAggregationSpec("count", "c")],
                              intervals=INTERVAL)


def check_granularities(engine, sh, zone, names=None):
    """Bucket timestamps (UTC instants) and per-bucket counts equal the datetime oracle's."""
    tz_ms = dict(ZONES)[zone]
    for gname in names or list(GRANULARITIES):
        r = engine.execute(granularity_query(sh, gname, zone), sh.ds)
        got = {int(t): int(c) for t, c in zip(r.data["timestamp"], r.data["c"]) if int(c)}
        _same_counts(got, counts(bucket_starts(sh.ms, gname, tz_ms)), f"{sh.ds.name} granularity {gname} {zone}")


def quarter_of_year_counts(sh, tz_ms, run):
    """T_QOY has no timeFormat pattern: a hand-built time key through the Lowerer.  ``run`` maps a
    ScanProgram to partials (ops.reference.run_reference or PreparedScan(prog).run())."""
    from spark_druid_olap_amd.engine.lower import KeyComp, Lowerer
    from spark_druid_olap_amd.engine.partials import finalize
    from spark_druid_olap_amd.ops import desc as D
    from spark_druid_olap_amd.query import spec as S

    kc = KeyComp("q", D.K_TIME, "__time", 4, base=1, tfield=T_QOY, tz_ms=tz_ms,
                 decoder=lambda ids: np.asarray(ids, dtype=np.int64) + 1)
    prog = Lowerer(sh.ds).lower_aggregate(INTERVAL, None, [], None, [S.FunctionAggregationSpec("count", "c")],
                                          extra_keys=[kc])
    out = finalize(prog, run(prog))
    got = {int(q): int(c) for q, c in zip(out["q"], out["c"]) if int(c)}
    want = counts((local(m, tz_ms).month - 1) // 3 + 1 for m in sh.ms.tolist())
    _same_counts(got, want, f"{sh.ds.name} quarter of year")



# ------------------------------------------------------------------- expression / filter checks
def _js_extreme(name, fields, expr, hi):
    from spark_druid_olap_amd.query import spec as S

    f, reset = ("Math.max", "-Infinity") if hi else ("Math.min", "Infinity")
    params = ", ".join(["current", "a", "b"][:1 + len(fields)])
    return S.JavascriptAggregationSpec(name, fields, f"function({params}) {{ return {f}(current, {expr}); }}",
                                       f"function(x, y) {{ return {f}(x, y); }}", f"function() {{ return {reset}; }}")


def _by_row(sh, aggs, filt=None):
    from spark_druid_olap_amd.query import spec as S

    return S.GroupByQuerySpec(sh.ds.name, [S.DefaultDimensionSpec("row")], aggregations=aggs, filter=filt,
                              intervals=INTERVAL)


def rows_of_expr(engine, sh, exprs):
    """{name: per-row f64 value} of javascript expressions {name: (fields, text over a, b)},
    five per query (each takes a Math.max and a Math.min aggregator)."""
    out, names = {}, list(exprs)
    for i in range(0, len(names), 5):
        aggs = []
        for k in names[i:i + 5]:
            fields, text = exprs[k]
            aggs += [_js_extreme(k + "_hi", fields, text, True), _js_extreme(k + "_lo", fields, text, False)]
        r = engine.execute(_by_row(sh, aggs), sh.ds)
        for k in names[i:i + 5]:
            out[k] = single_row_value(per_row(r, k + "_hi", sh.n), per_row(r, k + "_lo", sh.n), k)
    return out


def expression_cases(sh):
    """{name: ((fields, javascript), expected per row, ulp)}: every EOpCode over f64 and y, E_LUT
    through the numeric dimension, E_COL's decimal scale and E_CONST."""
    a, b = sh.cols["f64"], sh.cols["y"]
    cases = {}
    for op in EXACT_OPS + ULP_OPS:
        cases[op] = ((["f64", "y"], EXPR_JS[op].format(a="a", b="b")), expr_expected(op, a, b), 4 if op in ULP_OPS else 0)
    cases["lut"] = ((["f64", "dnum"], "a + b"), a + (sh.cols["dnum"] - 5.0), 0)
    cases["decimal"] = ((["dec"], "a * 3"), sh.cols["dec"].astype(np.float64) * 10.0 ** -2 * 3.0, 0)
    cases["const"] = ((["f64"], "0.5 - a"), 0.5 - a, 0)
    return cases


def check_expressions(engine, sh):
    cases = expression_cases(sh)
    got = rows_of_expr(engine, sh, {k: v[0] for k, v in cases.items()})
    a, b = sh.cols["f64"], sh.cols["y"]
    for k, (_, want, ulp) in cases.items():
        g = got[k]
        if k in ("min", "max"):  # fmin(-0.0, 0.0) may be either zero (IEEE 754-2008 minNum / maxNum)
            z = (a == 0) & (b == 0)
            g, want = np.where(z, np.abs(g), g), np.where(z, np.abs(want), want)
        assert_float_rows(g, want, ulp, f"expression {k}")


def count_by_row(engine, sh, filters):
    """{name: bool per row} of filters {name: FilterSpec}: each a filtered count in one query
    grouped by ``row`` (ten per query)."""
    from spark_druid_olap_amd.query import spec as S

    out, names = {}, list(filters)
    for i in range(0, len(names), 10):
        aggs = [S.FunctionAggregationSpec("count", "n")]
        aggs += [S.FilteredAggregationSpec(filters[k], S.FunctionAggregationSpec("count", k), k) for k in names[i:i + 10]]
        r = engine.execute(_by_row(sh, aggs), sh.ds)
        assert (per_row(r, "n", sh.n) == 1).all()
        for k in names[i:i + 10]:
            c = per_row(r, k, sh.n)
            assert set(np.unique(c).tolist()) <= {0, 1}, k
            out[k] = c.astype(bool)
    return out


def select_rows(engine, sh, filt):
    """bool per row: the rows a select query (the mask kernel) returns under the filter."""
    from spark_druid_olap_amd.query import spec as S

    q = S.SelectSpec(sh.ds.name, ["row"], [], filter=filt, pagingSpec=S.PagingSpec({}, sh.n + 1), intervals=INTERVAL)
    r = engine.execute(q, sh.ds)
    rows = np.asarray([int(x) for x in r.data["row"]], dtype=np.int64)
    assert len(set(rows.tolist())) == len(rows)
    m = np.zeros(sh.n, dtype=bool)
    m[rows] = True
    return m


def expression_filters(sh):
    """{name: (ExpressionFilterSpec, expected bool per row)}: ``op(f64, y) >= 1`` for every binary
    and unary operation (NaN fails), through F_EXPR."""
    from spark_druid_olap_amd.query import spec as S

    a, b = sh.cols["f64"], sh.cols["y"]
    out = {}
    for op in EXACT_OPS + ULP_OPS:
        v = expr_expected(op, a, b)
        with np.errstate(invalid="ignore"):
            d = v - 1.0
            want = d >= 0.0  # the lowering compares lhs - rhs with 0; NaN fails
        # a value within 4 ulp of the bound may fall on either side for log / exp / pow
        near = np.abs(d) < 1e-12 if op in ULP_OPS else np.zeros(len(v), dtype=bool)
        out[op] = (S.ExpressionFilterSpec(EXPR_JS[op].format(a="f64", b="y") + " >= 1"), want, near)
    return out


def check_expression_filters(engine, sh):
    fs = expression_filters(sh)
    got = count_by_row(engine, sh, {k: v[0] for k, v in fs.items()})
    for k, (_, want, near) in fs.items():
        bad = np.nonzero((got[k] != want) & ~near)[0]
        assert len(bad) == 0, f"expression filter {k}: rows {bad[:8]} (f64 {sh.cols['f64'][bad[:8]]}, y {sh.cols['y'][bad[:8]]})"


INT_TYPES = {"u8": (0, 255), "i16": (-2**15, 2**15 - 1), "i32": (-2**31, 2**31 - 1), "i64": (-2**62, 2**62)}


def range_filters(sh):
    """{name: (FilterSpec, expected bool per row from numpy)}."""
    from spark_druid_olap_amd.query import spec as S

    c, out = sh.cols, {}
    with np.errstate(invalid="ignore"):
        for col, lo, hi in (("f64", -1.5, 2.5), ("f32", float(np.float32(-0.1)), float(np.float32(0.1)))):
            v = c[col].astype(np.float64)
            assert (v == lo).any() and (v == hi).any()  # the bounds are stored values
            for ls in (False, True):
                for hs in (False, True):
                    want = (v > lo if ls else v >= lo) & (v < hi if hs else v <= hi)
                    out[f"{col}_{int(ls)}{int(hs)}"] = (S.BoundFilterSpec(col, lo, hi, ls, hs), want)
        for col, (lo, hi) in INT_TYPES.items():
            v = c[col].astype(np.int64)
            assert (v == lo).any() and (v == hi).any()
            out[f"{col}_min"] = (S.BoundFilterSpec(col, lo, lo), v == lo)
            out[f"{col}_max"] = (S.BoundFilterSpec(col, hi, hi), v == hi)
            out[f"{col}_all"] = (S.BoundFilterSpec(col, lo, hi), np.ones(sh.n, dtype=bool))
            out[f"{col}_in"] = (S.BoundFilterSpec(col, lo, hi, True, True), (v > lo) & (v < hi))
        # int64's own limits (the column stops at +-2^62 so that sums cannot wrap), non-strict and
        # strict, and bounds that a float would round
        v, lo, hi = c["i64"].astype(np.int64), -2**63, 2**63 - 1
        everything, nothing = np.ones(sh.n, dtype=bool), np.zeros(sh.n, dtype=bool)
        out["i64_limits"] = (S.BoundFilterSpec("i64", lo, hi), everything)
        out["i64_limits_strict"] = (S.BoundFilterSpec("i64", lo, hi, True, True), everything)
        out["i64_limits_text"] = (S.BoundFilterSpec("i64", str(lo), str(hi)), everything)
        out["i64_at_max"] = (S.BoundFilterSpec("i64", hi, hi), nothing)
        out["i64_at_min"] = (S.BoundFilterSpec("i64", lo, lo), nothing)
        out["i64_above_max"] = (S.BoundFilterSpec("i64", hi, None, True), nothing)
        out["i64_below_min"] = (S.BoundFilterSpec("i64", None, lo, False, True), nothing)
        out["i64_min_to_low"] = (S.BoundFilterSpec("i64", lo, -2**62), v == -2**62)
        out["i64_high_to_max"] = (S.BoundFilterSpec("i64", 2**62, hi), v == 2**62)
        out["i64_high_to_max_strict"] = (S.BoundFilterSpec("i64", 2**62, hi, True), nothing)
        out["i64_unrounded"] = (S.BoundFilterSpec("i64", 2**62 - 1, None, True), v == 2**62)  # float(2^62 - 1) == 2^62
        out["i64_equals"] = (S.SelectorFilterSpec("i64", 2**62), v == 2**62)
        out["i64_equals_max"] = (S.SelectorFilterSpec("i64", hi), nothing)
        out["dec_exact"] = (S.BoundFilterSpec("dec", "0.05", "0.25", True, False),
                            (c["dec"] > 5) & (c["dec"] <= 25))
        v = c["f64"]
        nan = np.isnan(v)
        assert nan.sum() >= 2
        rng = S.BoundFilterSpec("f64", float("-inf"), float("inf"))
        out["nan_range"] = (rng, ~nan)
        out["nan_not_range"] = (S.NotFilterSpec(rng), nan)
        out["nan_half"] = (S.BoundFilterSpec("f64", None, 0.0), v <= 0.0)
        out["nan_not_half"] = (S.NotFilterSpec(S.BoundFilterSpec("f64", None, 0.0)), ~(v <= 0.0))
        out["nan_expr"] = (S.ExpressionFilterSpec("f64 - f64 == 0"), np.isfinite(v))
        out["nan_expr_ne"] = (S.ExpressionFilterSpec("f64 != 1"), ~nan & (v != 1.0))
    some = [0, 1, 63, 64, 4095, 4096, 4159, 4160, sh.n - 1]
    out["in_row"] = (S.InFilterSpec("row", some), np.isin(c["row"], some))
    out["in_dnum"] = (S.InFilterSpec("dnum", [-5, 0, 3]), np.isin(c["dnum"] - 5, [-5, 0, 3]))
    return out


def check_range_filters(engine, sh, select=True):
    fs = range_filters(sh)
    got = count_by_row(engine, sh, {k: v[0] for k, v in fs.items()})
    for k, (f, want) in fs.items():
        assert (got[k] == want).all(), f"filter {k} as count by row: rows {np.nonzero(got[k] != want)[0][:8]}"
        if select:
            m = select_rows(engine, sh, f)
            assert (m == want).all(), f"filter {k} as select mask: rows {np.nonzero(m != want)[0][:8]}"


def padding_filters(sh):
    """{name: (FilterSpec or None, expected count over the first N rows)}: predicates a zero-filled
    padding row satisfies."""
    from spark_druid_olap_amd.query import spec as S

    c = sh.cols
    with np.errstate(invalid="ignore"):
        return {
            "all": (None, sh.n),
            "metric_zero": (S.SelectorFilterSpec("u8", 0), int((c["u8"] == 0).sum())),
            "float_zero": (S.SelectorFilterSpec("f64", 0), int((c["f64"] == 0).sum())),
            "dim_id0": (S.SelectorFilterSpec("grp", "g0"), int((c["grp"] == 0).sum())),
            "row_id0": (S.SelectorFilterSpec("row", 0), 1),
            "not_positive": (S.NotFilterSpec(S.BoundFilterSpec("f64", 0.0, None, True)), int((~(c["f64"] > 0)).sum())),
        }


def check_padding(sh, run):
    """``run`` maps a ScanProgram to partials."""
    from spark_druid_olap_amd.engine.lower import Lowerer
    from spark_druid_olap_amd.engine.partials import finalize
    from spark_druid_olap_amd.query import spec as S

    for k, (f, want) in padding_filters(sh).items():
        assert want > 0
        prog = Lowerer(sh.ds).lower_aggregate(INTERVAL, f, [], None, [S.FunctionAggregationSpec("count", "c")])
        got = finalize(prog, run(prog))["c"]
        assert [int(x) for x in got] == [want], (k, got, want)


def check_minmaxsum(engine, sh):
    from spark_druid_olap_amd.query import spec as S

    c, g = sh.cols, sh.cols["grp"]
    F = S.FunctionAggregationSpec

    def run(aggs):
        q = S.GroupByQuerySpec(sh.ds.name, [S.DefaultDimensionSpec("grp")], aggregations=aggs, intervals=INTERVAL)
        r = engine.execute(q, sh.ds)
        order = {v: i for i, v in enumerate(r.data["grp"])}
        assert sorted(order) == [f"g{i}" for i in range(7)]
        return lambda name, i: r.data[name][order[f"g{i}"]]

    for cols in (("u8", "i16", "i32"), ("i64", "dec")):
        at = run([F(f"long{op}", f"{col}_{op}", col) for col in cols for op in ("Min", "Max", "Sum")])
        for col in cols:
            sc = 100.0 if col == "dec" else 1
            for i in range(7):
                v = [int(x) for x in c[col][g == i]]
                assert at(f"{col}_Min", i) == min(v) / sc and at(f"{col}_Max", i) == max(v) / sc, (col, i)
                assert at(f"{col}_Sum", i) == sum(v) / sc, (col, i, at(f"{col}_Sum", i), sum(v))
    aggs, keep = [], {}
    for col in ("f64", "f32"):
        keep[col] = np.isfinite(c[col])
        flt = S.BoundFilterSpec(col, -3.5e38, 3.5e38) if col == "f32" else S.BoundFilterSpec(col, -1e301, 1e301)
        aggs += [S.FilteredAggregationSpec(flt, F(f"double{op}", f"{col}_{op}", col), f"{col}_{op}")
                 for op in ("Min", "Max", "Sum")]
    at = run(aggs)
    for col in ("f64", "f32"):
        for i in range(7):
            v = c[col][(g == i) & keep[col]].astype(np.float64)
            assert at(f"{col}_Min", i) == v.min() and at(f"{col}_Max", i) == v.max(), (col, i)
            np.testing.assert_allclose(at(f"{col}_Sum", i), math.fsum(v.tolist()), rtol=1e-9)


def check_exact_decimal_sum(engine, sh):
    """A_SUM_X: sum(dec * 1.07) per group is the exact integer sum(cents * 107) / 10^4."""
    from spark_druid_olap_amd.engine.lower import Lowerer
    from spark_druid_olap_amd.ops import desc as D
    from spark_druid_olap_amd.query import spec as S

    agg = S.JavascriptAggregationSpec("s", ["dec"], "function(current, a) { return current + a * 1.07; }",
                                      "function(x, y) { return x + y; }", "function() { return 0; }")
    dims = [S.DefaultDimensionSpec("grp")]
    prog = Lowerer(sh.ds).lower_aggregate(INTERVAL, None, dims, None, [agg])
    assert any(a["kind"] == D.A_SUM_X for a in prog.aops)
    r = engine.execute(S.GroupByQuerySpec(sh.ds.name, dims, aggregations=[agg], intervals=INTERVAL), sh.ds)
    for name, got in zip(r.data["grp"], r.data["s"]):
        cents = sh.cols["dec"][sh.cols["grp"] == int(name[1:])]
        assert got == sum(int(x) * 107 for x in cents) / 10.0 ** 4, (name, got)
    assert r.num_rows == 7
