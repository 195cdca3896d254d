"""Vectorised SQL expression evaluation and the scalar-function library.

The same evaluator runs (a) residual operators of a rewritten plan and plain (non-Druid) tables on
the host, and (b) *dictionary-domain* evaluation of pushed single-dimension expressions: a filter
``upper(s_name) = 'S1'`` or a grouping key ``substr(o_orderdate, 1, 7)`` is evaluated once over the
dimension's dictionary (C_d values) instead of once per row -- the MI355X replacement for the
reference's JavaScript filters/extractions (``sd/jscodegen/JSCodeGenerator.scala:76-451``,
``asd/ProjectFilterTransfom.scala:406-413``, ``asd/AggregateTransform.scala:85-94``).

Functions cover the Spark built-ins used by the reference's tests (string, math, date/time, cast,
conditional) and the sparkline ``spark-datetime`` UDFs (``dateTime``, ``period``, ``datePlus``,
``dateMinus``, ``dateIsBefore``..., Joda field accessors; ``sd/DateTimeExtractor.scala:157-189``).
"""
from __future__ import annotations

import math
import re
from typing import Any, Callable, Dict, List, Optional, Sequence

import numpy as np
import pandas as pd

from . import ast as A
from .types import (AnalysisError, INTEGRAL, base, broadcast, cast_vec, is_numeric, is_vec, pandas_dtype,
                    scalar_cast, to_series, wider)

# ------------------------------------------------------------------------------------------------
# registry
_FUNCS: Dict[str, "Fn"] = {}


class Fn:
    def __init__(self, name, ret, impl, nargs=None):
        self.name, self.ret, self.impl, self.nargs = name, ret, impl, nargs


def _reg(names, ret, nargs=None):
    def deco(impl):
        for n in names.split():
            _FUNCS[n.lower()] = Fn(n.lower(), ret, impl, nargs)
        return impl

    return deco


def has_function(name: str) -> bool:
    return name.lower() in _FUNCS or name.lower() in A.AGG_FUNCS


def _const(t):
    return lambda ts: t


def _first(ts):
    return ts[0] if ts else "null"


def _widest(ts):
    out = "null"
    for t in ts:
        out = wider(out, t)
    return out


# ------------------------------------------------------------------------------------------------
# typing
def quantile_args(call: A.Call):
    """(fractions, interpolate, array form) of a percentile / median / percentile_approx call.  The
    percentage is a literal in [0, 1], or -- ``percentile`` only -- ``array(...)`` of such literals;
    percentile_approx's accuracy argument is accepted and ignored."""
    n = call.name
    interp = n in ("percentile", "median")
    want = (1, 1) if n == "median" else ((2, 2) if n == "percentile" else (2, 3))
    if not (want[0] <= len(call.args) <= want[1]):
        raise AnalysisError(f"{n} takes {want[0]}" + (f"..{want[1]}" if want[1] != want[0] else "") + " arguments")
    if call.distinct:
        raise AnalysisError(f"{n}(DISTINCT) is not supported")
    if n == "median":
        return [0.5], True, False
    p = call.args[1]
    is_arr = isinstance(p, A.Call) and p.name == "array"
    if is_arr and not interp:
        raise AnalysisError(f"{n}: an array of percentages is supported by percentile only")
    lits = list(p.args) if is_arr else [p]
    out = []
    for x in lits:
        v = x.value if isinstance(x, A.Lit) else None
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (0.0 <= float(v) <= 1.0):
            raise AnalysisError(f"{n}: the percentage must be a literal between 0.0 and 1.0, got {x.sql()}")
        out.append(float(v))
    if not out:
        raise AnalysisError(f"{n}: empty percentage array")
    return out, interp, is_arr


def quantile_type(call: A.Call) -> str:
    _, interp, is_arr = quantile_args(call)
    t = typeof(call.args[0])
    if base(t) not in INTEGRAL and base(t) not in ("double", "float", "decimal"):
        raise AnalysisError(f"{call.name} over the non-numeric type {t}")
    return "array" if is_arr else ("double" if interp else t)


def comoment_type(call: A.Call) -> str:
    """corr / covar_samp / covar_pop: exactly two numeric arguments, no DISTINCT; a double."""
    n = call.name
    if call.distinct:
        raise AnalysisError(f"{n}(DISTINCT ...) is not supported")
    if len(call.args) != 2:
        raise AnalysisError(f"{n} takes exactly 2 arguments, got {len(call.args)}")
    for a in call.args:
        t = typeof(a)
        if base(t) not in INTEGRAL and base(t) not in ("double", "float", "decimal"):
            raise AnalysisError(f"{n} over the non-numeric type {t}")
    return "double"


def central_moment_type(call: A.Call) -> str:
    """skewness / kurtosis: exactly one numeric argument, no DISTINCT; a double."""
    n = call.name
    if call.distinct:
        raise AnalysisError(f"{n}(DISTINCT ...) is not supported")
    if len(call.args) != 1:
        raise AnalysisError(f"{n} takes exactly 1 argument, got {len(call.args)}")
    t = typeof(call.args[0])
    if base(t) not in INTEGRAL and base(t) not in ("double", "float", "decimal"):
        raise AnalysisError(f"{n} over the non-numeric type {t}")
    return "double"


def extreme_type(call: A.Call) -> str:
    """max_by / min_by (x, y): exactly two arguments, no DISTINCT; the type of x."""
    n = call.name
    if call.distinct:
        raise AnalysisError(f"{n}(DISTINCT ...) is not supported")
    if len(call.args) != 2:
        raise AnalysisError(f"{n} takes exactly 2 arguments, got {len(call.args)}")
    typeof(call.args[1])
    return typeof(call.args[0])


def histogram_args(call: A.Call) -> list:
    """The exact bucket edges (ops/buckets.py) of ``histogram(x, lo, hi, n)`` -- n equal buckets over
    [lo, hi) -- or ``histogram(x, array(b0, ..., bB))``: the limits are numeric literals, n a
    positive integer literal, lo < hi, the breaks at least two and strictly ascending."""
    from ..ops import buckets

    if call.distinct:
        raise AnalysisError("histogram(DISTINCT ...) is not supported")
    rest = call.args[1:]
    is_arr = len(rest) == 1 and isinstance(rest[0], A.Call) and rest[0].name == "array"
    if not is_arr and len(rest) != 3:
        raise AnalysisError("histogram takes (x, lo, hi, n) or (x, array(b0, ..., bB))")
    vals = []
    for x in (rest[0].args if is_arr else rest):
        v = x.value if isinstance(x, A.Lit) else None
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise AnalysisError(f"histogram: the limits must be numeric literals, got {x.sql()}")
        vals.append(v)
    try:
        return buckets.bucket_edges(breaks=vals) if is_arr else buckets.bucket_edges(*vals)
    except ValueError as e:
        raise AnalysisError(str(e)) from None


def histogram_type(call: A.Call) -> str:
    """histogram(x, ...): an array of B + 2 bigint counts [below, c_0 .. c_{B-1}, above]."""
    histogram_args(call)
    t = typeof(call.args[0])
    if base(t) not in INTEGRAL and base(t) not in ("double", "float", "decimal"):
        raise AnalysisError(f"histogram over the non-numeric type {t}")
    return "array"


def agg_type(name: str, ts: Sequence[str]) -> str:
    if name == "count" or name == "approx_count_distinct":
        return "bigint"
    if name == "sum":
        t = ts[0] if ts else "bigint"
        return "bigint" if base(t) in INTEGRAL else "double"
    if name in ("avg", "mean", "stddev", "stddev_samp", "stddev_pop", "variance", "var_samp", "var_pop"):
        return "double"
    if name in ("min", "max", "first", "last"):
        return ts[0]
    if name in ("grouping", "grouping_id"):
        return "int"
    if name in ("collect_set", "collect_list"):
        return "array"
    raise AnalysisError(f"unknown aggregate {name}")


def typeof(e: A.Expr) -> str:
    if isinstance(e, A.Lit):
        return e.dtype
    if isinstance(e, A.Ref):
        return e.dtype
    if isinstance(e, A.Alias):
        return typeof(e.child)
    if isinstance(e, A.BinOp):
        if e.op in ("and", "or", "=", "<>", "<", "<=", ">", ">=", "<=>"):
            return "boolean"
        lt, rt = typeof(e.l), typeof(e.r)
        if e.op == "/":
            return "double"
        if e.op == "div":
            return "bigint"
        if rt == "interval" and lt in ("date", "timestamp", "string"):
            return "timestamp" if lt != "date" else "date"
        if lt in ("date", "timestamp") and rt in ("date", "timestamp") and e.op == "-":
            return "int"
        t = wider(lt, rt)
        if base(t) == "string":
            return "double"
        return t
    if isinstance(e, A.UnOp):
        return "boolean" if e.op == "not" else typeof(e.child)
    if isinstance(e, A.Case):
        return _widest([typeof(v) for _, v in e.whens] + ([typeof(e.else_)] if e.else_ is not None else []))
    if isinstance(e, A.Cast):
        return e.to
    if isinstance(e, (A.InList, A.Like, A.IsNull)):
        return "boolean"
    if isinstance(e, A.IntervalLit):
        return "interval"
    if isinstance(e, A.SubqueryExpr):
        if e.kind == "scalar":
            return e.query.output[0].dtype
        return "boolean"
    if isinstance(e, A.WindowExpr):
        f = e.func
        if f.name in A.COMOMENT_FUNCS or f.name in A.EXTREME_FUNCS or f.name in A.HISTOGRAM_FUNCS or \
                f.name in A.CENTRAL_MOMENT_FUNCS:
            raise AnalysisError(f"{f.name} over a window is not supported")
        if f.name in ("rank", "dense_rank", "row_number", "ntile"):
            return "int"
        if f.name in ("percent_rank", "cume_dist"):
            return "double"
        if f.name in ("lag", "lead", "first_value", "last_value"):
            return typeof(f.args[0]) if f.args else "null"
        return typeof(f)
    if isinstance(e, A.Call):
        if e.name in A.QUANTILE_FUNCS:
            return quantile_type(e)
        if e.name in A.COMOMENT_FUNCS:
            return comoment_type(e)
        if e.name in A.CENTRAL_MOMENT_FUNCS:
            return central_moment_type(e)
        if e.name in A.EXTREME_FUNCS:
            return extreme_type(e)
        if e.name in A.HISTOGRAM_FUNCS:
            return histogram_type(e)
        ts = [typeof(a) for a in e.args]
        if e.is_agg:
            return agg_type(e.name, ts)
        f = _FUNCS.get(e.name)
        if f is None:
            raise AnalysisError(f"Undefined function: '{e.name}'")
        return f.ret(ts)
    raise AnalysisError(f"cannot type {e!r}")


# ------------------------------------------------------------------------------------------------
# evaluation
class Frame:
    """Columns by attribute id, all of length n."""

    def __init__(self, cols: Dict[int, pd.Series], n: int, subquery_eval: Optional[Callable] = None):
        self.cols = cols
        self.n = n
        self.subquery_eval = subquery_eval


def evaluate(e: A.Expr, fr: Frame):
    if isinstance(e, A.Lit):
        return e.value
    if isinstance(e, A.Ref):
        try:
            return fr.cols[e.rid]
        except KeyError:
            raise AnalysisError(f"unbound attribute {e.sql()}") from None
    if isinstance(e, A.Alias):
        return evaluate(e.child, fr)
    if isinstance(e, A.BinOp):
        return _binop(e, fr)
    if isinstance(e, A.UnOp):
        v = evaluate(e.child, fr)
        if e.op == "not":
            if is_vec(v):
                return ~v.astype("boolean")
            return None if v is None else (not v)
        if e.op == "-":
            return -v if v is not None else None
        if e.op == "~":
            return ~v if v is not None else None
    if isinstance(e, A.Cast):
        return cast_vec(evaluate(e.child, fr), typeof(e.child), e.to, fr.n)
    if isinstance(e, A.IsNull):
        v = evaluate(e.child, fr)
        if is_vec(v):
            r = v.isna()
            return (~r if e.negated else r).astype("boolean")
        r = v is None
        return (not r) if e.negated else r
    if isinstance(e, A.InList):
        return _in(e, fr)
    if isinstance(e, A.Like):
        return _like(e, fr)
    if isinstance(e, A.Case):
        return _case(e, fr)
    if isinstance(e, A.IntervalLit):
        return e
    if isinstance(e, A.SubqueryExpr):
        if fr.subquery_eval is None:
            raise AnalysisError("subquery evaluation not available here")
        return fr.subquery_eval(e, fr)
    if isinstance(e, A.Call):
        if e.is_agg:
            raise AnalysisError(f"aggregate {e.sql()} outside an aggregation")
        f = _FUNCS.get(e.name)
        if f is None:
            raise AnalysisError(f"Undefined function: '{e.name}'")
        args = [evaluate(a, fr) for a in e.args]
        ts = [typeof(a) for a in e.args]
        return f.impl(args, ts, fr.n)
    raise AnalysisError(f"cannot evaluate {e!r}")


def eval_series(e: A.Expr, fr: Frame) -> pd.Series:
    v = evaluate(e, fr)
    t = typeof(e)
    if is_vec(v):
        return v.reset_index(drop=True)
    if isinstance(v, A.IntervalLit):
        raise AnalysisError("interval is not a column value")
    return broadcast(v, fr.n, t)


def _num(v, t):
    """Arithmetic operand: strings are cast to double (Spark's implicit cast)."""
    if base(t) == "string":
        return cast_vec(v, "string", "double", 0)
    if base(t) == "boolean":
        return v
    return v


def _cmp_operands(l, r, lt, rt):
    """Coerce comparison operands to a common type."""
    t = wider(lt, rt)
    bt = base(t)
    if bt in ("date", "timestamp"):
        l = cast_vec(l, lt, "timestamp", 0) if base(lt) != bt or bt == "date" and base(lt) == "string" else l
        r = cast_vec(r, rt, "timestamp", 0) if base(rt) != bt or bt == "date" and base(rt) == "string" else r
        if not is_vec(l) and l is not None:
            l = pd.Timestamp(l)
        if not is_vec(r) and r is not None:
            r = pd.Timestamp(r)
    elif bt == "double" and (base(lt) == "string" or base(rt) == "string"):
        l = cast_vec(l, lt, "double", 0)
        r = cast_vec(r, rt, "double", 0)
    return l, r


def _binop(e: A.BinOp, fr: Frame):
    op = e.op
    if op in ("and", "or"):
        l = evaluate(e.l, fr)
        r = evaluate(e.r, fr)
        if not is_vec(l) and not is_vec(r):
            if op == "and":
                if l is False or r is False:
                    return False
                return None if l is None or r is None else True
            if l is True or r is True:
                return True
            return None if l is None or r is None else False
        lv = broadcast(l, fr.n, "boolean").astype("boolean")
        rv = broadcast(r, fr.n, "boolean").astype("boolean")
        return (lv & rv) if op == "and" else (lv | rv)
    l = evaluate(e.l, fr)
    r = evaluate(e.r, fr)
    lt, rt = typeof(e.l), typeof(e.r)
    if isinstance(r, A.IntervalLit) or isinstance(l, A.IntervalLit):
        if isinstance(l, A.IntervalLit):
            l, r, lt = r, l, rt
        return _add_interval(cast_vec(l, lt, "timestamp" if lt != "date" else "date", fr.n), r,
                             -1 if op == "-" else 1)
    if op in ("=", "<>", "<", "<=", ">", ">=", "<=>"):
        l, r = _cmp_operands(l, r, lt, rt)
        if op == "<=>":
            if not is_vec(l) and not is_vec(r):
                return l == r if (l is not None and r is not None) else (l is None and r is None)
            lv = broadcast(l, fr.n, lt)
            rv = broadcast(r, fr.n, rt)
            eq = (lv == rv).fillna(False).astype(bool)
            both = lv.isna().to_numpy() & rv.isna().to_numpy()
            return pd.Series(eq.to_numpy() | both, dtype="boolean")
        if not is_vec(l) and not is_vec(r):
            if l is None or r is None:
                return None
            return {"=": l == r, "<>": l != r, "<": l < r, "<=": l <= r, ">": l > r, ">=": l >= r}[op]
        if (not is_vec(l) and l is None) or (not is_vec(r) and r is None):
            return pd.Series([None] * fr.n, dtype="boolean")
        res = {"=": lambda: l == r, "<>": lambda: l != r, "<": lambda: l < r, "<=": lambda: l <= r,
               ">": lambda: l > r, ">=": lambda: l >= r}[op]()
        res = pd.Series(res).astype("boolean")
        # datetime NaT compares False instead of NULL
        for x in (l, r):
            if is_vec(x) and x.dtype.kind == "M":
                res = res.mask(x.isna().to_numpy(), pd.NA)
        return res
    if lt in ("date", "timestamp") and rt in ("date", "timestamp") and op == "-":
        return _datediff([l, r], [lt, rt], fr.n)
    l, r = _num(l, lt), _num(r, rt)
    if (not is_vec(l) and l is None) or (not is_vec(r) and r is None):
        return None
    if op == "+":
        return l + r
    if op == "-":
        return l - r
    if op == "*":
        return l * r
    if op == "/":
        if not is_vec(l) and not is_vec(r):
            return None if r == 0 else float(l) / float(r)
        lv = l.astype("Float64") if is_vec(l) else float(l)
        rv = r.astype("Float64") if is_vec(r) else float(r)
        if is_vec(rv):
            rv = rv.mask(rv == 0, pd.NA)
        elif rv == 0:
            return pd.Series([None] * fr.n, dtype="Float64")
        return lv / rv
    if op == "div":
        if not is_vec(l) and not is_vec(r):
            return None if r == 0 else int(l // r)
        rv = r.mask(r == 0, pd.NA) if is_vec(r) else (None if r == 0 else r)
        if rv is None:
            return pd.Series([None] * fr.n, dtype="Int64")
        return (l // rv).astype("Int64")
    if op == "%":
        if not is_vec(l) and not is_vec(r):
            return None if r == 0 else math.fmod(l, r) if isinstance(l, float) or isinstance(r, float) else int(math.fmod(l, r))
        lv, rv = broadcast(l, fr.n, lt), broadcast(r, fr.n, rt)
        rv = rv.mask(rv == 0, pd.NA)
        return pd.Series(np.fmod(lv.astype("Float64"), rv.astype("Float64"))).astype(pandas_dtype(typeof(e)))
    if op in ("&", "|", "^"):
        return {"&": lambda: l & r, "|": lambda: l | r, "^": lambda: l ^ r}[op]()
    raise AnalysisError(f"unsupported operator {op}")


def _in(e: A.InList, fr: Frame):
    v = evaluate(e.child, fr)
    ct = typeof(e.child)
    items = [evaluate(i, fr) for i in e.items]
    its = [typeof(i) for i in e.items]
    t = _widest([ct] + its)
    if not is_vec(v) and all(not is_vec(i) for i in items):
        if v is None:
            return None
        vv = scalar_cast(v, ct, t)
        vals = [scalar_cast(i, it, t) for i, it in zip(items, its)]
        hit = vv in [x for x in vals if x is not None]
        if hit:
            return not e.negated
        if any(x is None for x in vals):
            return None
        return e.negated
    vs = broadcast(v, fr.n, ct)
    vs = cast_vec(vs, ct, t, fr.n)
    if all(not is_vec(i) for i in items):
        vals = [scalar_cast(i, it, t) for i, it in zip(items, its)]
        has_null = any(x is None for x in vals)
        res = vs.isin([x for x in vals if x is not None]).astype("boolean")
    else:
        res = pd.Series([False] * fr.n, dtype="boolean")
        has_null = False
        for i, it in zip(items, its):
            iv = cast_vec(broadcast(i, fr.n, it), it, t, fr.n)
            res = res | (vs == iv).fillna(False).astype("boolean")
    res = res.mask(vs.isna().to_numpy(), pd.NA)
    if has_null:
        res = res.mask(~res.fillna(False).to_numpy(dtype=bool), pd.NA)
    return ~res if e.negated else res


def like_to_regex(p: str) -> str:
    out = []
    i = 0
    while i < len(p):
        c = p[i]
        if c == "\\" and i + 1 < len(p):
            out.append(re.escape(p[i + 1]))
            i += 2
            continue
        out.append(".*" if c == "%" else "." if c == "_" else re.escape(c))
        i += 1
    return "^" + "".join(out) + "$"


def _like(e: A.Like, fr: Frame):
    v = evaluate(e.child, fr)
    p = evaluate(e.pattern, fr)
    if is_vec(p):
        raise AnalysisError("non-constant LIKE pattern")
    if p is None:
        return None
    rx = like_to_regex(p) if e.kind == "like" else p
    if not is_vec(v):
        if v is None:
            return None
        m = (re.match(rx, str(v), re.S) is not None) if e.kind == "like" else (re.search(rx, str(v)) is not None)
        return (not m) if e.negated else m
    s = cast_vec(v, typeof(e.child), "string", fr.n)
    res = s.str.match(rx, flags=re.S) if e.kind == "like" else s.str.contains(rx, regex=True)
    res = res.astype("boolean")
    return ~res if e.negated else res


def _case(e: A.Case, fr: Frame):
    t = typeof(e)
    conds = [evaluate(c, fr) for c, _ in e.whens]
    vals = [evaluate(v, fr) for _, v in e.whens]
    els = evaluate(e.else_, fr) if e.else_ is not None else None
    if all(not is_vec(x) for x in conds + vals + [els]):
        for c, v, (_, ve) in zip(conds, vals, e.whens):
            if c:
                return scalar_cast(v, typeof(ve), t)
        return scalar_cast(els, typeof(e.else_), t) if e.else_ is not None else None
    n = fr.n
    out = cast_vec(broadcast(els, n, t), typeof(e.else_) if e.else_ is not None else t, t, n).copy()
    decided = np.zeros(n, dtype=bool)
    for c, v, (_, ve) in zip(conds, vals, e.whens):
        cm = broadcast(c, n, "boolean").fillna(False).to_numpy(dtype=bool) & ~decided
        if cm.any():
            vv = cast_vec(broadcast(v, n, typeof(ve)), typeof(ve), t, n)
            out = out.mask(cm, vv)
        decided |= cm
    return out


# ------------------------------------------------------------------------------------------------
# helpers for function impls
def _vec_or_scalar(fn_scalar, fn_vec):
    def impl(args, ts, n):
        if not any(is_vec(a) for a in args):
            if any(a is None for a in args):
                return None
            return fn_scalar(*args)
        return fn_vec(args, ts, n)

    return impl


def _ts(v, t, n=0):
    """Any date-ish value -> timestamp (Series or pd.Timestamp)."""
    bt = base(t)
    if bt in ("date", "timestamp"):
        return pd.Timestamp(v) if (not is_vec(v) and v is not None) else v
    return cast_vec(v, t, "timestamp", n)


def _str(v, t, n=0):
    if base(t) == "string":
        if is_vec(v) and isinstance(v.dtype, pd.CategoricalDtype):
            return v.astype("string")
        return v
    return cast_vec(v, t, "string", n)


def _map_scalar(fn, rtype):
    """Lift a scalar python function over Series (element-wise, NULL-propagating)."""
    def impl(args, ts, n):
        if not any(is_vec(a) for a in args):
            if any(a is None for a in args):
                return None
            return fn(*args)
        cols = [a if is_vec(a) else [a] * n for a in args]
        out = []
        for vals in zip(*cols):
            if any(v is None or v is pd.NA or v is pd.NaT or (isinstance(v, float) and v != v) for v in vals):
                out.append(None)
            else:
                out.append(fn(*[v.item() if isinstance(v, np.generic) else v for v in vals]))
        return to_series(pd.Series(out, dtype=object), rtype)

    return impl


# ------------------------------------------------------------------------------------------------
# string functions
@_reg("concat", _const("string"))
def _concat(args, ts, n):
    args = [_str(a, t, n) for a, t in zip(args, ts)]
    if not any(is_vec(a) for a in args):
        return None if any(a is None for a in args) else "".join(args)
    out = None
    for a in args:
        s = broadcast(a, n, "string")
        out = s if out is None else out + s
    return out


@_reg("concat_ws", _const("string"))
def _concat_ws(args, ts, n):
    sep = args[0]
    rest = [_str(a, t, n) for a, t in zip(args[1:], ts[1:])]
    if not any(is_vec(a) for a in rest):
        return sep.join(a for a in rest if a is not None)
    out = None
    for a in rest:
        s = broadcast(a, n, "string")
        out = s.fillna("") if out is None else out + sep + s.fillna("")
    return out


def _substr_s(s, pos, ln=None):
    s = str(s)
    pos = int(pos)
    start = pos - 1 if pos > 0 else (len(s) + pos if pos < 0 else 0)
    start = max(start, 0)
    if ln is None:
        return s[start:]
    return s[start:start + max(int(ln), 0)]


@_reg("substr substring", _const("string"))
def _substr(args, ts, n):
    s = _str(args[0], ts[0], n)
    rest = args[1:]
    if not is_vec(s):
        if s is None or any(a is None for a in rest):
            return None
        return _substr_s(s, *rest)
    if all(not is_vec(a) for a in rest):
        pos = int(rest[0])
        ln = int(rest[1]) if len(rest) > 1 else None
        if pos > 0:
            return s.str.slice(pos - 1, None if ln is None else pos - 1 + max(ln, 0))
    return _map_scalar(_substr_s, "string")([s] + list(rest), ["string"] + ts[1:], n)


def _str_method(name, rtype="string"):
    def impl(args, ts, n):
        s = _str(args[0], ts[0], n)
        if not is_vec(s):
            return None if s is None else getattr(str(s), name)()
        r = getattr(s.str, name)()
        return r

    return impl


_reg("upper ucase", _const("string"))(_str_method("upper"))
_reg("lower lcase", _const("string"))(_str_method("lower"))
_reg("trim", _const("string"))(_str_method("strip"))
_reg("ltrim", _const("string"))(_str_method("lstrip"))
_reg("rtrim", _const("string"))(_str_method("rstrip"))


@_reg("length char_length character_length", _const("int"))
def _length(args, ts, n):
    s = _str(args[0], ts[0], n)
    if not is_vec(s):
        return None if s is None else len(s)
    return s.str.len().astype("Int64")


@_reg("reverse", _const("string"))
def _reverse(args, ts, n):
    s = _str(args[0], ts[0], n)
    if not is_vec(s):
        return None if s is None else s[::-1]
    return s.str[::-1]


@_reg("initcap", _const("string"))
def _initcap(args, ts, n):
    return _map_scalar(lambda s: " ".join(w[:1].upper() + w[1:].lower() for w in str(s).split(" ")), "string")(
        [_str(args[0], ts[0], n)], ["string"], n)


@_reg("lpad", _const("string"))
def _lpad(args, ts, n):
    def f(s, ln, pad=" "):
        s, ln = str(s), int(ln)
        if len(s) >= ln:
            return s[:ln]
        fill = (pad * ln)[: ln - len(s)] if pad else ""
        return fill + s
    return _map_scalar(f, "string")([_str(args[0], ts[0], n)] + args[1:], ["string"] + ts[1:], n)


@_reg("rpad", _const("string"))
def _rpad(args, ts, n):
    def f(s, ln, pad=" "):
        s, ln = str(s), int(ln)
        if len(s) >= ln:
            return s[:ln]
        return s + ((pad * ln)[: ln - len(s)] if pad else "")
    return _map_scalar(f, "string")([_str(args[0], ts[0], n)] + args[1:], ["string"] + ts[1:], n)


@_reg("instr", _const("int"))
def _instr(args, ts, n):
    return _map_scalar(lambda s, sub: str(s).find(str(sub)) + 1, "int")([_str(args[0], ts[0], n), args[1]],
                                                                         ["string", "string"], n)


@_reg("locate", _const("int"))
def _locate(args, ts, n):
    def f(sub, s, pos=1):
        return str(s).find(str(sub), max(int(pos) - 1, 0)) + 1
    return _map_scalar(f, "int")([args[0], _str(args[1], ts[1], n)] + args[2:], ["string", "string"] + ts[2:], n)


@_reg("regexp_extract", _const("string"))
def _regexp_extract(args, ts, n):
    def f(s, p, idx=1):
        m = re.search(p, str(s))
        if not m:
            return ""
        return m.group(int(idx)) or ""
    return _map_scalar(f, "string")([_str(args[0], ts[0], n)] + args[1:], ["string"] + ts[1:], n)


@_reg("regexp_replace", _const("string"))
def _regexp_replace(args, ts, n):
    s = _str(args[0], ts[0], n)
    if is_vec(s) and not is_vec(args[1]) and not is_vec(args[2]):
        return s.str.replace(args[1], _java_repl(args[2]), regex=True)
    return _map_scalar(lambda s, p, r: re.sub(p, _java_repl(r), str(s)), "string")([s, args[1], args[2]],
                                                                                    ["string"] * 3, n)


def _java_repl(r: str) -> str:
    return re.sub(r"\$(\d)", r"\\\1", r)


@_reg("replace", _const("string"))
def _replace(args, ts, n):
    s = _str(args[0], ts[0], n)
    rep = args[2] if len(args) > 2 else ""
    if is_vec(s) and not is_vec(args[1]):
        return s.str.replace(args[1], rep, regex=False)
    return _map_scalar(lambda s, a, b="": str(s).replace(a, b), "string")([s, args[1], rep], ["string"] * 3, n)


@_reg("split", _const("array"))
def _split(args, ts, n):
    return _map_scalar(lambda s, p: re.split(p, str(s)), "object")([_str(args[0], ts[0], n), args[1]],
                                                                    ["string", "string"], n)


@_reg("repeat", _const("string"))
def _repeat(args, ts, n):
    return _map_scalar(lambda s, k: str(s) * int(k), "string")([_str(args[0], ts[0], n), args[1]], ts, n)


@_reg("ascii", _const("int"))
def _ascii(args, ts, n):
    return _map_scalar(lambda s: ord(s[0]) if s else 0, "int")([_str(args[0], ts[0], n)], ts, n)


# ------------------------------------------------------------------------------------------------
# math
def _unary_math(f_np, rtype="double"):
    def impl(args, ts, n):
        v = args[0]
        if base(ts[0]) == "string":
            v = cast_vec(v, "string", "double", n)
        if not is_vec(v):
            if v is None:
                return None
            try:
                r = float(f_np(np.float64(v)))
            except (ValueError, OverflowError):
                return None
            return None if math.isnan(r) else (int(r) if rtype == "bigint" else r)
        arr = v.astype("Float64").to_numpy(dtype="float64", na_value=np.nan)
        with np.errstate(all="ignore"):
            r = f_np(arr)
        s = pd.Series(r, dtype="Float64")
        s = s.mask(np.isnan(r), pd.NA)
        return _float_to_int_series(s) if rtype == "bigint" else s

    return impl


def _float_to_int_series(s):
    from .types import _float_to_int

    return _float_to_int(s.to_numpy(dtype="float64", na_value=np.nan))


for _nm, _f in [("sin", np.sin), ("cos", np.cos), ("tan", np.tan), ("asin", np.arcsin), ("acos", np.arccos),
                ("atan", np.arctan), ("sinh", np.sinh), ("cosh", np.cosh), ("tanh", np.tanh), ("sqrt", np.sqrt),
                ("exp", np.exp), ("ln", np.log), ("log10", np.log10), ("log2", np.log2), ("cbrt", np.cbrt),
                ("degrees", np.degrees), ("radians", np.radians), ("signum sign", np.sign),
                ("expm1", np.expm1), ("log1p", np.log1p), ("rint", np.rint)]:
    _reg(_nm, _const("double"))(_unary_math(_f))

_reg("floor", _const("bigint"))(_unary_math(np.floor, "bigint"))
_reg("ceil ceiling", _const("bigint"))(_unary_math(np.ceil, "bigint"))


@_reg("log", _const("double"))
def _log(args, ts, n):
    if len(args) == 1:
        return _unary_math(np.log)(args, ts, n)
    b = args[0]
    return _binary_math(lambda base_, x: np.log(x) / np.log(base_))([b, args[1]], ts, n)


def _binary_math(f):
    def impl(args, ts, n):
        a, b = [cast_vec(x, t, "double", n) if base(t) == "string" else x for x, t in zip(args, ts)]
        if not is_vec(a) and not is_vec(b):
            if a is None or b is None:
                return None
            with np.errstate(all="ignore"):
                r = float(f(np.float64(a), np.float64(b)))
            return None if math.isnan(r) else r
        av = broadcast(a, n, "double").astype("Float64").to_numpy(dtype="float64", na_value=np.nan)
        bv = broadcast(b, n, "double").astype("Float64").to_numpy(dtype="float64", na_value=np.nan)
        with np.errstate(all="ignore"):
            r = f(av, bv)
        s = pd.Series(r, dtype="Float64")
        return s.mask(np.isnan(r), pd.NA)

    return impl


_reg("pow power", _const("double"))(_binary_math(np.power))
_reg("atan2", _const("double"))(_binary_math(np.arctan2))
_reg("hypot", _const("double"))(_binary_math(np.hypot))


@_reg("abs", _first)
def _abs(args, ts, n):
    v = args[0]
    if not is_vec(v):
        return None if v is None else abs(v)
    return v.abs()


@_reg("negative", _first)
def _negative(args, ts, n):
    return None if (not is_vec(args[0]) and args[0] is None) else -args[0]


@_reg("positive", _first)
def _positive(args, ts, n):
    return args[0]


@_reg("pmod", lambda ts: wider(ts[0], ts[1]))
def _pmod(args, ts, n):
    a, b = args
    rt = wider(ts[0], ts[1])
    # Spark's Pmod: r = a % n with Java (truncated, sign-of-dividend) remainder; r < 0 -> (r + n) % n.
    # A negative divisor therefore keeps non-negative remainders: pmod(7, -5) = 2.
    if not is_vec(a) and not is_vec(b):
        if a is None or b is None or b == 0:
            return None
        if isinstance(a, int) and isinstance(b, int):
            r = int(np.fmod(a, b))
            return int(np.fmod(r + b, b)) if r < 0 else r
        r = math.fmod(a, b)
        return math.fmod(r + b, b) if r < 0 else r
    av = broadcast(a, n, ts[0])
    bv = broadcast(b, n, ts[1])
    bad = (bv.isna() | (bv == 0)).to_numpy(dtype=bool, na_value=True) | av.isna().to_numpy(dtype=bool)
    if base(rt) in INTEGRAL:
        x = av.astype("Int64").to_numpy(dtype=np.int64, na_value=0)
        y = bv.astype("Int64").to_numpy(dtype=np.int64, na_value=1)
        y = np.where(y == 0, 1, y)
    else:
        x = av.astype("Float64").to_numpy(dtype=np.float64, na_value=0.0)
        y = bv.astype("Float64").to_numpy(dtype=np.float64, na_value=1.0)
        y = np.where(y == 0, 1.0, y)
    r = np.fmod(x, y)
    r = np.where(r < 0, np.fmod(r + y, y), r)
    out = pd.Series(r).astype(pandas_dtype(rt))
    return out.mask(bad, pd.NA)


@_reg("round bround", lambda ts: ts[0] if base(ts[0]) in INTEGRAL else "double")
def _round(args, ts, n):
    v = args[0]
    d = int(args[1]) if len(args) > 1 and args[1] is not None else 0
    if base(ts[0]) == "string":
        v = cast_vec(v, "string", "double", n)
    if not is_vec(v):
        if v is None:
            return None
        return _half_up(float(v), d) if base(ts[0]) not in INTEGRAL else int(_half_up(float(v), d))
    if base(ts[0]) in INTEGRAL:
        if d >= 0:
            return v
        arr = v.astype("Float64").to_numpy(dtype="float64", na_value=np.nan)
        return _float_to_int_series(pd.Series(_half_up_np(arr, d), dtype="Float64"))
    arr = v.astype("Float64").to_numpy(dtype="float64", na_value=np.nan)
    r = _half_up_np(arr, d)
    return pd.Series(r, dtype="Float64").mask(np.isnan(r), pd.NA)


def _half_up(x: float, d: int) -> float:
    from decimal import ROUND_HALF_UP, Decimal

    if math.isnan(x) or math.isinf(x):
        return x
    q = Decimal(1).scaleb(-d)
    return float(Decimal(repr(x)).quantize(q, rounding=ROUND_HALF_UP))


def _half_up_np(arr, d):
    """ROUND(x, d) half away from zero (the magnitude rounded, the sign copied back)."""
    a = np.abs(np.asarray(arr, dtype=np.float64))
    if d:
        m = 10.0 ** d
        a *= m
    a += 0.5
    a += 1e-9
    np.floor(a, out=a)
    if d:
        a /= m
    return np.copysign(a, arr)


@_reg("rand random", _const("double"))
def _rand(args, ts, n):
    rng = np.random.default_rng(int(args[0]) if args else None)
    return pd.Series(rng.random(max(n, 1))[:n], dtype="Float64") if n else float(rng.random())


@_reg("greatest", _widest)
def _greatest(args, ts, n):
    return _extreme(args, ts, n, True)


@_reg("least", _widest)
def _least(args, ts, n):
    return _extreme(args, ts, n, False)


def _extreme(args, ts, n, hi):
    t = _widest(ts)
    vals = [cast_vec(a, at, t, n) for a, at in zip(args, ts)]
    if not any(is_vec(v) for v in vals):
        vs = [v for v in vals if v is not None]
        return (max(vs) if hi else min(vs)) if vs else None
    df = pd.concat([broadcast(v, n, t).reset_index(drop=True) for v in vals], axis=1)
    r = df.max(axis=1, skipna=True) if hi else df.min(axis=1, skipna=True)
    return to_series(r, t)


# ------------------------------------------------------------------------------------------------
# conditional / null handling
@_reg("coalesce nvl ifnull", _widest)
def _coalesce(args, ts, n):
    t = _widest(ts)
    vals = [cast_vec(a, at, t, n) for a, at in zip(args, ts)]
    if not any(is_vec(v) for v in vals):
        for v in vals:
            if v is not None:
                return v
        return None
    out = None
    for v in vals:
        if out is None:
            out = broadcast(v, n, t).copy()
        else:
            miss = out.isna().to_numpy()
            if not miss.any():
                break
            out = out.mask(miss, broadcast(v, n, t))
    return out


@_reg("nullif", _first)
def _nullif(args, ts, n):
    a, b = args
    if not is_vec(a) and not is_vec(b):
        return None if a == b else a
    av = broadcast(a, n, ts[0])
    eq = (av == b).fillna(False).to_numpy(dtype=bool)
    return av.mask(eq, pd.NA if av.dtype.kind != "M" else pd.NaT)


@_reg("if", lambda ts: wider(ts[1], ts[2]))
def _if(args, ts, n):
    c, a, b = args
    t = wider(ts[1], ts[2])
    if not any(is_vec(x) for x in args):
        return scalar_cast(a, ts[1], t) if c else scalar_cast(b, ts[2], t)
    cm = broadcast(c, n, "boolean").fillna(False).to_numpy(dtype=bool)
    out = cast_vec(broadcast(b, n, ts[2]), ts[2], t, n)
    return out.mask(cm, cast_vec(broadcast(a, n, ts[1]), ts[1], t, n))


@_reg("isnull", _const("boolean"))
def _isnull(args, ts, n):
    v = args[0]
    return v.isna().astype("boolean") if is_vec(v) else v is None


@_reg("isnotnull", _const("boolean"))
def _isnotnull(args, ts, n):
    v = args[0]
    return (~v.isna()).astype("boolean") if is_vec(v) else v is not None


@_reg("nanvl", _widest)
def _nanvl(args, ts, n):
    a, b = args
    if not is_vec(a):
        return b if (a is not None and isinstance(a, float) and math.isnan(a)) else a
    return a


@_reg("hash", _const("int"))
def _hash(args, ts, n):
    import zlib

    return _map_scalar(lambda *vs: zlib.crc32("|".join(map(str, vs)).encode()) - 2 ** 31, "int")(args, ts, n)


# ------------------------------------------------------------------------------------------------
# date / time (Spark built-ins)
def _date_part(fn_vec, fn_scalar, rtype="int"):
    def impl(args, ts, n):
        v = _ts(args[0], ts[0], n)
        if not is_vec(v):
            if v is None or v is pd.NaT:
                return None
            return fn_scalar(pd.Timestamp(v))
        r = fn_vec(v.dt)
        return pd.Series(r).astype("Int64") if rtype == "int" else r

    return impl


_reg("year", _const("int"))(_date_part(lambda d: d.year, lambda t: t.year))
_reg("month", _const("int"))(_date_part(lambda d: d.month, lambda t: t.month))
_reg("day dayofmonth", _const("int"))(_date_part(lambda d: d.day, lambda t: t.day))
_reg("dayofyear", _const("int"))(_date_part(lambda d: d.dayofyear, lambda t: t.dayofyear))
_reg("hour", _const("int"))(_date_part(lambda d: d.hour, lambda t: t.hour))
_reg("minute", _const("int"))(_date_part(lambda d: d.minute, lambda t: t.minute))
_reg("second", _const("int"))(_date_part(lambda d: d.second, lambda t: t.second))
_reg("quarter", _const("int"))(_date_part(lambda d: d.quarter, lambda t: t.quarter))
_reg("weekofyear", _const("int"))(_date_part(lambda d: d.isocalendar().week,
                                             lambda t: t.isocalendar()[1]))
_reg("dayofweek", _const("int"))(_date_part(lambda d: (d.dayofweek + 1) % 7 + 1,
                                            lambda t: (t.dayofweek + 1) % 7 + 1))


@_reg("to_date", _const("date"))
def _to_date(args, ts, n):
    v = args[0]
    if len(args) > 1 and args[1] is not None:
        return _unix_parse([v, args[1]], ts, n, out="date")
    return cast_vec(v, ts[0], "date", n) if base(ts[0]) != "date" else v


@_reg("to_timestamp", _const("timestamp"))
def _to_timestamp(args, ts, n):
    if len(args) > 1:
        return _unix_parse(args, ts, n, out="timestamp")
    return cast_vec(args[0], ts[0], "timestamp", n)


@_reg("current_date", _const("date"))
def _current_date(args, ts, n):
    return pd.Timestamp.utcnow().tz_localize(None).normalize()


@_reg("current_timestamp now", _const("timestamp"))
def _current_ts(args, ts, n):
    return pd.Timestamp.utcnow().tz_localize(None)


def _add_days(d, k, sign=1):
    if not is_vec(d) and not is_vec(k):
        if d is None or k is None:
            return None
        return (pd.Timestamp(d) + pd.Timedelta(days=sign * int(k))).normalize()
    if is_vec(k):
        kd = pd.to_timedelta(k.astype("Float64").to_numpy(dtype="float64", na_value=np.nan) * sign, unit="D")
        return (d + kd).dt.normalize() if is_vec(d) else (pd.Timestamp(d) + pd.Series(kd)).dt.normalize()
    return (d + pd.Timedelta(days=sign * int(k))).dt.normalize()


@_reg("date_add", _const("date"))
def _date_add(args, ts, n):
    return _add_days(cast_vec(args[0], ts[0], "date", n), args[1], 1)


@_reg("date_sub", _const("date"))
def _date_sub(args, ts, n):
    return _add_days(cast_vec(args[0], ts[0], "date", n), args[1], -1)


@_reg("datediff", _const("int"))
def _datediff(args, ts, n):
    a = cast_vec(args[0], ts[0], "date", n)
    b = cast_vec(args[1], ts[1], "date", n)
    if not is_vec(a) and not is_vec(b):
        if a is None or b is None:
            return None
        return int((pd.Timestamp(a) - pd.Timestamp(b)).days)
    r = (a - b)
    if is_vec(r):
        return pd.Series(r.dt.days).astype("Int64")
    return r


@_reg("add_months", _const("date"))
def _add_months(args, ts, n):
    d = cast_vec(args[0], ts[0], "date", n)
    k = args[1]
    if not is_vec(d) and not is_vec(k):
        if d is None or k is None:
            return None
        return _shift_months(pd.Timestamp(d), int(k))
    if not is_vec(k):
        return d + pd.DateOffset(months=int(k))
    return _map_scalar(lambda dd, kk: _shift_months(pd.Timestamp(dd), int(kk)), "date")([d, k], ["date", "int"], n)


def _shift_months(t: pd.Timestamp, k: int) -> pd.Timestamp:
    return (t + pd.DateOffset(months=k)).normalize()


@_reg("months_between", _const("double"))
def _months_between(args, ts, n):
    def f(a, b):
        a, b = pd.Timestamp(a), pd.Timestamp(b)
        return round((a.year - b.year) * 12 + (a.month - b.month) + (a.day - b.day) / 31.0, 8)
    return _map_scalar(f, "double")([_ts(args[0], ts[0], n), _ts(args[1], ts[1], n)], ["timestamp"] * 2, n)


@_reg("last_day", _const("date"))
def _last_day(args, ts, n):
    d = cast_vec(args[0], ts[0], "date", n)
    if not is_vec(d):
        return None if d is None else (pd.Timestamp(d) + pd.offsets.MonthEnd(0)).normalize()
    return d + pd.offsets.MonthEnd(0)


@_reg("next_day", _const("date"))
def _next_day(args, ts, n):
    days = {"MO": 0, "TU": 1, "WE": 2, "TH": 3, "FR": 4, "SA": 5, "SU": 6}

    def f(d, dow):
        t = pd.Timestamp(d)
        w = days.get(str(dow)[:2].upper())
        if w is None:
            return None
        delta = (w - t.dayofweek - 1) % 7 + 1
        return (t + pd.Timedelta(days=delta)).normalize()
    return _map_scalar(f, "date")([cast_vec(args[0], ts[0], "date", n), args[1]], ["date", "string"], n)


@_reg("trunc", _const("date"))
def _trunc(args, ts, n):
    def f(d, fmt):
        t = pd.Timestamp(d)
        f_ = str(fmt).upper()
        if f_ in ("YEAR", "YYYY", "YY"):
            return pd.Timestamp(t.year, 1, 1)
        if f_ in ("MONTH", "MON", "MM"):
            return pd.Timestamp(t.year, t.month, 1)
        return None
    return _map_scalar(f, "date")([cast_vec(args[0], ts[0], "date", n), args[1]], ["date", "string"], n)


@_reg("date_format", _const("string"))
def _date_format(args, ts, n):
    from ..query import joda

    v = _ts(args[0], ts[0], n)
    fmt = args[1]

    def f(t):
        return joda.format_ms(fmt, int(pd.Timestamp(t).value // 10 ** 6))
    if not is_vec(v):
        return None if v is None or v is pd.NaT else f(v)
    ms = v.astype("int64", errors="ignore")
    out = [None if x is pd.NaT else f(x) for x in v]
    _ = ms
    return pd.Series(out, dtype="string")


def _unix_parse(args, ts, n, out="seconds"):
    from ..query import joda

    v = args[0]
    fmt = args[1] if len(args) > 1 else "yyyy-MM-dd HH:mm:ss"

    def f(s):
        if isinstance(s, pd.Timestamp):
            ms = int(s.value // 10 ** 6)
        else:
            ms = joda.parse(fmt, str(s))
        if ms is None:
            return None
        if out == "seconds":
            return ms // 1000
        t = pd.Timestamp(ms * 10 ** 6)
        return t.normalize() if out == "date" else t
    rtype = {"seconds": "bigint", "date": "date", "timestamp": "timestamp"}[out]
    if base(ts[0]) in ("date", "timestamp"):
        return _map_scalar(lambda t: f(pd.Timestamp(t)), rtype)([v], ts[:1], n)
    if is_vec(v) and len(v) > 64:
        # evaluate per distinct value (dictionary-style)
        codes, uniq = pd.factorize(v)
        vals = [f(u) for u in uniq]
        res = pd.Series(vals, dtype=object).reindex(codes).reset_index(drop=True)
        res[codes < 0] = None
        return to_series(res, rtype)
    return _map_scalar(f, rtype)([v], ["string"], n)


@_reg("unix_timestamp", _const("bigint"))
def _unix_timestamp(args, ts, n):
    if not args:
        return int(pd.Timestamp.utcnow().value // 10 ** 9)
    return _unix_parse(args, ts, n, "seconds")


@_reg("from_unixtime", _const("string"))
def _from_unixtime(args, ts, n):
    from ..query import joda

    fmt = args[1] if len(args) > 1 else "yyyy-MM-dd HH:mm:ss"
    return _map_scalar(lambda s: joda.format_ms(fmt, int(s) * 1000), "string")([args[0]], ts[:1], n)


@_reg("from_utc_timestamp to_utc_timestamp", _const("timestamp"))
def _tz_shift(args, ts, n):
    from ..query.intervals import tz_offset_ms

    v = _ts(args[0], ts[0], n)
    off = tz_offset_ms(args[1]) if args[1] is not None else 0
    return v + pd.Timedelta(milliseconds=off)


# ------------------------------------------------------------------------------------------------
# sparkline spark-datetime UDFs
class Period:
    """ISO-8601 period (``P90D``, ``P1Y``, ``PT1H``) as Joda ``Period`` fields."""

    _RX = re.compile(r"^P(?:(-?\d+)Y)?(?:(-?\d+)M)?(?:(-?\d+)W)?(?:(-?\d+)D)?"
                     r"(?:T(?:(-?\d+)H)?(?:(-?\d+)M)?(?:(-?\d+(?:\.\d+)?)S)?)?$")

    def __init__(self, s: str):
        m = self._RX.match(s.strip().upper())
        if not m:
            raise AnalysisError(f"bad period {s!r}")
        y, mo, w, d, h, mi, sec = m.groups()
        self.years, self.months, self.weeks, self.days = (int(x or 0) for x in (y, mo, w, d))
        self.hours, self.minutes = int(h or 0), int(mi or 0)
        self.seconds = float(sec or 0)
        self.text = s

    def offset(self, sign: int = 1) -> pd.DateOffset:
        return pd.DateOffset(years=sign * self.years, months=sign * self.months,
                             days=sign * (self.days + 7 * self.weeks), hours=sign * self.hours,
                             minutes=sign * self.minutes, seconds=sign * self.seconds)

    def __repr__(self):
        return f"period({self.text})"

    def __eq__(self, o):
        return isinstance(o, Period) and o.text == self.text

    def __hash__(self):
        return hash(self.text)


@_reg("dateTime", _const("timestamp"))
def _date_time(args, ts, n):
    v = args[0]
    if len(args) > 1 and args[1] is not None:
        return _unix_parse([v, args[1]], ts, n, out="timestamp")
    return _ts(v, ts[0], n)


@_reg("dateTimeWithTZ", _const("timestamp"))
def _date_time_tz(args, ts, n):
    return _ts(args[0], ts[0], n)


@_reg("withZone", _first)
def _with_zone(args, ts, n):
    from ..query.intervals import tz_offset_ms

    v = args[0]
    off = tz_offset_ms(args[1]) if len(args) > 1 and args[1] is not None else 0
    return v + pd.Timedelta(milliseconds=off) if off else v


@_reg("period", _const("period"))
def _period(args, ts, n):
    if is_vec(args[0]):
        raise AnalysisError("period() expects a literal")
    return None if args[0] is None else Period(args[0])


def _date_shift(sign):
    def impl(args, ts, n):
        v = _ts(args[0], ts[0], n)
        p = args[1]
        if p is None:
            return None
        if isinstance(p, A.IntervalLit):
            return _add_interval(v, p, sign)
        if not isinstance(p, Period):
            p = Period(str(p))
        if not is_vec(v):
            return None if v is None else pd.Timestamp(v) + p.offset(sign)
        return v + p.offset(sign)

    return impl


_reg("datePlus", _const("timestamp"))(_date_shift(1))
_reg("dateMinus", _const("timestamp"))(_date_shift(-1))


def _date_cmp(op):
    def impl(args, ts, n):
        a = _ts(args[0], ts[0], n)
        b = _ts(args[1], ts[1], n)
        if not is_vec(a) and not is_vec(b):
            if a is None or b is None:
                return None
            return op(pd.Timestamp(a), pd.Timestamp(b))
        r = pd.Series(op(a, b)).astype("boolean")
        for x in (a, b):
            if is_vec(x):
                r = r.mask(x.isna().to_numpy(), pd.NA)
        return r

    return impl


_reg("dateIsBefore", _const("boolean"))(_date_cmp(lambda a, b: a < b))
_reg("dateIsAfter", _const("boolean"))(_date_cmp(lambda a, b: a > b))
_reg("dateIsBeforeOrEqual", _const("boolean"))(_date_cmp(lambda a, b: a <= b))
_reg("dateIsAfterOrEqual", _const("boolean"))(_date_cmp(lambda a, b: a >= b))
_reg("dateIsEqual", _const("boolean"))(_date_cmp(lambda a, b: a == b))


@_reg("dateBetween", _const("boolean"))
def _date_between(args, ts, n):
    lo = _date_cmp(lambda a, b: a >= b)([args[0], args[1]], [ts[0], ts[1]], n)
    hi = _date_cmp(lambda a, b: a <= b)([args[0], args[2]], [ts[0], ts[2]], n)
    return _binop_bool(lo, hi, n)


def _binop_bool(a, b, n):
    if not is_vec(a) and not is_vec(b):
        return None if a is None or b is None else (a and b)
    return broadcast(a, n, "boolean") & broadcast(b, n, "boolean")


# Joda field accessors applied to dateTime values (TimeElementExtractor, DateTimeExtractor.scala:157-189)
JODA_FIELD_FORMATS = {
    "era": "GG", "centuryofera": "CC", "yearofera": "YYYY", "yearofcentury": "yy", "year": "yyyy",
    "weekyear": "xxxx", "monthofyear": "MM", "monthofyearname": "MMMM", "weekofweekyear": "ww",
    "dayofyear": "DDD", "dayofmonth": "dd", "dayofweek": "ee", "dayofweekname": "EEEE",
    "hourofday": "HH", "minuteofhour": "mm", "secondofminute": "ss", "millisofsecond": "SSS",
}

_reg("monthOfYear", _const("int"))(_date_part(lambda d: d.month, lambda t: t.month))
_reg("monthOfYearName", _const("string"))(_date_part(lambda d: d.month_name().astype("string"),
                                                     lambda t: t.month_name(), "string"))
_reg("dayOfWeekName", _const("string"))(_date_part(lambda d: d.day_name().astype("string"),
                                                   lambda t: t.day_name(), "string"))
_reg("weekOfWeekyear", _const("int"))(_date_part(lambda d: d.isocalendar().week, lambda t: t.isocalendar()[1]))
_reg("weekyear", _const("int"))(_date_part(lambda d: d.isocalendar().year, lambda t: t.isocalendar()[0]))
_reg("hourOfDay", _const("int"))(_date_part(lambda d: d.hour, lambda t: t.hour))
_reg("minuteOfHour", _const("int"))(_date_part(lambda d: d.minute, lambda t: t.minute))
_reg("secondOfMinute", _const("int"))(_date_part(lambda d: d.second, lambda t: t.second))
_reg("millisOfSecond", _const("int"))(_date_part(lambda d: d.microsecond // 1000, lambda t: t.microsecond // 1000))
_reg("yearOfEra", _const("int"))(_date_part(lambda d: d.year, lambda t: t.year))
_reg("yearOfCentury", _const("int"))(_date_part(lambda d: d.year % 100, lambda t: t.year % 100))
_reg("centuryOfEra", _const("int"))(_date_part(lambda d: d.year // 100, lambda t: t.year // 100))
_reg("era", _const("int"))(_date_part(lambda d: (d.year > 0).astype(int), lambda t: int(t.year > 0)))
_reg("millis", _const("bigint"))(_date_part(lambda d: pd.Series(d.tz_localize(None) if False else d.floor("ms"))
                                            .astype("int64") // 10 ** 6, lambda t: int(t.value // 10 ** 6)))


def _add_interval(v, iv: A.IntervalLit, sign: int):
    off = pd.DateOffset(months=sign * iv.months, days=sign * iv.days, microseconds=sign * iv.micros)
    if not is_vec(v):
        return None if v is None else pd.Timestamp(v) + off
    return v + off


# ------------------------------------------------------------------------------------------------
# misc
@_reg("grouping__id spark_partition_id monotonically_increasing_id", _const("bigint"))
def _misc_ids(args, ts, n):
    return pd.Series(np.arange(n), dtype="Int64")


@_reg("element_at", _const("string"))
def _element_at(args, ts, n):
    return _map_scalar(lambda a, i: a[int(i) - 1] if 0 < int(i) <= len(a) else None, "string")(args, ts, n)


@_reg("array", _const("array"))
def _array(args, ts, n):
    cols = [a.tolist() if is_vec(a) else [a] * n for a in args]
    return pd.Series([list(r) for r in zip(*cols)] if cols else [[] for _ in range(n)], dtype=object)


def _quantile_at(args, ts, n):
    # element i of a pushed quantiles aggregator's result column (one array per group)
    v, i = args[0], int(args[1])
    rows = v.tolist() if is_vec(v) else [v] * n
    vals = [r[i] if isinstance(r, (list, tuple, np.ndarray)) else None for r in rows]
    if any(x is None for x in vals):
        return pd.Series([x.item() if isinstance(x, np.generic) else x for x in vals], dtype=object)
    return pd.Series(np.asarray(vals))


_reg("__quantile_at", _const("double"))(_quantile_at)
_reg("__quantile_at_long", _const("bigint"))(_quantile_at)


@_reg("size", _const("int"))
def _size(args, ts, n):
    return _map_scalar(lambda a: len(a), "int")(args, ts, n)


@_reg("md5", _const("string"))
def _md5(args, ts, n):
    import hashlib

    return _map_scalar(lambda s: hashlib.md5(str(s).encode()).hexdigest(), "string")(
        [_str(args[0], ts[0], n)], ["string"], n)


def _hex_of(v):
    if isinstance(v, (bytes, bytearray)):
        return bytes(v).hex().upper()
    if isinstance(v, bool):
        v = int(v)
    if isinstance(v, (int, np.integer)):
        return format(int(v) & 0xFFFFFFFFFFFFFFFF, "X")
    if isinstance(v, float):
        return format(int(v) & 0xFFFFFFFFFFFFFFFF, "X")
    return str(v).encode("utf-8").hex().upper()


@_reg("hex", _const("string"))
def _hex(args, ts, n):
    return _map_scalar(_hex_of, "string")(args, ts, n)


def _unhex_of(s):
    s = str(s)
    if len(s) % 2:
        s = "0" + s
    try:
        return bytes.fromhex(s)
    except ValueError:
        return None


@_reg("unhex", _const("binary"))
def _unhex(args, ts, n):
    return _map_scalar(_unhex_of, "binary")(args, ts, n)


@_reg("base64", _const("string"))
def _base64(args, ts, n):
    import base64

    return _map_scalar(lambda v: base64.b64encode(v if isinstance(v, (bytes, bytearray)) else str(v).encode())
                       .decode(), "string")(args, ts, n)


@_reg("unbase64", _const("binary"))
def _unbase64(args, ts, n):
    import base64
    import binascii

    def f(v):
        try:
            return base64.b64decode(str(v))
        except (binascii.Error, ValueError):
            return None
    return _map_scalar(f, "binary")(args, ts, n)


def function_names() -> List[str]:
    return sorted(_FUNCS)


def is_deterministic(e: A.Expr) -> bool:
    return not any(isinstance(x, A.Call) and x.name in ("rand", "random", "current_date", "current_timestamp",
                                                         "now", "monotonically_increasing_id")
                   for x in e.walk())


def constant_fold(e: A.Expr) -> A.Expr:
    """Fold sub-expressions without column references into literals."""
    def fold(x: A.Expr):
        if isinstance(x, (A.Lit, A.Ref, A.IntervalLit, A.SubqueryExpr, A.Alias, A.WindowExpr)) or not x.children:
            return None
        if isinstance(x, A.Call) and (x.is_agg or x.name in A.WINDOW_FUNCS):
            return None
        if isinstance(x, A.Case):
            # branches with a constant condition: drop the false / NULL ones, stop at a true one
            whens = [(c, v) for c, v in x.whens if not (isinstance(c, A.Lit) and c.value in (False, None))]
            t = typeof(x)
            if whens and isinstance(whens[0][0], A.Lit) and whens[0][0].value is True:
                r = whens[0][1]
                return r if typeof(r) == t else A.Cast(r, t)
            if not whens:
                r = x.else_ if x.else_ is not None else A.Lit(None, t)
                return r if typeof(r) == t else A.Cast(r, t)
            if len(whens) != len(x.whens):
                return A.Case(tuple(whens), x.else_)
        if any(not isinstance(c, A.Lit) for c in x.children):
            return None
        if not is_deterministic(x):
            return None
        try:
            v = evaluate(x, Frame({}, 1))
        except Exception:
            return None
        if isinstance(v, Period):
            return A.Lit(v, "period")
        if is_vec(v) or isinstance(v, A.IntervalLit):
            return None
        t = typeof(x)
        if isinstance(v, pd.Timestamp):
            return A.Lit(v, t)
        if isinstance(v, np.generic):
            v = v.item()
        return A.Lit(v, t)

    return e.transform(fold)
