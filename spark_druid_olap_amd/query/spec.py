"""Druid query model with Druid-compatible JSON (including the reference's ``jsonClass`` hints).

Covers every spec class of ``sd/DruidQuerySpec.scala`` (extraction functions 31-103, dimension
specs 108-138, granularity 140-150, filters 152-281, aggregations 283-377, post-aggregations
379-430, limit/having/topN metric 437-506, segment intervals 509-541, context 558-571, and the
query types GroupBy/TimeSeries/TopN/Search/Select 573-1127) plus the thetaSketch aggregator the
index spec declares but the reference never modelled.

``to_json()`` emits ``{"jsonClass": <class>, "type"/"queryType": ...}`` exactly like the
reference's json4s ShortTypeHints (``sd/Utils.scala:38-105``), and ``from_json()`` accepts both
that form and plain Druid JSON (dispatching on ``type`` / ``queryType``).
"""
from __future__ import annotations

import copy
import dataclasses
import json
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Union

from .granularity import Granularity

_BY_CLASS: Dict[str, type] = {}
_BY_TYPE: Dict[str, Dict[str, type]] = {}


def _register(family: str, *types: str):
    def deco(cls):
        _BY_CLASS[cls.__name__] = cls
        for t in types:
            _BY_TYPE.setdefault(family, {})[t] = cls
        cls._family = family
        return cls

    return deco


class Spec:
    """Base: dataclass <-> Druid JSON with jsonClass hints."""

    _family = ""
    _renames: Dict[str, str] = {}

    def to_json(self) -> Dict[str, Any]:
        out: Dict[str, Any] = {"jsonClass": type(self).__name__}
        for f in dataclasses.fields(self):
            if f.name.startswith("_"):
                continue
            v = getattr(self, f.name)
            if v is None:
                continue
            key = self._renames.get(f.name, f.name)
            out[key] = _enc(v)
        return out

    def to_json_str(self, indent: Optional[int] = 2) -> str:
        return json.dumps(self.to_json(), indent=indent)

    def copy(self, **changes):
        c = copy.copy(self)
        c.__dict__.pop("_deferred_memo", None)  # (find_deferred's memo describes the original)
        for k, v in changes.items():
            setattr(c, k, v)
        return c


def _enc(v):
    if isinstance(v, Spec):
        return v.to_json()
    if isinstance(v, Granularity):
        return v.to_json()
    if isinstance(v, list):
        return [_enc(x) for x in v]
    if isinstance(v, dict):
        return {k: _enc(x) for k, x in v.items()}
    return v


def from_json(d: Union[str, Dict[str, Any]], family: Optional[str] = None):
    """Decode any spec (query, filter, aggregation, ...) from Druid JSON."""
    if isinstance(d, str):
        d = json.loads(d)
    if d is None:
        return None
    cls = None
    jc = d.get("jsonClass")
    if jc and jc in _BY_CLASS:
        cls = _BY_CLASS[jc]
    elif family is not None:
        key = d.get("queryType") if family == "query" else d.get("type")
        cls = _BY_TYPE.get(family, {}).get(key)
        if cls is None and family == "dimension" and isinstance(d, dict) and "dimension" in d:
            cls = DefaultDimensionSpec
    if cls is None:
        raise ValueError(f"cannot decode spec {d!r} (family={family})")
    return cls._decode(d)


def _fieldmap(cls):
    inv = {v: k for k, v in cls._renames.items()}
    return {f.name: f for f in dataclasses.fields(cls)}, inv


class _Decodable:
    _nested: Dict[str, str] = {}  # field -> family (list or single)

    @classmethod
    def _decode(cls, d):
        fmap, inv = _fieldmap(cls)
        kw = {}
        for k, v in d.items():
            if k == "jsonClass":
                continue
            name = inv.get(k, k)
            if name not in fmap:
                continue
            fam = cls._nested.get(name)
            if fam == "granularity":
                v = Granularity.parse(v)
            elif fam is not None and v is not None:
                if isinstance(v, list):
                    v = [from_json(x, fam) if isinstance(x, dict) else x for x in v]
                elif isinstance(v, dict):
                    v = from_json(v, fam)
            kw[name] = v
        return cls(**kw)


# ============================================================================ extraction functions
@_register("extraction", "regex")
@dataclass
class RegexExtractionFunctionSpec(Spec, _Decodable):
    expr: str
    type: str = "regex"


@_register("extraction", "partial")
@dataclass
class PartialExtractionFunctionSpec(Spec, _Decodable):
    expr: str
    type: str = "partial"


@_register("extraction", "searchQuery")
@dataclass
class SearchQueryExtractionFunctionSpec(Spec, _Decodable):
    query: str
    type: str = "searchQuery"


@_register("extraction", "timeFormat")
@dataclass
class TimeFormatExtractionFunctionSpec(Spec, _Decodable):
    format: str
    timeZone: Optional[str] = None
    locale: Optional[str] = None
    type: str = "timeFormat"


@_register("extraction", "time")
@dataclass
class TimeParsingExtractionFunctionSpec(Spec, _Decodable):
    timeFormat: str
    resultFormat: str
    type: str = "time"


@_register("extraction", "javascript")
@dataclass
class JavaScriptExtractionFunctionSpec(Spec, _Decodable):
    function: str
    injective: bool = False
    type: str = "javascript"


@_register("extraction", "lookup")
@dataclass
class InExtractionFnSpec(Spec, _Decodable):
    """Druid 'lookup' extraction over a map: the reference's IN-list encoding (99-103)."""
    lookup: Dict[str, Any]
    retainMissingValue: bool = False
    replaceMissingValueWith: Optional[str] = None
    injective: bool = False
    type: str = "lookup"

    @staticmethod
    def for_values(values):
        return InExtractionFnSpec({"type": "map", "map": {str(v): "true" for v in values}})


@_register("extraction", "substring")
@dataclass
class SubstringExtractionFunctionSpec(Spec, _Decodable):
    index: int
    length: Optional[int] = None
    type: str = "substring"


@_register("extraction", "upper")
@dataclass
class UpperExtractionFunctionSpec(Spec, _Decodable):
    type: str = "upper"


@_register("extraction", "lower")
@dataclass
class LowerExtractionFunctionSpec(Spec, _Decodable):
    type: str = "lower"


# ============================================================================ dimension specs
@_register("dimension", "default")
@dataclass
class DefaultDimensionSpec(Spec, _Decodable):
    dimension: str
    outputName: Optional[str] = None
    type: str = "default"

    def __post_init__(self):
        if self.outputName is None:
            self.outputName = self.dimension


@_register("dimension", "extraction")
@dataclass
class ExtractionDimensionSpec(Spec, _Decodable):
    dimension: str
    outputName: str
    extractionFn: Any = None
    type: str = "extraction"
    _nested = {"extractionFn": "extraction"}


# ============================================================================ filters
@_register("filter", "noop")
@dataclass
class NoopFilterSpec(Spec, _Decodable):
    type: str = "noop"


@_register("filter", "selector")
@dataclass
class SelectorFilterSpec(Spec, _Decodable):
    dimension: str
    value: Any
    type: str = "selector"


@_register("filter", "idRange")
@dataclass
class IdRangeFilterSpec(Spec, _Decodable):
    """Engine extension: rows whose dimension dictionary id lies in [lo, hi) (dictionaries are
    sorted, so this is a value range).  Emitted by the engine itself for key-range passes
    (engine/executor.py KeyRangePasses), never by the SQL planner."""
    dimension: str
    lo: int
    hi: int
    type: str = "idRange"


@_register("filter", "regex")
@dataclass
class RegexFilterSpec(Spec, _Decodable):
    dimension: str
    pattern: str
    type: str = "regex"


@_register("filter", "search")
@dataclass
class ContainsFilterSpec(Spec, _Decodable):
    """{type: search, dimension, query: {type: contains|insensitive_contains, value, caseSensitive}}"""
    dimension: str
    query: Dict[str, Any]
    type: str = "search"


@_register("filter", "and", "or")
@dataclass
class LogicalFilterSpec(Spec, _Decodable):
    type: str
    fields: List[Any]
    _nested = {"fields": "filter"}


@_register("filter", "not")
@dataclass
class NotFilterSpec(Spec, _Decodable):
    field: Any
    type: str = "not"
    _nested = {"field": "filter"}


@_register("filter", "extraction")
@dataclass
class ExtractionFilterSpec(Spec, _Decodable):
    dimension: str
    value: Any
    extractionFn: Any
    type: str = "extraction"
    _nested = {"extractionFn": "extraction"}


@_register("filter", "javascript")
@dataclass
class JavascriptFilterSpec(Spec, _Decodable):
    dimension: str
    function: str
    type: str = "javascript"


@_register("filter", "expression")
@dataclass
class ExpressionFilterSpec(Spec, _Decodable):
    """Row predicate over several columns, ``<arith> <cmp> <arith>`` (Druid's native expression
    filter syntax, arithmetic in the javascript-aggregator subset).  The reference cannot push
    these (a Druid javascript filter sees one dimension, ``sd/jscodegen/JSCodeGenerator.scala``);
    here they run in the scan kernel's expression VM (TPC-H Q4/Q12 ``l_commitdate < l_receiptdate``,
    Q5 ``c_nation = s_nation``)."""
    expression: str
    type: str = "expression"


@_register("datasource", "query")
@dataclass
class QueryDataSourceSpec(Spec, _Decodable):
    """Druid's query data source: the rows of an inner (groupBy) query are the input of the outer
    groupBy -- nested aggregation (TPC-H Q13 ``count(*) ... group by c_count`` over per-customer
    order counts; SQL count(DISTINCT) rewritten as two aggregation levels).  The engine runs the
    outer level on the inner query's device-resident partials (engine/nested.py)."""
    query: Any
    type: str = "query"
    _nested = {"query": "query"}


@dataclass
class DeferredFilterSpec(Spec):
    """A filter whose operand is an uncorrelated scalar subquery (TPC-H Q22 ``c_acctbal >
    (select avg(c_acctbal) ...)``).  Spark runs such subqueries before the main plan
    (``ScalarSubquery``); the planner keeps the predicate here with ``build(values)`` -> concrete
    filter, and the executor runs the subqueries (pushed GPU queries themselves) and calls
    ``resolve_deferred`` before lowering.  Never reaches the engine unresolved."""
    expression: str
    type: str = "deferred"

    def __post_init__(self):
        self.subqueries: list = []
        self.build = None


def find_deferred(spec) -> List["DeferredFilterSpec"]:
    """The DeferredFilterSpecs of a spec tree (memoised on the spec: specs are not mutated once
    built -- ``copy`` / ``resolve_deferred`` make new ones -- and servers ask for every statement)."""
    memo = getattr(spec, "__dict__", None)
    if memo is not None and "_deferred_memo" in memo:
        return list(memo["_deferred_memo"])
    out = _find_deferred(spec)
    if memo is not None:
        memo["_deferred_memo"] = tuple(out)
    return out


def _find_deferred(spec) -> List["DeferredFilterSpec"]:
    out: List[DeferredFilterSpec] = []

    def go(v):
        if isinstance(v, DeferredFilterSpec):
            out.append(v)
        elif isinstance(v, Spec):
            for f in dataclasses.fields(v):
                go(getattr(v, f.name))
        elif isinstance(v, (list, tuple)):
            for x in v:
                go(x)

    go(spec)
    return out


def resolve_deferred(spec, values: Dict[int, Any]):
    """Copy of ``spec`` with every DeferredFilterSpec replaced by ``build(values)`` (``values``:
    id(subquery expr) -> its scalar result).  Unchanged sub-specs are shared, not copied."""

    def go(v):
        if isinstance(v, DeferredFilterSpec):
            return v.build(values)
        if isinstance(v, Spec):
            changes = {}
            for f in dataclasses.fields(v):
                x = getattr(v, f.name)
                y = go(x)
                if y is not x:
                    changes[f.name] = y
            return v.copy(**changes) if changes else v
        if isinstance(v, list):
            ys = [go(x) for x in v]
            return ys if any(a is not b for a, b in zip(ys, v)) else v
        return v

    return go(spec)


@_register("filter", "bound")
@dataclass
class BoundFilterSpec(Spec, _Decodable):
    dimension: str
    lower: Optional[Any] = None
    upper: Optional[Any] = None
    lowerStrict: bool = False
    upperStrict: bool = False
    alphaNumeric: bool = False
    type: str = "bound"


@_register("filter", "in")
@dataclass
class InFilterSpec(Spec, _Decodable):
    dimension: str
    values: List[Any]
    type: str = "in"


@_register("filter", "spatial")
@dataclass
class SpatialFilterSpec(Spec, _Decodable):
    dimension: str
    bound: Dict[str, Any]  # {type: rectangular, minCoords: [...], maxCoords: [...]}
    type: str = "spatial"


@_register("filter", "interval")
@dataclass
class IntervalFilterSpec(Spec, _Decodable):
    dimension: str
    intervals: List[str]
    type: str = "interval"


# ============================================================================ aggregations
FUNCTION_AGGS = ("count", "longSum", "doubleSum", "longMin", "longMax", "doubleMin", "doubleMax")


@_register("aggregation", *FUNCTION_AGGS)
@dataclass
class FunctionAggregationSpec(Spec, _Decodable):
    type: str
    name: str
    fieldName: Optional[str] = None


@_register("aggregation", "cardinality")
@dataclass
class CardinalityAggregationSpec(Spec, _Decodable):
    name: str
    fieldNames: List[str]
    byRow: bool = True
    type: str = "cardinality"


@_register("aggregation", "hyperUnique")
@dataclass
class HyperUniqueAggregationSpec(Spec, _Decodable):
    name: str
    fieldName: str
    type: str = "hyperUnique"


@_register("aggregation", "javascript")
@dataclass
class JavascriptAggregationSpec(Spec, _Decodable):
    name: str
    fieldNames: List[str]
    fnAggregate: str
    fnCombine: str
    fnReset: str
    type: str = "javascript"


@_register("aggregation", "filtered")
@dataclass
class FilteredAggregationSpec(Spec, _Decodable):
    filter: Any
    aggregator: Any
    name: Optional[str] = None
    type: str = "filtered"
    _nested = {"filter": "filter", "aggregator": "aggregation"}

    def __post_init__(self):
        if self.name is None and self.aggregator is not None:
            self.name = self.aggregator.name


@_register("aggregation", "thetaSketch")
@dataclass
class ThetaSketchAggregationSpec(Spec, _Decodable):
    name: str
    fieldName: str
    size: int = 16384
    isInputThetaSketch: bool = False
    type: str = "thetaSketch"


@_register("aggregation", "quantiles")
@dataclass
class QuantilesAggregationSpec(Spec, _Decodable):
    """Exact per-group order statistics of a numeric column: one value per fraction in the result
    column.  ``interpolate``: Spark's ``percentile`` (linear interpolation between the ranks
    floor / ceil of p (n-1), a double); otherwise the element at rank max(0, ceil(p n) - 1)
    (``percentile_approx``'s contract, met exactly), of the column's own type."""
    name: str
    fieldName: str
    fractions: List[float] = field(default_factory=list)
    interpolate: bool = True
    type: str = "quantiles"


@_register("aggregation", "distinctCount")
@dataclass
class DistinctCountAggregationSpec(Spec, _Decodable):
    """Exact number of distinct non-null values of one dimension among the selected rows (Druid's
    ``distinctCount`` extension: a bitmap of dictionary ids per group).  This engine's null is the
    ``""`` dictionary entry, as for ``count(dim)``; the result is a long."""
    name: str
    fieldName: str
    type: str = "distinctCount"


@_register("aggregation", "variance")
@dataclass
class VarianceAggregationSpec(Spec, _Decodable):
    """Variance of a long / decimal / double metric over the selected rows (the ``variance``
    aggregator of Druid's stats extension).  ``estimator``: ``"sample"`` (n - 1 in the denominator,
    the default) or ``"population"`` (n).  The result is a double, NaN for a group of fewer than two
    rows (one row, under ``"population"``: 0)."""
    name: str
    fieldName: str
    estimator: str = "sample"
    type: str = "variance"


@_register("aggregation", "skewness")
@dataclass
class SkewnessAggregationSpec(Spec, _Decodable):
    """Skewness of a long / decimal / double metric over the selected rows, Spark's
    ``sqrt(n) M3 / M2^1.5`` with ``Mk`` the sum of (x - mean)^k: a double, NaN for a group whose
    rows hold one value only.  The type name is this project's own, as ``covariance``."""
    name: str
    fieldName: str
    type: str = "skewness"


@_register("aggregation", "kurtosis")
@dataclass
class KurtosisAggregationSpec(Spec, _Decodable):
    """Excess kurtosis of a long / decimal / double metric over the selected rows, Spark's
    ``n M4 / M2^2 - 3``: a double, NaN for a group whose rows hold one value only.  The type name is
    this project's own, as ``covariance``."""
    name: str
    fieldName: str
    type: str = "kurtosis"


@_register("aggregation", "covariance")
@dataclass
class CovarianceAggregationSpec(Spec, _Decodable):
    """Covariance of two long / decimal / double metrics over the selected rows.  ``estimator``:
    ``"sample"`` (n - 1 in the denominator, the default) or ``"population"`` (n).  The result is a
    double, NaN for a group of fewer than two rows (one row, under ``"population"``: 0).  The type
    name is this project's own: Druid's stats extension has no two-column aggregator."""
    name: str
    fieldName: str
    fieldName2: str
    estimator: str = "sample"
    type: str = "covariance"


@_register("aggregation", "correlation")
@dataclass
class CorrelationAggregationSpec(Spec, _Decodable):
    """Pearson correlation of two long / decimal / double metrics over the selected rows: a double
    in [-1, 1], NaN for a group of fewer than two rows or one in which a column is constant.  The
    type name is this project's own, as ``covariance``."""
    name: str
    fieldName: str
    fieldName2: str
    type: str = "correlation"


@dataclass
class _ExtremeBySpec(Spec, _Decodable):
    name: str
    fieldName: str
    byFieldName: str


@_register("aggregation", "maxBy")
@dataclass
class MaxByAggregationSpec(_ExtremeBySpec):
    """``fieldName`` (a long / decimal / double metric) of the selected row with the largest
    ``byFieldName`` (such a metric, or ``"__time"``); among rows that tie, the last in the shard's
    storage order.  Ordered by ``"__time"`` this is Druid's longLast / doubleLast.  The result has
    the payload's type (long, or double for double and decimal payloads).  The type name is this
    project's own: Druid has no two-column aggregator."""
    type: str = "maxBy"


@_register("aggregation", "minBy")
@dataclass
class MinByAggregationSpec(_ExtremeBySpec):
    """``fieldName`` of the selected row with the smallest ``byFieldName``; among rows that tie, the
    first in storage order (ordered by ``"__time"``: Druid's longFirst / doubleFirst).  The type
    name is this project's own, as ``maxBy``."""
    type: str = "minBy"


@_register("aggregation", "fixedBucketsHistogram")
@dataclass
class FixedBucketsHistogramAggregationSpec(Spec, _Decodable):
    """Counts of the selected rows' ``fieldName`` (a long / decimal / double metric) in
    ``numBuckets`` equal buckets over [``lowerLimit``, ``upperLimit``) -- the aggregator of Druid's
    histogram extension -- or, this project's own, in the buckets between the strictly ascending
    ``breaks``, used instead of the three limits when present.  Limits and breaks are read as the
    exact decimal value of their shortest text (0.1 is 1/10); a value v is in bucket i iff
    e_i <= v < e_{i+1}.  The result is one array of numBuckets + 2 longs per group: [below,
    c_0 .. c_{B-1}, above]; NaN counts as above.  ``outlierHandlingMode``: ``"ignore"`` reports the
    array as is, ``"overflow"`` adds below into c_0 and above into c_{B-1} and reports 0 at the two
    ends (``"clip"`` is not supported)."""
    name: str
    fieldName: str
    numBuckets: Optional[int] = None
    lowerLimit: Optional[float] = None
    upperLimit: Optional[float] = None
    outlierHandlingMode: str = "ignore"
    breaks: Optional[List[float]] = None
    type: str = "fixedBucketsHistogram"


# ============================================================================ post aggregations
@_register("postagg", "fieldAccess")
@dataclass
class FieldAccessPostAggregationSpec(Spec, _Decodable):
    fieldName: str
    name: Optional[str] = None
    type: str = "fieldAccess"


@_register("postagg", "constant")
@dataclass
class ConstantPostAggregationSpec(Spec, _Decodable):
    value: float
    name: Optional[str] = None
    type: str = "constant"


@_register("postagg", "hyperUniqueCardinality")
@dataclass
class HyperUniqueCardinalityPostAggregationSpec(Spec, _Decodable):
    fieldName: str
    name: Optional[str] = None
    type: str = "hyperUniqueCardinality"


@_register("postagg", "stddev")
@dataclass
class StddevPostAggregationSpec(Spec, _Decodable):
    """Square root of the named ``variance`` aggregator's column (the stats extension's ``stddev``)."""
    name: str
    fieldName: str
    type: str = "stddev"


@_register("postagg", "arithmetic")
@dataclass
class ArithmeticPostAggregationSpec(Spec, _Decodable):
    fn: str
    fields: List[Any]
    name: Optional[str] = None
    ordering: Optional[str] = None
    type: str = "arithmetic"
    _nested = {"fields": "postagg"}


@_register("postagg", "javascript")
@dataclass
class JavascriptPostAggregationSpec(Spec, _Decodable):
    name: str
    fieldNames: List[str]
    function: str
    type: str = "javascript"


# ============================================================================ limit / having / topN metric
@_register("orderby", "ordering")
@dataclass
class OrderByColumnSpec(Spec, _Decodable):
    dimension: str
    direction: str = "ascending"  # ascending | descending
    dimensionOrder: Optional[str] = None

    @classmethod
    def _decode(cls, d):
        if isinstance(d, str):
            return OrderByColumnSpec(d)
        return super()._decode(d)

    @property
    def ascending(self) -> bool:
        return self.direction.lower().startswith("asc")


@_register("limit", "default")
@dataclass
class LimitSpec(Spec, _Decodable):
    limit: int
    columns: List[Any] = field(default_factory=list)
    type: str = "default"

    @classmethod
    def _decode(cls, d):
        cols = [OrderByColumnSpec(c) if isinstance(c, str) else OrderByColumnSpec._decode(c)
                for c in d.get("columns", [])]
        return LimitSpec(int(d.get("limit", 2 ** 31 - 1)), cols)


@_register("having", "equalTo", "greaterThan", "lessThan")
@dataclass
class ComparisonHavingSpec(Spec, _Decodable):
    type: str
    aggregation: str
    value: float


@_register("having", "and", "or")
@dataclass
class LogicalHavingSpec(Spec, _Decodable):
    type: str
    havingSpecs: List[Any]
    _nested = {"havingSpecs": "having"}


@_register("having", "not")
@dataclass
class NotHavingSpec(Spec, _Decodable):
    havingSpec: Any
    type: str = "not"
    _nested = {"havingSpec": "having"}


@_register("topnmetric", "numeric")
@dataclass
class NumericTopNMetricSpec(Spec, _Decodable):
    metric: str
    type: str = "numeric"


@_register("topnmetric", "lexicographic")
@dataclass
class LexiCographicTopNMetricSpec(Spec, _Decodable):
    previousStop: Optional[str] = None
    type: str = "lexicographic"


@_register("topnmetric", "alphaNumeric")
@dataclass
class AlphaNumericTopNMetricSpec(Spec, _Decodable):
    previousStop: Optional[str] = None
    type: str = "alphaNumeric"


@_register("topnmetric", "inverted")
@dataclass
class InvertedTopNMetricSpec(Spec, _Decodable):
    metric: Any
    type: str = "inverted"
    _nested = {"metric": "topnmetric"}


@_register("paging", "paging")
@dataclass
class PagingSpec(Spec, _Decodable):
    pagingIdentifiers: Dict[str, int] = field(default_factory=dict)
    threshold: int = 10000
    fromNext: bool = True


@_register("searchquery", "contains", "insensitive_contains", "fragment", "regex")
@dataclass
class SearchQueryQuerySpec(Spec, _Decodable):
    type: str
    value: Any = None
    caseSensitive: bool = False
    values: Optional[List[str]] = None


@_register("segintervals", "segments")
@dataclass
class SegmentIntervals(Spec, _Decodable):
    """Segment-pinned intervals (reference 509-541); used for per-GPU partial queries."""
    segments: List[Dict[str, Any]]
    type: str = "segments"


# ============================================================================ context
@dataclass
class QuerySpecContext(Spec, _Decodable):
    queryId: Optional[str] = None
    timeout: Optional[int] = None
    priority: Optional[int] = None
    useCache: Optional[bool] = None
    populateCache: Optional[bool] = None
    bySegment: Optional[bool] = None
    chunkPeriod: Optional[str] = None
    minTopNThreshold: Optional[int] = None
    maxResults: Optional[int] = None
    maxIntermediateRows: Optional[int] = None
    groupByStrategy: Optional[str] = None
    # engine extension: floating-point sums in exact fixed point (bitwise run-to-run reproducible
    # under any atomic / merge order); see engine/lower.py Lowerer.deterministic
    deterministic: Optional[bool] = None


_BY_CLASS["QuerySpecContext"] = QuerySpecContext


def _ctx(d):
    if d is None:
        return None
    if isinstance(d, QuerySpecContext):
        return d
    fmap, _ = _fieldmap(QuerySpecContext)
    return QuerySpecContext(**{k: v for k, v in d.items() if k in fmap})


# ============================================================================ queries
class QuerySpec(Spec):
    """Common behaviour of all query types (reference trait QuerySpec, 573-604)."""

    queryType: str = ""

    def intervalList(self) -> List[str]:
        return list(self.intervals)

    def setIntervals(self, ints: List[str]) -> "QuerySpec":
        return self.copy(intervals=list(ints))

    def setFilter(self, f) -> "QuerySpec":
        return self.copy(filter=f)

    @property
    def aggregation_specs(self) -> List[Any]:
        return list(getattr(self, "aggregations", None) or [])

    @classmethod
    def _decode(cls, d):
        obj = _Decodable._decode.__func__(cls, d)  # type: ignore[attr-defined]
        if getattr(obj, "context", None) is not None:
            obj.context = _ctx(obj.context)
        if isinstance(getattr(obj, "intervals", None), dict):
            obj.intervals = [s["itvl"] for s in obj.intervals.get("segments", [])]
        return obj


@_register("query", "groupBy")
@dataclass
class GroupByQuerySpec(QuerySpec, _Decodable):
    dataSource: str
    dimensions: List[Any]
    limitSpec: Optional[LimitSpec] = None
    having: Optional[Any] = None
    granularity: Granularity = field(default_factory=lambda: Granularity("all"))
    filter: Optional[Any] = None
    aggregations: List[Any] = field(default_factory=list)
    postAggregations: Optional[List[Any]] = None
    intervals: List[str] = field(default_factory=list)
    context: Optional[QuerySpecContext] = None
    queryType: str = "groupBy"
    _nested = {"dataSource": "datasource", "dimensions": "dimension", "limitSpec": "limit", "having": "having",
               "granularity": "granularity",
               "filter": "filter", "aggregations": "aggregation", "postAggregations": "postagg"}

    @classmethod
    def _decode(cls, d):
        return QuerySpec._decode.__func__(cls, d)


@_register("query", "timeseries")
@dataclass
class TimeSeriesQuerySpec(QuerySpec, _Decodable):
    dataSource: str
    intervals: List[str]
    descending: bool = False
    granularity: Granularity = field(default_factory=lambda: Granularity("all"))
    filter: Optional[Any] = None
    aggregations: List[Any] = field(default_factory=list)
    postAggregations: Optional[List[Any]] = None
    context: Optional[QuerySpecContext] = None
    queryType: str = "timeseries"
    _nested = {"granularity": "granularity", "filter": "filter", "aggregations": "aggregation",
               "postAggregations": "postagg"}

    @classmethod
    def _decode(cls, d):
        return QuerySpec._decode.__func__(cls, d)


@_register("query", "topN")
@dataclass
class TopNQuerySpec(QuerySpec, _Decodable):
    dataSource: str
    dimension: Any
    metric: Any
    threshold: int
    intervals: List[str] = field(default_factory=list)
    granularity: Granularity = field(default_factory=lambda: Granularity("all"))
    filter: Optional[Any] = None
    aggregations: List[Any] = field(default_factory=list)
    postAggregations: Optional[List[Any]] = None
    context: Optional[QuerySpecContext] = None
    queryType: str = "topN"
    _nested = {"dimension": "dimension", "metric": "topnmetric", "granularity": "granularity", "filter": "filter",
               "aggregations": "aggregation", "postAggregations": "postagg"}

    @classmethod
    def _decode(cls, d):
        d = dict(d)
        if isinstance(d.get("dimension"), str):
            d["dimension"] = {"type": "default", "dimension": d["dimension"], "outputName": d["dimension"]}
        if isinstance(d.get("metric"), str):
            d["metric"] = {"type": "numeric", "metric": d["metric"]}
        return QuerySpec._decode.__func__(cls, d)


@_register("query", "search")
@dataclass
class SearchQuerySpec(QuerySpec, _Decodable):
    dataSource: str
    intervals: List[str]
    granularity: Granularity = field(default_factory=lambda: Granularity("all"))
    filter: Optional[Any] = None
    searchDimensions: List[str] = field(default_factory=list)
    query: Optional[SearchQueryQuerySpec] = None
    limit: int = 2 ** 31 - 1
    sort: Optional[Dict[str, str]] = None
    context: Optional[QuerySpecContext] = None
    queryType: str = "search"
    _nested = {"granularity": "granularity", "filter": "filter", "query": "searchquery"}

    @classmethod
    def _decode(cls, d):
        return QuerySpec._decode.__func__(cls, d)


@_register("query", "select")
@dataclass
class SelectSpec(QuerySpec, _Decodable):
    dataSource: str
    dimensions: List[str]
    metrics: List[str]
    filter: Optional[Any] = None
    pagingSpec: PagingSpec = field(default_factory=PagingSpec)
    intervals: List[str] = field(default_factory=list)
    descending: bool = False
    granularity: Granularity = field(default_factory=lambda: Granularity("all"))
    context: Optional[QuerySpecContext] = None
    queryType: str = "select"
    _nested = {"filter": "filter", "pagingSpec": "paging", "granularity": "granularity"}

    @classmethod
    def _decode(cls, d):
        return QuerySpec._decode.__func__(cls, d)


@dataclass
class DummyQuerySpec(QuerySpec, _Decodable):
    """Test stub (reference 1103-1127)."""
    dataSource: str = "dummy"
    intervals: List[str] = field(default_factory=list)
    queryType: str = "dummy"


_BY_CLASS["DummyQuerySpec"] = DummyQuerySpec
# aliases used by the reference's jsonClass hints
_BY_CLASS["GroupByQuerySpecWithSegIntervals"] = GroupByQuerySpec
_BY_CLASS["TimeSeriesQuerySpecWithSegIntervals"] = TimeSeriesQuerySpec
_BY_CLASS["TopNQuerySpecWithSegIntervals"] = TopNQuerySpec
_BY_CLASS["SearchQuerySpecWithSegIntervals"] = SearchQuerySpec
_BY_CLASS["SelectSpecWithIntervals"] = SelectSpec
_BY_CLASS["SelectSpecWithSegmentIntervals"] = SelectSpec


def query_from_json(s: Union[str, Dict[str, Any]]) -> QuerySpec:
    return from_json(s, "query")


def walk_filter(f, fn):
    """Pre-order visit of a filter tree."""
    if f is None:
        return
    fn(f)
    if isinstance(f, LogicalFilterSpec):
        for c in f.fields:
            walk_filter(c, fn)
    elif isinstance(f, NotFilterSpec):
        walk_filter(f.field, fn)
