"""LIKE / contains / fragment over a materialized string dictionary, matched by the HIP kernel
(ops/csrc/dict_match.hip) -- against plain Python per entry, then through SQL and a search query."""
import re
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import torch

from spark_druid_olap_amd.engine import dict_match
from spark_druid_olap_amd.engine.executor import Engine, _search_filter
from spark_druid_olap_amd.engine.lower import Lowerer
from spark_druid_olap_amd.query import spec as S
from spark_druid_olap_amd.segment.dictionary import Dictionary
from spark_druid_olap_amd.sql.functions import like_to_regex

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TILE = 48 * 1024
N = 4 * 256 + 37  # four full tiles and a ragged fifth: the last bitset word is partial

EDGE = ["", "a", "b", "%", "_", "\\", "a%b", "a%bc", "x_y", "a\\b", "line\nbreak", "aaab", "abab", "ab", "aXbXc",
        "abc", "abcabc", "xabc", "abcx", "bc", "xbc", "aab", "abb", "ABC", "aB", "Ab", "tick", "KIT", "I", "i",
        "\u0130stanbul", "5 \u212a", "é", "café", "cafés", "éé", "abéx", "日本",
        "日本語", "\U0001f600", "a\U0001f600", "ab\U0001f600ab", "é日", "aa", "éa",
        "m0400" + "ab" * (TILE // 2) + "c"]  # (longer than the LDS tile; sorts into the middle of a tile)


def _dictionary(has_null: bool) -> Dictionary:
    fill = [f"m{i:04d}" + "ab" * (i % 7) + "cX"[i % 2] * (i % 3) for i in range(N - len(EDGE))]
    d, _ = Dictionary.build(EDGE + fill + ([None] if has_null else []))
    assert len(d.values) == N and d.has_null == has_null
    ends = np.cumsum([len(v.encode()) for v in d.values])
    assert (ends % 16 == 0).any() and (ends % 16 == 1).any()  # on / one past a 16-byte heap boundary
    assert 0 < list(d.values).index(EDGE[-1]) % 256 < 255
    return d


@pytest.fixture(scope="module")
def dicts():
    return {h: _dictionary(h) for h in (False, True)}


def _device_mask(d, spec):
    """The id mask the lowerer derives for ``spec``, which the device must have matched."""
    ds = SimpleNamespace(dims={"name": SimpleNamespace(dictionary=d)}, metrics={}, device=DEV)
    low = Lowerer(ds, device_match=True)
    kind, _, mask = low._filter_ir(spec)
    assert kind == "ids" and low.dict_match_device == 1
    return mask


LIKES = ["abc", "abc%", "%abc", "%abc%", "a%b%c", "_bc%", "%_", "%", "", "__", "a\\%b%", "%\\_%", "%aab%", "%ab%ab",
         "%é_", "%" + "ab" * 100 + "d"]  # (the last: longer than every entry but one, still on the device)


@pytest.mark.parametrize("has_null", [False, True])
@pytest.mark.parametrize("pattern", LIKES)
def test_like_matches_python_regex(dicts, monkeypatch, pattern, has_null):
    monkeypatch.setattr(dict_match, "DEVICE_MIN_CARD", 0)
    d = dicts[has_null]
    rx = re.compile(like_to_regex(pattern)[1:-1], re.S)
    want = np.array([v is not None and rx.fullmatch(v) is not None for v in d.all_values()])
    for negated in (False, True):
        f = S.JavascriptFilterSpec("name", "function(x) { return true; }")
        f._pylike = (pattern, negated)
        exp = np.array([v is not None for v in d.all_values()]) & ~want if negated else want
        assert np.array_equal(_device_mask(d, f), exp), (pattern, negated)


@pytest.mark.parametrize("has_null", [False, True])
@pytest.mark.parametrize("needle", ["ab", "AB", "i", "k", "é"])
def test_contains_matches_python_in(dicts, monkeypatch, needle, has_null):
    monkeypatch.setattr(dict_match, "DEVICE_MIN_CARD", 0)
    d = dicts[has_null]
    vals = d.all_values()
    cs = S.ContainsFilterSpec("name", {"type": "contains", "value": needle, "caseSensitive": True})
    assert np.array_equal(_device_mask(d, cs), np.array([v is not None and needle in v for v in vals]))
    ci = S.ContainsFilterSpec("name", {"type": "insensitive_contains", "value": needle})
    want = np.array([v is not None and needle.lower() in v.lower() for v in vals])
    assert np.array_equal(_device_mask(d, ci), want)  # (U+0130 / the Kelvin sign: the flagged-entry recheck)


@pytest.mark.parametrize("has_null", [False, True])
@pytest.mark.parametrize("needles", [["ab"], ["i"], ["k"], ["é"], ["a", "B"]])
def test_fragment_matches_python_in(dicts, monkeypatch, needles, has_null):
    monkeypatch.setattr(dict_match, "DEVICE_MIN_CARD", 0)
    d = dicts[has_null]
    f = _search_filter("name", S.SearchQueryQuerySpec("fragment", values=needles))
    want = np.array([v is not None and all(x.lower() in v.lower() for x in needles) for v in d.all_values()])
    assert np.array_equal(_device_mask(d, f), want)


# ------------------------------------------------------------------ through the public interface
@pytest.fixture(scope="module")
def session():
    from spark_druid_olap_amd.segment.ingest import ingest
    from spark_druid_olap_amd.session import Session

    names = [v for v in EDGE[:-1] if v and "\n" not in v and "\\" not in v] + [f"n{i:03d}ab{'c' * (i % 2)}" for i in range(300)]
    rng = np.random.default_rng(7)
    n = 3000
    df = pd.DataFrame({"ts": pd.date_range("2016-01-01", periods=n, freq="h").strftime("%Y-%m-%dT%H:%M:%S"),
                       "name": rng.choice(np.array(names, dtype=object), n), "m": rng.integers(1, 100, n)})
    spec = {"type": "index", "spec": {"dataSchema": {
        "dataSource": "ev", "parser": {"type": "string", "parseSpec": {
            "format": "tsv", "timestampSpec": {"column": "ts", "format": "iso"}, "columns": ["ts", "name", "m"],
            "dimensionsSpec": {"dimensions": ["name"]}}},
        "metricsSpec": [{"type": "longSum", "name": "m", "fieldName": "m"}],
        "granularitySpec": {"type": "uniform", "segmentGranularity": "MONTH", "queryGranularity": "none",
                            "rollup": False, "intervals": ["2016-01-01/2016-12-31"]}}}}
    s = Session(engine=Engine(use_native=True))
    s.register_datasource(ingest(spec, data=df, device="cuda"))
    s.register_table("evBase", df)
    s.sql('CREATE TABLE evd USING org.sparklinedata.druid OPTIONS (sourceDataframe "evBase", '
          'timeDimensionColumn "ts", druidDatasource "ev")')
    return s, df


@pytest.mark.parametrize("negated", [False, True])
def test_sql_like_is_matched_on_the_device(session, monkeypatch, negated):
    monkeypatch.setattr(dict_match, "DEVICE_MIN_CARD", 0)
    s, df = session
    q = s.sql(f"select count(*), sum(m) from evd where name {'not ' if negated else ''}like '%ab%c'")
    rows = q.collect()
    sel = df[df.name.str.fullmatch(".*ab.*c", flags=re.S) != negated]
    assert len(sel) and [tuple(int(x) for x in rows[0])] == [(len(sel), int(sel.m.sum()))]
    assert [st["stats"].get("dict_match_device") for st in q.last_stats["druid"]] == [1]


def test_search_query_is_matched_on_the_device(session, monkeypatch):
    monkeypatch.setattr(dict_match, "DEVICE_MIN_CARD", 0)
    s, df = session
    sq = S.SearchQuerySpec("ev", ["2016-01-01/2017-01-01"], searchDimensions=["name"],
                           query=S.SearchQueryQuerySpec("insensitive_contains", "K"))
    r = s.engine.execute(sq, s.catalog.cluster.get("ev"))
    want = {}
    for v in df.name:
        if "k" in v.lower():
            want[v] = want.get(v, 0) + 1
    assert "5 \u212a" in want and dict(zip(r.data["value"].tolist(), r.data["count"].tolist())) == want
    assert r.stats.get("dict_match_device") == 1
