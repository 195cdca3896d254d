"""What the device text matcher (engine/dict_match.py) declines keeps its host answer."""
import re
from types import SimpleNamespace

import numpy as np
import torch

from spark_druid_olap_amd.engine import dict_match
from spark_druid_olap_amd.engine.lower import Lowerer
from spark_druid_olap_amd.query import spec as S
from spark_druid_olap_amd.segment.dictionary import Dictionary, WordsDictionary
from spark_druid_olap_amd.segment.textheap import text_heap
from spark_druid_olap_amd.sql.functions import like_to_regex


def _like_mask(d, pattern, device_match):
    f = S.JavascriptFilterSpec("name", "function(x) { return true; }")
    f._pylike = (pattern, False)
    rx = re.compile(like_to_regex(pattern), re.S)
    f._pyvec = lambda vals: np.array([v is not None and rx.match(v) is not None for v in vals])
    ds = SimpleNamespace(dims={"name": SimpleNamespace(dictionary=d)}, metrics={}, device=torch.device("cpu"))
    low = Lowerer(ds, device_match=device_match)
    mask = low._filter_ir(f)[2]
    assert low.dict_match_device == 0
    return mask


def test_declined_predicates_keep_the_host_mask(monkeypatch):
    monkeypatch.setattr(dict_match, "DEVICE_MIN_CARD", 0)
    # nine '%'-separated pieces: one more than the pattern program holds
    pattern = "%a%b%c%d%e%f%g%h%i%"
    assert dict_match.compile_like(pattern) is None and dict_match.compile_like(pattern[:-2]) is not None
    assert dict_match.compile_like("%" + "x" * 257) is None
    d, _ = Dictionary.build(["abcdefghi", "xaxbxcxdxexfxgxhxix", "abcdefgh", "", None])
    got = _like_mask(d, pattern, True)
    assert got.tolist() == [False, False, False, True, True] and np.array_equal(got, _like_mask(d, pattern, False))
    # a lazy phrase dictionary has no text heap and answers through its own like_mask
    w = WordsDictionary(["almond", "blue", "green", "red"], 2, 12)
    assert text_heap(w, "cpu") is None
    got = _like_mask(w, "%green%", True)
    assert np.array_equal(got, w.like_mask("%green%")) and np.array_equal(got, _like_mask(w, "%green%", False))
    assert got.any() and not got.all()
