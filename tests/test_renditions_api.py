"""Renditions (several JPEGs of one decoded picture): the Python spec normaliser and the constants
shared with include/h2j.h.  No GPU."""
import os
import re

import pytest

import h2j

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spec_scalar_pair_dict():
    assert h2j.rendition_spec(0) == (0, 0, 0, 0, 0)
    assert h2j.rendition_spec(3) == (3, 0, 0, 0, 0)
    assert h2j.rendition_spec((50, 0)) == (0, 0, 50, 0, 0)
    assert h2j.rendition_spec((None, 40)) == (0, 0, 0, 40, 0)
    assert h2j.rendition_spec({}) == (0, 0, 0, 0, 0)
    assert h2j.rendition_spec({"scale": 1, "max_dim": 100}) == (1, 100, 0, 0, 0)
    assert h2j.rendition_spec({"fit": (62, 38), "stretch": True}) == (0, 0, 62, 38, h2j.FIT_STRETCH)
    assert h2j.rendition_spec({"fit": (62, None)}) == (0, 0, 62, 0, 0)
    # values are the engine's to judge (a rendition with invalid options fails alone)
    assert h2j.rendition_spec(7) == (7, 0, 0, 0, 0)


@pytest.mark.parametrize("bad", [True, "1", 1.5, None, (1, 2, 3), {"scales": 1}, {"fit": 5}])
def test_spec_rejects(bad):
    with pytest.raises(ValueError):
        h2j.rendition_spec(bad)


def test_one_list_for_every_item():
    specs = [0, 3, (50, 0), {"fit": (10, 10), "stretch": True}]
    exp = [(0, 0, 0, 0, 0), (3, 0, 0, 0, 0), (0, 0, 50, 0, 0), (0, 0, 10, 10, 1)]
    assert h2j.normalize_renditions(specs, 3) == [exp, exp, exp]
    assert h2j.normalize_renditions(specs, 0) == []
    assert h2j.normalize_renditions([2], 2) == [[(2, 0, 0, 0, 0)]] * 2
    # two ints in a list are two scales, not a fit
    assert h2j.normalize_renditions([0, 3], 1) == [[(0, 0, 0, 0, 0), (3, 0, 0, 0, 0)]]
    # a tuple pair is a fit
    assert h2j.normalize_renditions([(32, 32)], 1) == [[(0, 0, 32, 32, 0)]]


def test_per_item_lists():
    got = h2j.normalize_renditions([[0, 1], [2], [(50, 0), {"scale": 3}]], 3)
    assert got == [[(0, 0, 0, 0, 0), (1, 0, 0, 0, 0)], [(2, 0, 0, 0, 0)], [(0, 0, 50, 0, 0), (3, 0, 0, 0, 0)]]
    # per-item lists of two ints each stay lists of scales
    assert h2j.normalize_renditions([[0, 1], [2, 3]], 2) == [[(0, 0, 0, 0, 0), (1, 0, 0, 0, 0)],
                                                             [(2, 0, 0, 0, 0), (3, 0, 0, 0, 0)]]
    # the same as the shared form when every item has the same list
    assert h2j.normalize_renditions([[0, 3], [0, 3]], 2) == h2j.normalize_renditions([0, 3], 2)


def test_length_errors():
    with pytest.raises(ValueError):
        h2j.normalize_renditions([[0], [1]], 3)          # 2 per-item lists for 3 streams
    with pytest.raises(ValueError):
        h2j.normalize_renditions([[0], [1], [2]], 2)
    with pytest.raises(ValueError):
        h2j.normalize_renditions([], 2)                  # no rendition
    with pytest.raises(ValueError):
        h2j.normalize_renditions([[0], []], 2)
    with pytest.raises(ValueError):
        h2j.normalize_renditions(list(range(h2j.MAX_RENDITIONS + 1)), 1)
    with pytest.raises(ValueError):
        h2j.normalize_renditions([[0] * (h2j.MAX_RENDITIONS + 1)], 1)
    assert len(h2j.normalize_renditions([0] * h2j.MAX_RENDITIONS, 1)[0]) == h2j.MAX_RENDITIONS
    for bad in (None, 3, {"scale": 1}, [[0], 1]):
        with pytest.raises(ValueError):
            h2j.normalize_renditions(bad, 2)


def test_constants_match_header():
    src = open(os.path.join(ROOT, "include", "h2j.h")).read()
    m = re.search(r"#define\s+H2J_MAX_RENDITIONS\s+(\d+)", src)
    assert m and int(m.group(1)) == h2j.MAX_RENDITIONS
    m = re.search(r"#define\s+H2J_ERR_RENDITIONS\s+\((-\d+)\)", src)
    assert m and int(m.group(1)) == h2j.ERR_RENDITIONS
    assert h2j.STAT_KEYS[23:25] == ["renditions", "parsed"]
    assert re.search(r"\[23\] renditions", src) and re.search(r"\[24\] parsed", src)
