"""The structured NW corpus (tests/nw_corpus.py) on the CPU: its census models the reference's
alignment, and the corpus as a whole reaches the branches of the GPU trace that random strings do
not (tests/test_gpu_nw.py sends the same pairs to the device)."""
import pytest

from oracle import oracle
from tests import nw_corpus as nc


@pytest.fixture(scope="module")
def cen():
    return nc.censuses()


def test_corpus_is_deterministic_and_small():
    c = nc.corpus()
    assert len(c) == 26 and list(c)[:2] == ["head_a", "head_b"] and "periodic/3" in c
    nc.corpus.cache_clear()
    assert nc.corpus() == c
    assert all(len(a) < 2500 and len(b) < 2500 for a, b in c.values())


def test_census_alignment_is_the_oracles(cen):
    for name, (a, b) in nc.corpus().items():
        assert (cen[name].out1, cen[name].out2) == oracle.nw_diff(a, b), name


def test_every_rewalk_ends_somewhere(cen):
    for name, c in cen.items():
        assert c.rewalked == c.merged_first_row + c.merged_later + c.reached_top, name
        assert c.rewalked <= max(c.strips - 1, 0), name


def test_corpus_reaches_the_trace_branches(cen):
    """Floors over the whole corpus: conditions the GPU tests rely on, not measurements."""
    v = cen.values()
    assert any(c.merged_first_row >= 1 for c in v)
    assert any(c.merged_later >= 1 for c in v)
    assert any(c.reached_top >= 3 for c in v)
    assert any(c.col0_rows >= 300 for c in v)
    assert any(c.max_deviation >= 500 for c in v)
    assert any(c.strips >= 3 and c.row0_entry >= 500 for c in v)
    assert any(c.strips >= 3 and c.rewalked == 0 for c in v)


def test_named_pairs_do_what_they_are_named_for(cen):
    assert cen["allsame_sq"].strips == 3 and cen["allsame_sq"].rewalked == 0
    assert cen["head_b"].strips == 3 and cen["head_b"].row0_entry == nc.K
    assert cen["shift+"].max_deviation == nc.K and cen["shift-"].max_deviation == nc.K
    assert cen["head_a"].col0_rows >= 300
