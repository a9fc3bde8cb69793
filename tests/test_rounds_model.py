"""CPU checks of tests/rounds_model.py, the host model of gdsm_rounds' page-data side that
tests/test_gpu_rounds_data.py compares the device with: for every trace generator and every
prefix, the model's stream applied by the C oracle reproduces the model's home copy, the stream is
empty exactly when nothing changed, and the generators stay inside gdsm_rounds' contract and hold
the cases they are there for (no device)."""
import numpy as np
import pytest

from oracle import oracle
from tests import rounds_model as rm

GENERATORS = {"edges": rm.edges_trace, "hand-off": rm.handoff_trace,
              "sizes-small": rm.sizes_small_trace, "sizes-large": rm.sizes_large_trace}


@pytest.fixture(scope="module", params=list(GENERATORS))
def trace(request):
    return GENERATORS[request.param]()


def test_generators_stay_inside_the_contract(trace):
    assert rm.contract_violations(trace) == []


def test_model_stream_reproduces_the_home_copy_at_every_prefix(trace):
    """Round by round: oracle.apply of the round's stream onto the pre-round REPLICA (at the
    round's home pages) gives the model's REPLICA; the stream is empty exactly when no listed page
    changed; TWIN == CURRENT on the listed pages afterwards; pages no entry lists keep TWIN and
    REPLICA; CURRENT changes only where a descriptor lies."""
    twin0, rep0, cur0 = trace.twin.copy(), trace.rep.copy(), trace.cur.copy()
    for r, st in enumerate(rm.replay(trace)):
        rd = trace.rounds[r]
        ids = np.asarray(rd.ids, np.int64)
        assert len(st.rec_off) == len(ids) + 1 and int(st.rec_off[0]) == 0
        assert int(st.rec_off[-1]) == len(st.data)
        changed = bool((twin0[ids] != st.cur[ids]).any()) if len(ids) else False
        assert (len(st.data) > 0) == changed, r
        want = rep0.copy()
        if len(ids):
            assert oracle.apply(want, st.rec_off, st.data, rd.home) == 0
        assert np.array_equal(want, st.rep), r
        assert np.array_equal(st.twin[ids], st.cur[ids]), r
        rest = np.setdiff1d(np.arange(trace.n_pages), ids)
        assert np.array_equal(st.twin[rest], twin0[rest]), r
        rest_h = np.setdiff1d(np.arange(trace.n_pages), rd.home)
        assert np.array_equal(st.rep[rest_h], rep0[rest_h]), r
        written = np.zeros(trace.n_pages * rm.PAGE, bool)
        for dst, _, nb in rd.desc:
            written[dst:dst + nb] = True
        assert not (st.cur.reshape(-1) != cur0.reshape(-1))[~written].any(), r
        twin0, rep0, cur0 = st.twin.copy(), st.rep.copy(), st.cur.copy()


def test_model_prefix_equals_the_replay():
    t = rm.edges_trace()
    for k, st in enumerate(rm.replay(t), 1):
        m = rm.model(t, k)
        for a, b in zip((m.twin, m.cur, m.rep, m.rec_off, m.data),
                        (st.twin, st.cur, st.rep, st.rec_off, st.data)):
            assert np.array_equal(a, b), k


def test_descriptor_masks_change_exactly_the_masked_bytes():
    b = rm.TraceBuilder.fresh("t", 2, seed=1)
    before = b.now.copy()
    b.write(64, 32, [0, 5, 31], pad=True)
    b.write(4096 + 8, 8)
    assert np.flatnonzero(b.now != before).tolist() == [64, 69, 95]
    b.release([0, 1], [1, 0])
    t = b.build()
    assert rm.contract_violations(t) == []
    (dst, so, nb), _ = t.rounds[0].desc
    assert (dst, so, nb) == (64, 8, 32) and np.array_equal(t.src[so:so + nb], b.now[64:96])


def test_contract_check_sees_each_violation():
    def one(ids, desc, home=None):
        b = rm.TraceBuilder.fresh("t", 4, seed=2)
        t = b.build()
        t.src = np.zeros(4096, np.uint8)
        t.rounds = [rm.Round(np.array(ids, np.uint32),
                             np.array(ids if home is None else home, np.uint32), desc)]
        return rm.contract_violations(t)
    assert one([1], [(4096, 0, 64)]) == []
    assert one([1], [(4100, 0, 64)])          # misaligned
    assert one([1], [(4096, 0, 64), (4152, 64, 16)])  # overlap in one 8-B word
    assert one([1], [(8192, 0, 8)])           # a write on a page not released
    assert one([1, 1], [])                    # a page listed twice
    assert one([4], [])                       # outside the arenas
    assert one([1], [], home=[9])
    assert one(list(range(4)) * 513, [])      # 2052 pages


def test_edges_trace_holds_its_cases():
    t = rm.edges_trace()
    P = rm.PAGE
    assert len(t.rounds) == 8 and max(len(r.ids) for r in t.rounds) == 6
    assert [r for r in range(8) if not len(t.rounds[r].ids)] == [0, 3, 7]  # first, middle, last
    listed = np.unique(np.concatenate([r.ids for r in t.rounds]))
    for p in (22, 23):  # dirty and never released
        assert p not in listed and (t.twin[p] != t.cur[p]).any()
    sts = [rm.model(t, k) for k in range(1, 9)]
    size = lambda k, p: int(np.diff(sts[k].rec_off)[list(t.rounds[k].ids).index(p)])  # noqa: E731
    assert size(1, 3) == 0 and size(1, 9) == 0          # clean: no descriptor / bytes equal TWIN
    assert size(1, 4) > 0                               # dirty before the call, no descriptor
    assert any(nb == 0 for _, _, nb in t.rounds[1].desc)
    halves = [(d % 16, nb) for d, _, nb in t.rounds[1].desc]
    assert (8, 8) in halves and (0, 8) in halves and (8, 16) in halves
    assert sum(d // P == 20 for d, _, _ in t.rounds[1].desc) == 4
    assert any(d // P + 2 == (d + nb - 1) // P for d, _, nb in t.rounds[2].desc)
    ch = sts[2].cur[11] != sts[1].cur[11]
    for e in (1024, 2048, 3072):                        # runs across the quarter edges
        assert ch[e - 1] and ch[e]
    assert ch[0] and ch[P - 1]
    assert size(4, 12) == 4 + 4 + P                     # every byte: one run
    assert size(4, 13) == rm.MAX_RECORD == 4 + 4 * 2048 + 2048
    assert t.rounds[4].home[2] == t.rounds[4].home[3]   # two view pages, one home page
    assert len(sts[7].rec_off) == 1 and len(sts[7].data) == 0
    assert all((np.asarray(r.home) != np.asarray(r.ids)).all() for r in t.rounds)


def test_handoff_trace_rotates_the_list_and_touches_the_previous_word():
    t = rm.handoff_trace()
    assert len(t.rounds) == 300
    assert all(sorted(r.ids) == sorted(rm.HANDOFF_IDS) for r in t.rounds)
    assert [int(t.rounds[r].ids[0]) for r in range(4)] == [2, 5, 7, 2]
    for r in (1, 2, 299):
        d0 = {d // rm.PAGE: d % rm.PAGE for d, _, _ in t.rounds[r - 1].desc}
        for d, _, nb in t.rounds[r].desc:
            assert nb == 16 and d % rm.PAGE + 8 == d0[d // rm.PAGE] + (16 if r > 1 else 8)


def test_sizes_traces_have_the_issue_sizes_and_densities():
    for t, sizes in ((rm.sizes_small_trace(), rm.SMALL_SIZES),):
        assert tuple(len(r.ids) for r in t.rounds) == sizes
    t = rm.sizes_large_trace()
    assert tuple(len(r.ids) for r in t.rounds) == rm.LARGE_SIZES == (1, 33, 0, 257, 32, 2048, 5, 256)
    assert t.n_pages == 4096
    sizes = np.diff(rm.model(t, 6).rec_off)
    assert (sizes == 0).any() and (sizes == rm.MAX_RECORD).any() and (sizes == 4 + 4 + 4096).any()
    per_page = np.bincount(np.array([d // rm.PAGE for d, _, _ in t.rounds[5].desc]),
                           minlength=4096)[t.rounds[5].ids]
    assert set(per_page.tolist()) == {0, 1, 2, 3}
