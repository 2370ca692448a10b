"""CPU: composer_amd.novelty.copy_bans -- the host restatement of the copy guard's ban set (include/composer_hip.h, "copy guard")
that the GPU tests compare the scan kernel and both decode chains with -- against a triple loop over (p, k, j), on the shared cases
(tests/copy_guard_cases.py) and on hand cases for every clause of the contract.  Deliberately wrong restatements (the flags of
copy_guard_cases.brute_bans) show that each comparison the GPU tests rely on can fail: a start bit ignored, TIME_SHIFT not exempt,
clipping instead of "equals nothing", a window that reaches in front of position 0."""
import numpy as np
import pytest

import copy_guard_cases as cg
from composer_amd import novelty

L = cg.LAYOUT
ON, OFF, TS, A, B = L.note_on0, L.note_off0, L.time_shift0, 388, 389      # A / B: the pedal pair, tokens that are no note and no shift
V = cg.V


def bans(corpus, history, M, starts=None, N=0, vel=None):
    return novelty.copy_bans(np.asarray(corpus, np.uint16), starts, history, V, L, M, N, vel)


def cols(b):
    return sorted(int(v) for v in np.flatnonzero(b))


@pytest.mark.parametrize("name", cg.SMALL)
def test_copy_bans_equals_the_triple_loop(name):
    c = cg.case(name)
    ref = cg.reference(name)[0]
    some = False
    for b in range(c.B):
        want = cg.brute_bans(c.corpus, c.starts, c.hist[b, :c.lens[b]], V, c.layout, c.M, c.N, c.velocity)
        assert np.array_equal(ref[b], want), (name, b, cols(ref[b]), cols(want))
        some = some or want.any()
        if c.lens[b] < c.M:
            assert not want.any()
    assert some or c.n <= c.M, name                      # the case bans something: the comparison is not empty


def test_every_planted_window_bans_its_continuation():
    """The plants of the shared cases do what they were planted for (unless a start was put inside on purpose)."""
    hit = 0
    for name in cg.NAMES:
        c, ref = cg.case(name), cg.reference(name)[0]
        st = set(c.starts.tolist())
        for b, p, k in c.plants:
            if any(q in st for q in range(p - c.M + 1, p + 1)):
                continue
            cn = int(c.corpus[p])
            if TS <= cn < TS + L.time_shift_n:
                assert not ref[b, cn]
                continue
            v = cg.tok_under(cn, -k, L, None)            # the column that stands for c[p] under k
            if c.velocity and cg.VELOCITY[0] <= cn < sum(cg.VELOCITY):
                assert ref[b, cg.VELOCITY[0]:sum(cg.VELOCITY)].all(), (name, b, p)
            elif v is not None:
                assert ref[b, v], (name, b, p, k, v)
            hit += 1
    assert hit >= 20


def test_history_shorter_than_max_copy_bans_nothing():
    assert cols(bans([A, B, 60], [B], 2)) == []
    assert cols(bans([A, B, 60], [], 1)) == []
    assert cols(bans([A, B, 60], [A, B], 2)) == [60]


def test_the_window_never_reaches_in_front_of_position_0():
    corpus, h = [A, 60, 61, B], [B, A]                   # c[-1], c[0] read as a window would ban c[1]
    assert cols(bans(corpus, h, 2)) == []
    assert cols(cg.brute_bans(corpus, None, h, V, L, 2, wrap=True, ignore_starts=True)) == [60]
    assert cols(bans(corpus, [A], 1)) == [60]            # p = M = 1 is the first position


def test_piece_starts():
    corpus, h = [A, B, 60, 61], [A, B]
    assert cols(bans(corpus, h, 2)) == [60]
    assert cols(bans(corpus, h, 2, starts=[0, 1])) == []              # a start inside the window
    assert cols(bans(corpus, h, 2, starts=[0, 2])) == []              # the continuation begins a piece
    assert cols(cg.brute_bans(corpus, [0, 2], h, V, L, 2, ignore_starts=True)) == [60]
    corpus = [61, A, B, 60]
    assert cols(bans(corpus, h, 2, starts=[0, 1])) == [60]            # a start exactly at p - M: the window is the piece's beginning


def test_time_shift_continuations_are_never_banned():
    corpus, h = [A, B, TS + 2, A, B, 60], [A, B]
    assert cols(bans(corpus, h, 2)) == [60]
    assert cols(cg.brute_bans(corpus, None, h, V, L, 2, ts_exempt=False)) == [60, TS + 2]
    # ... not even through a velocity range that covers TIME_SHIFT ids
    got = bans([A, B, TS + 1], h, 2, vel=(TS, 4))
    assert cols(got) == []


def test_two_positions_ban_two_columns():
    assert cols(bans([A, B, 62, A, B, 60, A, B], [A, B], 2)) == [60, 62]


def test_transposition_equals_nothing_outside_the_pitch_range():
    # the history under k = +1 is NOTE_ON 127, NOTE_OFF 128: no such pitch, so it equals nothing -- clipping would invent a match
    corpus, h = [ON + 127, OFF + 127, B], [ON + 126, OFF + 127]
    assert cols(bans(corpus, h, 2, N=2)) == []
    assert cols(cg.brute_bans(corpus, None, h, V, L, 2, N=2, clip=True)) == [B]
    # a transposed copy whose continuation leaves 0 .. 127: k = -2 matches, the banned pitch would be 127 + 2
    corpus, h = [ON + 10, A, ON + 127], [ON + 12, A]
    assert cols(bans(corpus, h, 2, N=2)) == []
    assert cols(bans([ON + 10, A, ON + 100], h, 2, N=2)) == [ON + 102]
    assert cols(bans([ON + 10, A, OFF + 0], [ON + 8, A], 2, N=2)) == []       # k = +2: pitch 0 - 2
    assert cols(bans([ON + 10, A, ON + 100], [ON + 13, A], 2, N=2)) == []     # |k| = 3 > N


def test_a_window_without_a_note_bans_every_transposition_of_the_continuation():
    assert cols(bans([A, B, ON + 60], [A, B], 2, N=2)) == [ON + p for p in range(58, 63)]
    assert cols(bans([A, B, OFF + 1], [A, B], 2, N=2)) == [OFF + p for p in range(0, 4)]
    assert cols(bans([A, B, ON + 60], [A, B], 2, N=0)) == [ON + 60]
    assert cols(bans([A, B, A], [A, B], 2, N=2)) == [A]


def test_velocity_folding_bans_the_whole_range():
    v0, vn = cg.VELOCITY
    assert cols(bans([A, B, v0 + 4], [A, B], 2)) == [v0 + 4]
    assert cols(bans([A, B, v0 + 4], [A, B], 2, vel=cg.VELOCITY)) == list(range(v0, v0 + vn))
    assert cols(bans([A, v0 + 9, 60], [A, v0 + 1], 2)) == []
    assert cols(bans([A, v0 + 9, 60], [A, v0 + 1], 2, vel=cg.VELOCITY)) == [60]


def test_ids_that_equal_nothing():
    assert cols(bans([A, B, 60], [A, 70000], 1)) == []
    assert cols(bans([A, B, 60], [-1, A, B], 2)) == [60]              # only the last M ids are read


def test_refusals():
    ok = dict(corpus=np.asarray([A, B, 60], np.uint16), starts=None, history=[A, B], V=V, layout=L, max_copy=2)
    assert novelty.copy_bans(**ok).any()
    for kw in (dict(max_copy=0), dict(max_copy=65), dict(transpose=-1), dict(transpose=25), dict(layout=None),
               dict(velocity_range=(100, 40)), dict(velocity_range=(250, 10)), dict(velocity_range=(65530, 10)),
               dict(starts=[1]), dict(starts=[0, 3]), dict(starts=[0, 2, 1])):
        with pytest.raises(ValueError):
            novelty.copy_bans(**dict(ok, **kw))
    corpus = novelty.Corpus(np.asarray([A, B, 60], np.uint16), layout=L, velocity_range=cg.VELOCITY)
    g = corpus.guard(2, transpose=1, ignore_velocity=True)
    assert (g.max_copy, g.transpose) == (2, 1) and cols(g.bans([A, B], V)) == [59, 60, 61]
    for args in ((0,), (65,), (2, 25)):
        with pytest.raises(ValueError):
            corpus.guard(*args)
    with pytest.raises(ValueError):
        novelty.Corpus(np.asarray([A, B, 60], np.uint16), layout=L).guard(2, ignore_velocity=True)
    with pytest.raises(ValueError):
        novelty.Corpus(np.asarray([A, B, 60], np.uint16)).guard(2)            # no layout


def test_each_mistake_shows_on_the_shared_cases():
    """The wrong restatements differ from copy_bans somewhere on the shared cases, so the device comparison on the same cases would
    see a kernel that makes one of these mistakes."""
    seen = {"ignore_starts": False, "ts_exempt": False, "clip": False}
    for name in ("n257_m2", "n257_m16", "n257_m1", "n7_m1"):
        c, ref = cg.case(name), cg.reference(name)[0]
        for b in range(c.B):
            h = c.hist[b, :c.lens[b]]
            for flag, kw in (("ignore_starts", dict(ignore_starts=True)), ("ts_exempt", dict(ts_exempt=False)), ("clip", dict(clip=True))):
                if seen[flag] or (flag == "clip" and c.N == 0):
                    continue
                wrong = cg.brute_bans(c.corpus, c.starts, h, V, c.layout, c.M, c.N, c.velocity, **kw)
                seen[flag] = seen[flag] or not np.array_equal(wrong, ref[b])
    assert all(seen.values()), seen
