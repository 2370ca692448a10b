"""Host checks of the event grammar (composer_amd/grammar.py, the restatement of include/composer_hip.h "event-grammar decoding"):
the events it calls ignored are exactly the ones NoteSequence.from_events drops, a stream drawn from the allowed ids has none, the
refusals of the contract are raised on the Python side, and pitch_range_bans sets the expected bits.  No GPU."""
import numpy as np
import pytest

from composer_amd import dataset as D
from composer_amd import grammar as G
from composer_amd.notes import NoteSequence

LAYOUTS = {"default": (10, 100, 32), "small": (10, 10, 4)}          # (time_step_increment, max_time_steps, velocity_bins)


def layout(name):
    tsi, mts, vb = LAYOUTS[name]
    vr = D.event_value_ranges(tsi, mts, vb)
    return G.EventGrammar.from_dataset_params(tsi, mts, vb), vr, D.event_ranges(vr), tsi, vb


def random_stream(g, rng, n):
    """ids that collide often: half of them NOTE_ON / NOTE_OFF / pedal events over six pitches, half anything"""
    pitches = rng.integers(0, 128, 6)
    out = rng.integers(0, g.vocab_size, n)
    for i in np.flatnonzero(rng.random(n) < 0.5):
        kind = rng.integers(0, 5)
        p = int(pitches[rng.integers(0, 6)])
        out[i] = (g.note_on0 + p, g.note_on0 + p, g.note_off0 + p, g.sustain_on, g.sustain_off)[kind]
    return out


def test_layouts_match_the_dataset():
    g = layout("default")[0]
    assert (g.vocab_size, g.note_on0, g.note_off0, g.time_shift0, g.time_shift_n, g.sustain_on, g.sustain_off) == \
        (390, 0, 128, 288, 100, 388, 389)
    s = layout("small")[0]
    assert (s.vocab_size, s.note_on0, s.note_off0, s.time_shift0, s.time_shift_n, s.sustain_on, s.sustain_off) == \
        (272, 0, 128, 260, 10, 270, 271)
    assert D.vocab_size(10, 10, 4) == 272


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_deleting_the_ignored_events_changes_no_note_and_no_pedal_period(name):
    g, vr, rg, tsi, vb = layout(name)
    rng = np.random.default_rng(7)
    total_ignored = 0
    for _ in range(1500):
        ids = random_stream(g, rng, int(rng.integers(1, 80)))
        ign = g.ignored_events(ids)
        total_ignored += len(ign)
        kept = np.delete(ids, ign)
        a = NoteSequence.from_events([D.id_to_event(int(i), rg, vr) for i in ids], tsi, vb)
        b = NoteSequence.from_events([D.id_to_event(int(i), rg, vr) for i in kept], tsi, vb)
        assert a.notes == b.notes and a.sustain_periods == b.sustain_periods
        assert g.ignored_events(kept) == []                          # what is left has no ignored event
        assert g.fold(ids) == g.fold(kept)                           # and the same state, time steps included
    assert total_ignored > 5000                                      # the streams did exercise the four cases


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_a_stream_drawn_from_the_allowed_ids_has_no_ignored_event(name):
    g = layout(name)[0]
    rng = np.random.default_rng(11)
    for _ in range(200):
        st, ids = G.GrammarState(), []
        for _ in range(120):
            ok = np.flatnonzero(~g.banned(st))
            assert np.isin(np.arange(g.time_shift0, g.time_shift0 + g.time_shift_n), ok).all()     # a TIME_SHIFT is never banned
            i = int(ok[rng.integers(0, len(ok))])
            assert g.step(st, i) is False
            ids.append(i)
        assert g.ignored_events(ids) == []
        assert g.fold(ids) == st


def test_banned_follows_the_rule_bits_and_the_static_vector():
    g0 = layout("default")[0]
    st = g0.fold([g0.note_on0 + 60, g0.sustain_on, g0.time_shift0 + 4, g0.time_shift0])
    assert np.flatnonzero(st.sounding).tolist() == [60] and st.pedal and st.time_steps == 6
    assert st.sounding_words().tolist() == [0, 1 << 28, 0, 0]
    for rules in range(8):
        g = G.EventGrammar(390, 0, 128, 288, 100, 388, 389, rules=rules)
        want = np.zeros(390, bool)
        if rules & G.NOTE_OFF_SOUNDING:
            want[128:256] = True
            want[128 + 60] = False
        if rules & G.NOTE_ON_SILENT:
            want[60] = True
        if rules & G.PEDAL:
            want[388] = True
        assert np.array_equal(g.banned(st), want), rules
        static = G.ban_words(390, [5, 300, 389])
        want[[5, 300, 389]] = True
        assert np.array_equal(g.banned(st, static), want), rules
    # no sustain ids: the PEDAL rule bans nothing
    g = G.EventGrammar(300, 0, 128, 256, 44, rules=G.ALL)
    assert g.banned(G.GrammarState()).sum() == 128


def test_every_refusal_of_the_contract_is_raised():
    ok = dict(vocab_size=390, note_on0=0, note_off0=128, time_shift0=288, time_shift_n=100, sustain_on=388, sustain_off=389)
    G.EventGrammar(**ok)
    bad = [
        (dict(note_on0=300), "outside"),                     # a range outside [0, V)
        (dict(note_off0=-1), "outside"),
        (dict(time_shift0=300), "outside"),
        (dict(sustain_off=390), "outside"),
        (dict(note_off0=100), "overlap"),                    # overlapping ranges
        (dict(time_shift0=200), "overlap"),
        (dict(sustain_on=5), "overlap"),
        (dict(sustain_on=389), "overlap"),
        (dict(sustain_on=-1), "sustain"),                    # one sustain id without the other
        (dict(sustain_off=-1), "sustain"),
        (dict(time_shift_n=0), "time_shift_n"),
        (dict(rules=8), "rule"),                             # unknown rule bits
    ]
    for change, word in bad:
        with pytest.raises(ValueError, match=word):
            G.EventGrammar(**dict(ok, **change))
    g = G.EventGrammar(**ok)
    # a static vector that bans everything it must not
    with pytest.raises(ValueError, match="TIME_SHIFT"):
        G.check_static_bans(390, G.ban_words(390, np.arange(288, 388)), g)
    G.check_static_bans(390, G.ban_words(390, np.arange(288, 387)), g)
    G.check_static_bans(390, G.ban_words(390, np.arange(288, 388)), None)          # without a layout: any id will do
    with pytest.raises(ValueError, match="all 390"):
        G.check_static_bans(390, G.ban_words(390, np.ones(390, bool)), None)
    with pytest.raises(ValueError, match="outside"):
        G.ban_words(390, [390])
    with pytest.raises(ValueError, match="mask"):
        G.ban_words(390, np.zeros(391, bool))


def test_ban_words_and_pitch_range_bans_set_exactly_the_expected_bits():
    for name in sorted(LAYOUTS):
        g = layout(name)[0]
        V = g.vocab_size
        w = g.pitch_range_bans(48, 84)
        assert w.dtype == np.uint32 and w.shape == ((V + 31) // 32,)
        want = np.zeros(V, bool)
        want[g.note_on0:g.note_on0 + 48] = True
        want[g.note_on0 + 85:g.note_on0 + 128] = True
        assert np.array_equal(G.words_to_mask(V, w), want)
        for c in range(V):
            assert bool((int(w[c >> 5]) >> (c & 31)) & 1) == bool(want[c])
        assert not G.words_to_mask(V, g.pitch_range_bans(0, 127)).any()
        assert G.words_to_mask(V, g.pitch_range_bans(60, 60)).sum() == 127
        # the three spellings of a ban set give the same words; bits at or above V are dropped
        assert np.array_equal(G.ban_words(V, np.flatnonzero(want)), w) and np.array_equal(G.ban_words(V, want), w)
        full = np.full((V + 31) // 32, 0xFFFFFFFF, np.uint32)
        assert G.words_to_mask(V, G.ban_words(V, full)).all() and int(G.ban_words(V, full)[-1]) == (1 << (V & 31)) - 1
    for lo, hi in ((-1, 5), (5, 128), (70, 60)):
        with pytest.raises(ValueError, match="pitch range"):
            layout("default")[0].pitch_range_bans(lo, hi)
