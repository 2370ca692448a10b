"""Timed generation on the host: `composer_amd.grammar.TimedRules`, the restatement of the contract in include/composer_hip.h
("timed generation") that the GPU tests compare the decode chains with, and the command line's refusals.  No GPU."""
import numpy as np
import pytest
from click.testing import CliRunner

from composer_amd import cli, dataset as D, grammar as G, notes as N

INC, MAXSTEPS, VBINS = 10, 100, 32               # the default dataset configuration: 390 ids, TIME_SHIFT 288 .. 387


def grammar(rules=G.ALL):
    return G.EventGrammar.from_dataset_params(INC, MAXSTEPS, VBINS, rules=rules)


def state(g, sounding=(), pedal=False, time_steps=0, t_end=0):
    s = np.zeros(128, bool)
    s[list(sounding)] = True
    return G.TimedState(G.GrammarState(s, pedal, time_steps), t_end)


def shifts(g, b):
    return b[g.time_shift0:g.time_shift0 + g.time_shift_n]


@pytest.mark.parametrize("left", [1, 7, 100, 101, 5000])
def test_play_truncates_the_time_shifts_at_t_end(left):
    g = grammar()
    tr = G.TimedRules(g, 9999, 0)
    st = state(g, sounding=[60], time_steps=40, t_end=40 + left)
    assert tr.phase(st) == G.PLAY and st.steps_left == left
    b = tr.banned(st)
    want = np.arange(g.time_shift_n) + 1 > left          # shift j (j + 1 steps) would pass t_end
    assert np.array_equal(shifts(g, b), want)
    assert (~shifts(g, b)).sum() == min(left, 100) and not b[g.time_shift0]
    if left >= 100:                                      # nothing truncated: the grammar's own ban set
        assert np.array_equal(b, g.banned(st.g))
    else:
        rest = b.copy()
        rest[g.time_shift0:g.time_shift0 + g.time_shift_n] = False
        assert np.array_equal(rest, g.banned(st.g))      # ... and nothing else changes


def test_no_time_budget_is_always_play_and_truncates_nothing():
    g = grammar()
    tr = G.TimedRules(g, 0, 3)
    assert tr.t_end([60, 300, 301]) == 0
    st = tr.begin([60, 300, 301])
    assert tr.phase(st) == G.PLAY and st.steps_left == 0 and np.array_equal(tr.banned(st), g.banned(st.g))


def test_polyphony_cap_at_n_and_n_minus_one():
    g = grammar(rules=0)
    tr = G.TimedRules(g, 0, 3)
    on = slice(g.note_on0, g.note_on0 + 128)
    assert not tr.banned(state(g, sounding=[60, 64]))[on].any()              # N - 1 sound: every NOTE_ON stays
    b = tr.banned(state(g, sounding=[60, 64, 67]))
    assert b[on].all() and b.sum() == 128                                    # N sound: no NOTE_ON, nothing else banned
    assert tr.banned(state(g, sounding=[1, 33, 65, 97]))[on].all()           # (one pitch in every word of the set)
    static = G.ban_words(g.vocab_size, [5, 200])
    bs = tr.banned(state(g, sounding=[60, 64, 67]), static)
    assert bs[5] and bs[200] and bs.sum() == 129                             # the static vector on top


def test_ending_releases_only_and_ignores_static_vector_and_rules():
    g = grammar()
    tr = G.TimedRules(g, 50, 2)
    st = state(g, sounding=[60, 100], pedal=True, time_steps=90, t_end=90)
    assert tr.phase(st) == G.ENDING
    allowed = {g.note_off0 + 60, g.note_off0 + 100, g.sustain_off}
    everything = G.ban_words(g.vocab_size, [i for i in range(g.vocab_size) if i != g.time_shift0])
    for static in (None, everything):                    # a static vector that bans all three releases changes nothing
        assert set(np.flatnonzero(~tr.banned(st, static)).tolist()) == allowed
    assert set(np.flatnonzero(~G.TimedRules(grammar(0), 50, 0).banned(st)).tolist()) == allowed       # nor do the rule bits
    st.g.pedal = False
    assert set(np.flatnonzero(~tr.banned(st)).tolist()) == allowed - {g.sustain_off}
    only_pedal = state(g, pedal=True, time_steps=90, t_end=90)
    assert tr.phase(only_pedal) == G.ENDING and np.flatnonzero(~tr.banned(only_pedal)).tolist() == [g.sustain_off]


def test_done_allows_the_filler_only_freezes_the_state_and_sets_done_at_once():
    g = grammar()
    tr = G.TimedRules(g, 7, 0)
    prompt = [60, g.time_shift0 + 4, g.sustain_on]                           # 5 steps of prompt time: not charged
    assert tr.t_end(prompt) == 12
    st = tr.begin(prompt)
    assert tr.phase(st) == G.PLAY and st.done_at == -1
    assert tr.step(st, g.time_shift0 + 6) == -1 and tr.phase(st) == G.ENDING and st.steps_left == 0
    assert tr.step(st, g.note_off0 + 60) == -1 and tr.phase(st) == G.ENDING
    assert tr.step(st, g.sustain_off) == 3 and tr.phase(st) == G.DONE
    assert np.flatnonzero(~tr.banned(st)).tolist() == [g.time_shift0]
    frozen = st.g.copy()
    for k in range(3):                                   # the filler does not move time, whatever id it is
        assert tr.step(st, g.time_shift0) == 3
        assert st.g == frozen and st.produced == 4 + k and tr.phase(st) == G.DONE
    got = tr.fold(prompt, [g.time_shift0 + 6, g.note_off0 + 60, g.sustain_off, g.time_shift0, g.time_shift0])
    assert got.g == frozen and got.done_at == 3 and got.produced == 5 and got.g.time_steps == 12


def test_refused_arguments():
    g = grammar()
    with pytest.raises(ValueError, match="time_steps"):
        G.TimedRules(g, -1, 0)
    with pytest.raises(ValueError, match="max_polyphony"):
        G.TimedRules(g, 0, -1)
    no_step = G.ban_words(g.vocab_size, [g.time_shift0])
    with pytest.raises(ValueError, match="TIME_SHIFT"):
        G.TimedRules(g, 5, 0).check_static_bans(no_step)
    G.TimedRules(g, 0, 4).check_static_bans(no_step)     # the cap alone needs no shift
    G.TimedRules(g, 5, 0).check_static_bans(G.ban_words(g.vocab_size, [g.time_shift0 + 1]))


def test_a_finished_stream_keeps_every_note_and_ends_at_t_end():
    """A walk through the ban sets (any allowed id, chosen by a fixed generator): converted with NoteSequence.from_events, every
    NOTE_ON the state accepted is a note, no note ends after t_end * time_step_increment ms and the last release is exactly there."""
    g = grammar()
    vr = D.event_value_ranges(INC, MAXSTEPS, VBINS)
    rg = D.event_ranges(vr)
    tr = G.TimedRules(g, 130, 4)
    prompt = [g.note_on0 + 60, g.time_shift0 + 9, g.sustain_on, g.note_on0 + 64]
    rng = np.random.default_rng(12)
    st = tr.begin(prompt)
    ids, accepted, endings = [], 2, 0                    # the prompt's two NOTE_ONs
    while st.done_at < 0:
        allowed = np.flatnonzero(~tr.banned(st))
        if tr.phase(st) == G.PLAY:                       # short shifts now and then: a few hundred events until t_end
            is_shift = (allowed >= g.time_shift0) & (allowed < g.time_shift0 + g.time_shift_n)
            allowed = allowed[is_shift][:4] if rng.random() < 0.3 else allowed[~is_shift]
        i = int(rng.choice(allowed))
        accepted += g.note_on0 <= i < g.note_on0 + 128   # (rules ALL: a NOTE_ON that is drawn is one the state accepts)
        assert int(st.g.sounding.sum()) <= 4
        endings += tr.phase(st) == G.ENDING
        tr.step(st, i)
        ids.append(i)
        assert len(ids) < 5000
    assert st.g.time_steps == st.t_end == 140 and not st.g.sounding.any() and not st.g.pedal and st.done_at == len(ids)
    seq = N.NoteSequence.from_events([D.id_to_event(i, rg, vr) for i in prompt + ids], INC, VBINS)
    end_ms = st.t_end * INC
    assert endings >= 2                                  # the precondition of "the last release is exactly there"
    assert len(seq.notes) == accepted and accepted > 2
    assert max(n.end for n in seq.notes) <= end_ms
    assert max([n.end for n in seq.notes] + [p.end for p in seq.sustain_periods]) == end_ms
    assert all(p.end is not None and p.end <= end_ms for p in seq.sustain_periods)
    # the same stream cut where an event count would have cut it loses what still sounds
    cut = N.NoteSequence.from_events([D.id_to_event(i, rg, vr) for i in prompt + ids[:len(ids) // 2]], INC, VBINS)
    assert len(cut.notes) <= len(seq.notes)


@pytest.mark.parametrize("args, word", [(["--duration", "0"], "--duration 0.0: SECONDS must be a number > 0"),
                                        (["--duration", "nan"], "--duration nan: SECONDS must be a number > 0"),
                                        (["--duration", "-1.5"], "--duration -1.5: SECONDS must be a number > 0"),
                                        (["--duration", "inf"], "--duration inf: SECONDS must be a number > 0"),
                                        (["--max-polyphony", "0"], "--max-polyphony 0: must be >= 1"),
                                        (["--max-polyphony", "-2"], "--max-polyphony -2: must be >= 1")])
def test_cli_refuses_bad_values_before_touching_a_device(args, word, tmp_path, monkeypatch):
    """`word` is the refusal's own text: a command line without these options answers "No such option" instead"""
    def no_device(*a, **k):
        raise AssertionError("a model was created for a command line that must be refused")
    monkeypatch.setattr(cli, "create_model", no_device)
    r = CliRunner().invoke(cli.cli, ["generate", "transformer", str(tmp_path), str(tmp_path / "out.mid"), "--prompt-ids", "60"] + args)
    assert r.exit_code == 2 and "Usage" in r.output and word in r.output
    assert not (tmp_path / "out.mid").exists()


def test_cli_help_names_the_options_and_length_keeps_its_default():
    h = CliRunner().invoke(cli.cli, ["generate", "--help"]).output
    assert "--duration" in h and "--max-polyphony" in h and "kv-slide" in h
    p = {o.name: o.default for o in cli.generate.params}
    assert p["generate_length"] == 1024 and p["duration"] is None and p["max_polyphony"] is None
