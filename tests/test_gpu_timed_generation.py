"""-m gpu: timed generation (include/composer_hip.h, "timed generation") against its host restatement
`composer_amd.grammar.TimedRules`, with the method of tests/test_gpu_event_grammar.py: both chains are stepped one id at a time,
every id must equal cmp_k_sample_ex on the row masked by the host's ban set of that draw, and after every id the device's grammar
state and budget state must equal the host fold.  Both sides of every comparison run the same device arithmetic on the same
values, so nothing is undecidable and nothing is skipped.

A random model rarely draws one of a few allowed shifts among 300 columns, so the runs that must show every phase use a static
vector that leaves few columns: every VELOCITY id, NOTE_ON outside six pitches and TIME_SHIFT above eight steps are banned.  Time
then moves about two steps per draw: a budget of 7 steps ends within the 20 ids the kv mode has room for, one of 130 steps ends
after about 70 ids, behind the first slides of the 32-position window.  Each run asserts the coverage it is there for.
"""
import ctypes as C

import numpy as np
import pytest
import yaml
from click.testing import CliRunner

from test_gpu_event_grammar import (KEEP_SMALL, MODES, ROW_PARAMS, V0, W_SMALL, begin, check_against_the_masked_rows, grammar, ptr,
                                    set_grammar, small_model)

pytestmark = pytest.mark.gpu

PITCHES6 = (48, 55, 60, 64, 67, 72)
TAIL = [48, 60, 67, 388]                       # three NOTE_ONs and SUSTAIN_ON (ids of the default layout): the end of every prompt
# (mode, budget in steps, ids to run)
RUNS = [("literal", 7, 24), ("kv", 7, 20), ("kv-slide", 7, 40), ("kv-slide", 130, 110)]


def few_columns(g):
    from composer_amd import grammar as G
    mask = np.zeros(g.vocab_size, bool)
    mask[256:288] = True                                                     # every VELOCITY id
    mask[g.note_on0:g.note_on0 + 128] = True
    mask[[g.note_on0 + p for p in PITCHES6]] = False
    mask[g.time_shift0 + 8:g.time_shift0 + g.time_shift_n] = True            # shifts of more than eight steps
    return G.ban_words(g.vocab_size, mask)


def prompts_for(B):
    """ragged (in kv-slide the rows slide at different steps), every row with some prompt time that the budget must not charge"""
    return [np.array([288 + b] * (2 * (B - 1 - b)) + TAIL, np.int32) for b in range(B)]


def set_budget(m, batched, steps, cap):
    from composer_amd import _lib
    _lib.check(m._lib.cmp_decode_budget(m._h, 1 if batched else 0, steps, cap), "cmp_decode_budget")


def sk(mode):
    return {"slide_keep": KEEP_SMALL} if mode == "kv-slide" else {}


def run_timed(m, batched, mode, prompts, prm, seed, tr, words, n):
    """Steps one id at a time.  Returns ids [B][n], the row each id was drawn from Z [B][n][V], the ban set [B][n][V], the phase
    and the steps left of each draw [B][n] (all from the host fold) and the final host states; asserts the device's grammar state
    and budget state against the host fold after every id."""
    from composer_amd import _lib
    g = tr.grammar
    V, B = m.vocab_size, len(prompts)
    Z = np.zeros((B, n, V), np.float32)
    Z[:, 0] = np.stack([m(p.reshape(1, -1))[0][0, -1] for p in prompts])      # the first id: the prompt's last position
    set_grammar(m, batched, g, words)
    set_budget(m, batched, tr.time_steps, tr.max_polyphony)
    begin(m, batched, prompts, mode, prm, seed)
    host = [tr.begin(p) for p in prompts]
    ids = np.zeros((B, n), np.int32)
    bans = np.zeros((B, n, V), bool)
    phases = np.zeros((B, n), np.int64)
    left = np.zeros((B, n), np.int64)
    one = np.zeros((B, 1), np.int32)
    zb = np.zeros((B, V), np.float32)
    for i in range(n):
        for b in range(B):
            bans[b, i], phases[b, i], left[b, i] = tr.banned(host[b], words), tr.phase(host[b]), host[b].steps_left
        if batched:
            _lib.check(m._lib.cmp_decode_batch_steps(m._h, 1, ptr(one)), "batch_steps")
            if i >= 1:
                _lib.check(m._lib.cmp_decode_batch_logits_get(m._h, ptr(zb)), "batch_logits")
        else:
            _lib.check(m._lib.cmp_decode_steps(m._h, 1, ptr(one)), "steps")
            if i >= 1:
                _lib.check(m._lib.cmp_decode_logits_get(m._h, ptr(zb)), "logits")
        ids[:, i] = one[:, 0]
        if i >= 1:
            Z[:, i] = zb
        for b in range(B):
            tr.step(host[b], ids[b, i])
            dev = m.decode_grammar_state(batched=batched, row=b)
            assert dev == host[b].g, (mode, batched, b, i, dev, host[b])
            bs = m.decode_budget_state(batched=batched, row=b)
            assert bs == (host[b].steps_left, tr.phase(host[b]), host[b].done_at), (mode, batched, b, i, bs, host[b])
    return ids, Z, bans, phases, left, host


def coverage(g, ids, phases, left, host, plens, slide):
    """What the rows of one chain showed, any row counting: (a PLAY draw whose shift set the budget truncated below the eight
    shifts the static vector leaves, an ENDING of at least two draws, DONE followed by two fillers equal to time_shift0, a slide
    before DONE)."""
    from composer_amd import grammar as G
    trunc = ending = filler = slid = False
    for b in range(len(ids)):
        trunc |= bool(((phases[b] == G.PLAY) & (left[b] < 8)).any())
        ending |= int((phases[b] == G.ENDING).sum()) >= 2
        d = host[b].done_at
        if d >= 0:
            assert (phases[b, d:] == G.DONE).all() and (phases[b, :d] != G.DONE).all()
            assert (ids[b, d:] == g.time_shift0).all()                       # every id behind done_at is the filler
            filler |= len(ids[b]) - d >= 2
            # the id with index W - P + 1 is the first one drawn from a re-encode (the cache holds W positions)
            slid |= slide and d >= W_SMALL - plens[b] + 2
    return trunc, ending, filler, slid


def whole_call_checks(tr, p, out, ids_row, host_row, n):
    d = host_row.done_at
    assert out.tolist() == ids_row[:d if d >= 0 else n].tolist()
    if d >= 0:                                                               # prompt ++ result: a finished piece
        end = tr.grammar.fold(np.concatenate([p, out]))
        assert not end.sounding.any() and not end.pedal and end.time_steps == tr.t_end(p)


# ---------------------------------------------------------------- 1. stepwise identity and phase coverage, both chains
@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("mode, budget, n", RUNS)
def test_batch1_chain_draws_the_masked_rows_id_and_keeps_the_budget_state(mode, budget, n, graph, monkeypatch):
    from composer_amd import grammar as G
    monkeypatch.setenv("COMPOSER_NO_GRAPH", "0" if graph else "1")
    m = small_model()
    g = grammar()
    tr = G.TimedRules(g, budget, 0)
    words = few_columns(g)
    p = prompts_for(5)[0]                                                    # 12 ids, 8 steps of prompt time
    assert len(p) == 12 and tr.t_end(p) == 8 + budget
    seen = np.zeros(4, bool)
    for j, prm in enumerate([ROW_PARAMS[0], ROW_PARAMS[3], ROW_PARAMS[5]]):   # the last one greedy
        seed = 31 + j
        ids, Z, bans, phases, left, host = run_timed(m, False, mode, [p], [prm], seed, tr, words, n)
        check_against_the_masked_rows(ids, Z, bans, [prm], seed, (mode, budget, graph, prm))
        cov = coverage(g, ids, phases, left, host, [len(p)], mode == "kv-slide" and budget == 130)
        print("batch-1", mode, budget, graph, prm, "done_at", host[0].done_at, "coverage", cov)
        if prm[0] > 0:
            seen |= np.array(cov)
        # steps(n) in chunks equals n steps of one, cut at done_at
        out = m.generate(p, n, temperature=prm[0], top_k=prm[1], top_p=prm[2], mode=mode, seed=seed, grammar=g, banned_ids=words,
                         duration_steps=budget, **sk(mode))
        whole_call_checks(tr, p, out, ids[0], host[0], n)
        assert m.decode_budget_state()[2] == host[0].done_at
    assert seen[:3].all(), (mode, budget, seen)
    if mode == "kv-slide" and budget == 130:
        assert seen[3] and m.decode_slide_stats()[0] >= 1, seen
    m.close()


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("mode, budget, n", RUNS)
def test_batched_chain_draws_each_rows_masked_id_and_keeps_each_rows_budget_state(mode, budget, n, graph, monkeypatch):
    from composer_amd import grammar as G
    monkeypatch.setenv("COMPOSER_NO_GRAPH", "0" if graph else "1")
    m = small_model()
    g = grammar()
    tr = G.TimedRules(g, budget, 0)
    words = few_columns(g)
    B, seed = 5, 57
    prompts = prompts_for(B)
    assert sorted(len(p) for p in prompts) == [4, 6, 8, 10, 12]
    prm = [ROW_PARAMS[(b + 3) % len(ROW_PARAMS)] for b in range(B)]           # row 2 greedy
    assert [q[0] for q in prm].count(0.0) == 1
    ids, Z, bans, phases, left, host = run_timed(m, True, mode, prompts, prm, seed, tr, words, n)
    check_against_the_masked_rows(ids, Z, bans, prm, seed, (mode, budget, graph))
    cov = coverage(g, ids, phases, left, host, [len(p) for p in prompts], mode == "kv-slide" and budget == 130)
    print("batched", mode, budget, graph, "done_at", [h.done_at for h in host], "coverage", cov)
    assert all(cov[:3]), (mode, budget, cov)
    if mode == "kv-slide" and budget == 130:
        assert cov[3] and m.decode_slide_stats(batched=True)[0] >= 1, cov
    kw = dict(temperature=[q[0] for q in prm], top_k=[q[1] for q in prm], top_p=[q[2] for q in prm])
    out = m.generate_batch(prompts, n, mode=mode, seed=seed, grammar=g, banned_ids=words, duration_steps=budget, **kw, **sk(mode))
    assert isinstance(out, list) and len(out) == B
    for b in range(B):
        whole_call_checks(tr, prompts[b], out[b], ids[b], host[b], n)
    m.close()


# ---------------------------------------------------------------- 2. the polyphony cap
@pytest.mark.parametrize("batched", [False, True])
def test_the_cap_bans_every_note_on_while_three_pitches_sound(batched):
    """No time budget.  The few columns of the phase runs again, so that a release (three NOTE_OFFs among about twelve allowed
    columns) comes within a few draws and the NOTE_ONs of the three silent pitches come back."""
    from composer_amd import grammar as G
    m = small_model()
    g = grammar()
    tr = G.TimedRules(g, 0, 3)
    words = few_columns(g)
    n, seed = 20, 9
    prompts = [np.array([48, 60, 67], np.int32), np.array([300, 55, 64, 72, 289], np.int32)][:2 if batched else 1]
    prm = [ROW_PARAMS[0], ROW_PARAMS[3]][:len(prompts)]
    ids, Z, bans, phases, left, host = run_timed(m, batched, "kv", prompts, prm, seed, tr, words, n)
    check_against_the_masked_rows(ids, Z, bans, prm, seed, ("cap", batched))
    is_on = (ids >= g.note_on0) & (ids < g.note_on0 + 128)
    is_off = (ids >= g.note_off0) & (ids < g.note_off0 + 128)
    for b, p in enumerate(prompts):
        assert bans[b, 0, g.note_on0:g.note_on0 + 128].all()                 # three pitches sound at the first draw
        assert not g.banned(g.fold(p), words)[g.note_on0:g.note_on0 + 128].all()      # ... and only the cap bans the other three
        st = g.fold(p)
        for i in range(n):
            if is_on[b, i]:                                                  # no NOTE_ON until a NOTE_OFF made room
                assert int(st.sounding.sum()) < 3 and is_off[b, :i].any(), (b, i)
            g.step(st, ids[b, i])
            assert int(st.sounding.sum()) <= 3, (b, i)
        assert (phases[b] == G.PLAY).all() and host[b].done_at == -1
        assert m.decode_budget_state(batched, b) == (0, G.PLAY, -1)
    assert is_on.any()                                                       # ... and the cap lets go again
    m.close()


# ---------------------------------------------------------------- 3. whole calls
@pytest.mark.parametrize("B", [1, 5])
def test_a_batched_row_is_the_batch1_chain_with_seed_plus_b(B):
    from composer_amd import grammar as G
    m = small_model()
    g = grammar()
    tr = G.TimedRules(g, 40, 4)
    words = few_columns(g)
    prompts = prompts_for(5)[:B]
    prm = [ROW_PARAMS[b] for b in range(B)]                                  # (a greedy or top-5 row may never shift time)
    seed, cap = 19, 200
    kw = dict(temperature=[q[0] for q in prm], top_k=[q[1] for q in prm], top_p=[q[2] for q in prm])
    full = m.generate_batch(prompts, cap, mode="kv-slide", slide_keep=KEEP_SMALL, seed=seed, grammar=g, banned_ids=words,
                            duration_steps=40, max_polyphony=4, **kw)
    done = [m.decode_budget_state(True, b)[2] for b in range(B)]
    for b in range(B):
        t, k, q = prm[b]
        alone = m.generate(prompts[b], cap, temperature=t, top_k=k, top_p=q, mode="kv-slide", slide_keep=KEEP_SMALL, seed=seed + b,
                           grammar=g, banned_ids=words, duration_steps=40, max_polyphony=4)
        assert alone.tolist() == full[b].tolist(), b
        assert done[b] == len(full[b]) == m.decode_budget_state()[2] and 0 < done[b] < cap         # every row finished
        st = tr.fold(prompts[b], full[b])
        assert st.done_at == len(full[b]) and not st.g.sounding.any() and not st.g.pedal and st.g.time_steps == tr.t_end(prompts[b])
        on = (full[b] >= g.note_on0) & (full[b] < g.note_on0 + 128)
        assert set((full[b][on] - g.note_on0).tolist()) <= set(PITCHES6)
    assert len({len(r) for r in full}) > 1 or B == 1                         # rows of unequal length
    m.close()


def test_a_cap_of_six_events_comes_first():
    m = small_model()
    g = grammar()
    words = few_columns(g)                                                   # at most 8 steps per id: 130 steps need 17 ids or more
    p = prompts_for(5)[0]
    out = m.generate(p, 6, temperature=1.0, mode="kv", seed=3, grammar=g, banned_ids=words, duration_steps=130)
    assert len(out) == 6 and m.decode_budget_state()[2] == -1 and m.decode_budget_state()[0] >= 130 - 48
    outb = m.generate_batch([p, p[4:]], 6, temperature=1.0, mode="kv", seed=3, grammar=g, banned_ids=words, duration_steps=130)
    assert [len(r) for r in outb] == [6, 6] and outb[0].tolist() == out.tolist()
    assert [m.decode_budget_state(True, b)[2] for b in range(2)] == [-1, -1]
    m.close()


# ---------------------------------------------------------------- 4. off is off
@pytest.mark.parametrize("mode", MODES)
def test_off_after_a_timed_run_is_a_model_that_never_had_a_budget(mode):
    from composer_amd import _lib
    m, fresh = small_model(), small_model()
    g = grammar()
    words = few_columns(g)
    n = {"literal": 24, "kv": 20, "kv-slide": 3 * W_SMALL}[mode]
    prompts = prompts_for(5)
    prm = [ROW_PARAMS[(b + 3) % len(ROW_PARAMS)] for b in range(5)]
    kw = dict(temperature=[q[0] for q in prm], top_k=[q[1] for q in prm], top_p=[q[2] for q in prm])
    t, k, q = prm[0]
    base1 = fresh.generate(prompts[0], n, temperature=t, top_k=k, top_p=q, mode=mode, seed=11, grammar=g, banned_ids=words, **sk(mode))
    baseb = fresh.generate_batch(prompts, n, mode=mode, seed=11, grammar=g, banned_ids=words, **kw, **sk(mode))
    plain = fresh.generate(prompts[0], n, temperature=t, top_k=k, top_p=q, mode=mode, seed=11, **sk(mode))
    on1 = m.generate(prompts[0], n, temperature=t, top_k=k, top_p=q, mode=mode, seed=11, grammar=g, banned_ids=words,
                     duration_steps=7, max_polyphony=2, **sk(mode))
    onb = m.generate_batch(prompts, n, mode=mode, seed=11, grammar=g, banned_ids=words, duration_steps=7, max_polyphony=2, **kw, **sk(mode))
    assert on1.tolist() != base1[:len(on1)].tolist() or len(on1) < n          # the budget did change the run
    assert any(len(r) < n for r in onb)
    # cmp_decode_budget(m, ., 0, 0) itself, then the begin and step calls of the library: the grammar and the vector still in force
    for c in (0, 1):
        _lib.check(m._lib.cmp_decode_budget(m._h, c, 0, 0), "off")
    begin(m, False, [prompts[0]], mode, [prm[0]], 11)
    out = np.zeros(n, np.int32)
    _lib.check(m._lib.cmp_decode_steps(m._h, n, ptr(out)), "steps")
    assert out.tolist() == base1.tolist()
    assert m.decode_budget_state() == (0, 0, -1)
    begin(m, True, prompts, mode, prm, 11)
    outb = np.zeros((5, n), np.int32)
    _lib.check(m._lib.cmp_decode_batch_steps(m._h, n, ptr(outb)), "batch_steps")
    assert outb.tolist() == baseb.tolist()
    # ... and the wrapper without the new arguments, the grammar gone too: the plain sampler
    assert m.generate(prompts[0], n, temperature=t, top_k=k, top_p=q, mode=mode, seed=11, **sk(mode)).tolist() == plain.tolist()
    m.close(); fresh.close()


# ---------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_configuration_alone():
    from composer_amd import _lib, grammar as G
    m = small_model()
    lib, h = m._lib, m._h
    left, ph, da = C.c_int64(), C.c_int32(), C.c_int32()
    for c in (0, 1):
        assert lib.cmp_decode_budget_state(h, c, 0, C.byref(left), C.byref(ph), C.byref(da)) == -4          # before begin
    g = grammar()
    words = few_columns(g)
    p = prompts_for(5)[0]
    want1 = m.generate(p, 20, temperature=1.0, mode="kv", seed=2, grammar=g, banned_ids=words, duration_steps=7, max_polyphony=3)
    wantb = m.generate_batch([p, p[4:]], 20, temperature=1.0, mode="kv", seed=2, grammar=g, banned_ids=words, duration_steps=7,
                             max_polyphony=3)
    assert 0 < len(want1) < 20 and all(0 < len(r) < 20 for r in wantb)      # all three rows finished within the 20 ids
    assert lib.cmp_decode_budget_state(h, 0, 1, C.byref(left), C.byref(ph), C.byref(da)) == -1              # a bad row
    assert lib.cmp_decode_budget_state(h, 1, 2, C.byref(left), C.byref(ph), C.byref(da)) == -1
    assert lib.cmp_decode_budget_state(h, 1, -1, C.byref(left), C.byref(ph), C.byref(da)) == -1

    def decodes_as_before():
        begin(m, False, [p], "kv", [(1.0, 0, 1.0)], 2)
        out = np.zeros(32, np.int32)
        _lib.check(lib.cmp_decode_steps(h, 20, ptr(out)), "steps")
        assert out[:m.decode_budget_state()[2]].tolist() == want1.tolist()
        begin(m, True, [p, p[4:]], "kv", [(1.0, 0, 1.0)] * 2, 2)
        outb = np.zeros((2, 20), np.int32)
        _lib.check(lib.cmp_decode_batch_steps(h, 20, ptr(outb)), "batch_steps")
        for b in range(2):
            assert outb[b, :m.decode_budget_state(True, b)[2]].tolist() == wantb[b].tolist()

    # negative values: refused at the call
    for c in (0, 1):
        assert lib.cmp_decode_budget(h, c, -1, 0) == -1 and "time_steps" in _lib.last_error()
        assert lib.cmp_decode_budget(h, c, 5, -1) == -1 and "max_polyphony" in _lib.last_error()
    decodes_as_before()
    one = np.zeros((2, 1), np.int32)
    pb = np.zeros((2, len(p)), np.int32); pb[0] = p; pb[1, :len(p) - 4] = p[4:]
    lens = np.array([len(p), len(p) - 4], np.int32)
    # a budget without a layout, and a time budget over a static vector that bans time_shift0: refused at begin, before any device
    # work -- the decode in progress goes on
    no_step = G.ban_words(V0, np.flatnonzero(G.words_to_mask(V0, words)).tolist() + [g.time_shift0])
    for gg, ww, word in ((None, words, "layout"), (g, no_step, "time_shift0")):
        for c in (0, 1):
            set_grammar(m, c, gg, ww)
        assert lib.cmp_decode_begin(h, ptr(p), len(p), _lib.DECODE_KV, 1.0, 2) == -1 and word in _lib.last_error()
        assert lib.cmp_decode_batch_begin(h, ptr(pb), ptr(lens), 2, len(p), _lib.DECODE_KV, 1.0, 2) == -1 and word in _lib.last_error()
        _lib.check(lib.cmp_decode_steps(h, 1, ptr(one)), "steps")            # (the 21st id of the run above: a filler)
        assert one[0, 0] == g.time_shift0
        _lib.check(lib.cmp_decode_batch_steps(h, 1, ptr(one)), "batch_steps")
        assert one[:, 0].tolist() == [g.time_shift0] * 2
        for c in (0, 1):
            set_grammar(m, c, g, words)
        decodes_as_before()
    # the cap alone does not need the one-step shift
    for c in (0, 1):
        set_grammar(m, c, g, no_step)
        _lib.check(lib.cmp_decode_budget(h, c, 0, 3), "cap only")
    begin(m, False, [p], "kv", [(1.0, 0, 1.0)], 2)
    for c in (0, 1):
        set_grammar(m, c, g, words)
        _lib.check(lib.cmp_decode_budget(h, c, 7, 3), "back")
    # the Python wrapper refuses the same cases from its arguments, before it touches the configuration
    with pytest.raises(ValueError, match="grammar"):
        m.generate(p, 4, duration_steps=5)
    with pytest.raises(ValueError, match="grammar"):
        m.generate_batch([p], 4, max_polyphony=2)
    with pytest.raises(ValueError, match="duration_steps"):
        m.generate(p, 4, grammar=g, duration_steps=0)
    with pytest.raises(ValueError, match="max_polyphony"):
        m.generate(p, 4, grammar=g, max_polyphony=-1)
    with pytest.raises(ValueError, match="TIME_SHIFT"):
        m.generate(p, 4, grammar=g, banned_ids=no_step, duration_steps=5)
    decodes_as_before()
    m.close()


# ---------------------------------------------------------------- 6. CLI
def test_cli_duration_and_max_polyphony(tmp_path):
    from composer_amd import cli, checkpoint as ckpt, dataset as D, grammar as G
    cfg = yaml.safe_load(open(cli.get_default_config()))
    mc = cfg["transformer"]["model"]
    mc.update({"window_size": 32, "embedding_size": 64, "decoder_layers_count": 2, "attention_head_count": 4,
               "attention_dropout_rate": 0.0, "residual_dropout_rate": 0.0})
    cfg["transformer"]["runtime"] = {"dtype": "fp32", "seed": 3}
    run = tmp_path / "run"
    run.mkdir()
    (run / "config.yml").write_text(yaml.safe_dump(cfg))
    model, _ = cli.create_model(cli.ModelType.TRANSFORMER, cli.get_config_from_restoredir(run), dtype="fp32")
    ckpt.CheckpointManager(str(run)).save(model.state_dict(), {"step": 1})
    model.close()
    g = grammar(0)
    prompt = [60, 300, 388, 64]
    res = CliRunner().invoke(cli.cli, ["generate", "transformer", str(run), str(tmp_path / "out.data"), "--prompt-ids", "60,300,388,64",
                                       "--duration", "1.5", "--max-polyphony", "4", "--num-samples", "3", "--decode-mode", "kv-slide"],
                             catch_exceptions=False)
    assert res.exit_code == 0, res.output
    assert "150 steps" in res.stderr and res.stderr.count("finished yes") == 3 and "finished no" not in res.stderr
    t0 = g.fold(prompt).time_steps
    rows = []
    for i in range(3):
        got, _ = D.read_data_file(tmp_path / ("out-%d.data" % i))
        got = got.astype(np.int64)
        assert got[:4].tolist() == prompt and 4 < len(got) < 4 + 1024
        st = g.fold(prompt)
        for e in got[4:]:
            g.step(st, e)
            assert int(st.sounding.sum()) <= 4
        assert not st.sounding.any() and not st.pedal and st.time_steps == t0 + 150
        assert "sample %d: %d events, 1.500 s, finished yes" % (i, len(got) - 4) in res.stderr
        rows.append(got.tolist())
    assert rows[0] != rows[1]
    # --keep-best scores the prompt plus each row's own ids (rows of unequal length); one sample alone goes through the batch-1 chain
    res = CliRunner().invoke(cli.cli, ["generate", "transformer", str(run), str(tmp_path / "kb.data"), "--prompt-ids", "60,300,388,64",
                                       "--duration", "0.3", "--num-samples", "3", "--keep-best", "1", "--decode-mode", "kv-slide"],
                             catch_exceptions=False)
    assert res.exit_code == 0, res.output
    assert res.stderr.count("mean log-probability") == 3 and "sample 0: " in res.stderr and "sample 1: " not in res.stderr
    res = CliRunner().invoke(cli.cli, ["generate", "transformer", str(run), str(tmp_path / "one.data"), "--prompt-ids", "60,300,388,64",
                                       "--duration", "0.3"], catch_exceptions=False)
    assert res.exit_code == 0 and "finished yes" in res.stderr, res.output
    for name in ("kb-0.data", "one.data"):
        got, _ = D.read_data_file(tmp_path / name)
        st = g.fold(got.astype(np.int64))
        assert not st.sounding.any() and not st.pedal and st.time_steps == t0 + 30, name
