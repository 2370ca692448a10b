"""-m gpu: the copy guard in both decode chains (include/composer_hip.h, "copy guard") against its host restatement
`composer_amd.novelty.copy_bans`, with the method of tests/test_gpu_event_grammar.py: a chain is stepped one id at a time, the row
each id was drawn from is read back, and the id must equal cmp_k_sample_ex on that row with the host's ban set of the draw at -inf
(copy bans OR grammar / budget bans in PLAY, the copy bans ignored in ENDING and DONE) -- same seed and draw counter.  Both sides
run the same device arithmetic on the same values: nothing is undecidable, nothing is skipped.  The per-row counter must equal the
host's sum after every id.

The model is the tiny one of the grammar tests (V 390, window 32, slide_keep 12), so kv-slide slides several times in a run.  A
random model does not reproduce a corpus by itself: every run first decodes unguarded and puts prompt ++ that output into the corpus
between stretches of noise, so that the guarded run, which starts out on the same ids, meets the rule at once; small max_copy values
(1, 2, 4) keep chance matches with the noise coming afterwards."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_event_grammar import (KEEP_SMALL, MODES, ROW_PARAMS, V0, W_SMALL, begin, check_against_the_masked_rows, grammar, ptr,
                                    set_grammar, small_model, steps_for)
from test_gpu_timed_generation import few_columns, set_budget

pytestmark = pytest.mark.gpu

VELOCITY = (256, 32)


def sk(mode):
    return {"slide_keep": KEEP_SMALL} if mode == "kv-slide" else {}


def gen_kw(prm):
    return dict(temperature=prm[0], top_k=prm[1], top_p=prm[2])


def corpus_of(seqs, rng, noise=60):
    """noise ++ seq ++ noise ++ seq ... as one piece per stretch of noise -> (ids uint16, starts)"""
    parts, starts, at = [], [], 0
    for s in list(seqs) + [None]:
        nz = rng.integers(0, V0, noise)
        starts.append(at)
        parts.append(nz)
        at += noise
        if s is not None:
            parts.append(np.asarray(s))
            at += len(s)
    return np.concatenate(parts).astype(np.uint16), starts


def make_corpus(seqs, rng, g):
    from composer_amd import novelty
    ids, starts = corpus_of(seqs, rng)
    return novelty.Corpus(ids, starts, None, g, VELOCITY)


def attach(m, batched, guard):
    from composer_amd import _lib
    if guard is None:
        return m._lib.cmp_decode_copy_guard(m._h, 1 if batched else 0, None, None)
    ds, o = guard.attach_args()
    return m._lib.cmp_decode_copy_guard(m._h, 1 if batched else 0, ds, C.byref(o))


def run_guarded(m, batched, mode, prompts, prm, seed, guard, g, words, n, tr=None):
    """Steps one id at a time under the guard.  Returns ids [B][n], the rows Z [B][n][V], the ban sets [B][n][V] (host), the
    host's banned_columns per row and the phases [B][n]; asserts the device counter against the host's after every id."""
    from composer_amd import _lib, grammar as G
    V, B = m.vocab_size, len(prompts)
    Z = np.zeros((B, n, V), np.float32)
    Z[:, 0] = np.stack([m(p.reshape(1, -1))[0][0, -1] for p in prompts])      # the first id: the prompt's last position
    set_grammar(m, batched, g, words)
    set_budget(m, batched, tr.time_steps if tr else 0, tr.max_polyphony if tr else 0)
    assert attach(m, batched, guard) == 0, _lib.last_error()
    begin(m, batched, prompts, mode, prm, seed)
    static = G.words_to_mask(V, words) if words is not None else np.zeros(V, bool)
    host = [tr.begin(p) if tr else (g.fold(p) if g is not None else None) for p in prompts]
    hist = [list(map(int, p)) for p in prompts]
    ids = np.zeros((B, n), np.int32)
    bans = np.zeros((B, n, V), bool)
    phases = np.zeros((B, n), np.int64)
    count = np.zeros(B, np.int64)
    one = np.zeros((B, 1), np.int32)
    zb = np.zeros((B, V), np.float32)
    for i in range(n):
        for b in range(B):
            if tr:
                other, phases[b, i] = tr.banned(host[b], words), tr.phase(host[b])
            else:
                other = g.banned(host[b], words) if g is not None else static
            if phases[b, i] == G.PLAY:
                copy = guard.bans(hist[b], V)
                count[b] += int((copy & ~static).sum())
                other = other | copy
            bans[b, i] = other
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
            hist[b].append(int(ids[b, i]))
            if tr:
                tr.step(host[b], ids[b, i])
            elif g is not None:
                g.step(host[b], ids[b, i])
            assert m.decode_copy_guard_state(batched, b) == count[b], (mode, batched, b, i, count[b])
    return ids, Z, bans, count, phases, host


def only_time_shifts_past(rep, seq, M, g):
    """every match of more than M events of a NoveltyReport consists of TIME_SHIFT events only from its (M + 1)-th event on"""
    seq = np.asarray(seq)
    for s in np.flatnonzero(rep.len > M):
        tail = seq[s + M:s + int(rep.len[s])]
        assert ((tail >= g.time_shift0) & (tail < g.time_shift0 + g.time_shift_n)).all(), (int(s), int(rep.len[s]), tail.tolist())


# ---------------------------------------------------------------- a. the test that fails without the feature
@pytest.mark.parametrize("batched", [False, True])
def test_a_guarded_decode_does_not_play_the_corpus_back(batched):
    """Seed 11 was not searched for: among 96 ids of a nearly flat 390-way distribution about 70 are no TIME_SHIFT, and the
    precondition below is asserted on the unguarded output itself, so the test cannot pass vacuously."""
    m = small_model()
    g = grammar(rules=0)
    M, n, seed = 8, 96, 11
    rng = np.random.default_rng(3)
    # prompts of at most M events: a longer prompt, itself in the corpus, would be a match of more than M events before any draw
    prompts = [rng.integers(0, V0, 8).astype(np.int32), rng.integers(0, V0, 5).astype(np.int32)][:2 if batched else 1]

    def decode(guard):
        if batched:
            out = m.generate_batch(prompts, n, temperature=1.0, mode="kv-slide", seed=seed, copy_guard=guard, **sk("kv-slide"))
            return [out[b] for b in range(len(prompts))]
        return [m.generate(prompts[0], n, temperature=1.0, mode="kv-slide", seed=seed, copy_guard=guard, **sk("kv-slide"))]
    S = decode(None)
    for p, s in zip(prompts, S):
        non_ts = ~((s >= g.time_shift0) & (s < g.time_shift0 + g.time_shift_n))
        assert int(non_ts[max(0, M - len(p)):].sum()) >= 8                 # draws with t >= M whose unguarded id the rule must ban
    corpus = make_corpus([np.concatenate([p, s]) for p, s in zip(prompts, S)], rng, g)
    try:
        # unguarded, the sample IS the corpus: the novelty check finds all of it
        rep = corpus.match([np.concatenate([prompts[0], S[0]])], min_match=M + 1)[0]
        assert rep.longest[0] == len(prompts[0]) + n
        guard = corpus.guard(M)
        out = decode(guard)
        assert m.decode_slide_stats(batched)[0] >= 1
        for b, (p, s, o) in enumerate(zip(prompts, S, out)):
            assert o.tolist() != s.tolist(), b
            assert m.decode_copy_guard_state(batched, b) > 0, b
            seq = np.concatenate([p, o])
            only_time_shifts_past(corpus.match([seq], min_match=M + 1)[0], seq, M, g)
            only_time_shifts_past(corpus.match_host([seq], min_match=M + 1)[0], seq, M, g)
    finally:
        m.close()
        corpus.close()


# ---------------------------------------------------------------- b. stepwise identity, both chains
B1_RUNS = [(ROW_PARAMS[0], 1, 0, False), (ROW_PARAMS[3], 2, 1, True), (ROW_PARAMS[5], 1, 2, False)]     # (sampling, M, N, fold); the last greedy


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_batch1_chain_draws_the_masked_rows_id(mode, graph, monkeypatch):
    monkeypatch.setenv("COMPOSER_NO_GRAPH", "0" if graph else "1")
    m = small_model()
    g = grammar()
    rng = np.random.default_rng(21)
    n, seed = steps_for(mode), 31
    total = 0
    for j, (prm, M, N, fold) in enumerate(B1_RUNS):
        p = rng.integers(0, V0, int(rng.integers(3, 13))).astype(np.int32)
        words = g.pitch_range_bans(30, 100) if j == 1 else None
        free = m.generate(p, n, mode=mode, seed=seed + j, grammar=g, banned_ids=words, **gen_kw(prm), **sk(mode))
        corpus = make_corpus([np.concatenate([p, free])], rng, g)
        guard = corpus.guard(M, transpose=N, ignore_velocity=fold)
        try:
            ids, Z, bans, count, _, _ = run_guarded(m, False, mode, [p], [prm], seed + j, guard, g, words, n)
            check_against_the_masked_rows(ids, Z, bans, [prm], seed + j, (mode, graph, prm, M, N))
            # (the greedy run of this flat model repeats one TIME_SHIFT id, which no copy rule bans: its ids may stay what they were)
            assert count[0] > 0 and (prm[0] == 0.0 or ids[0].tolist() != free.tolist()), (mode, j)
            total += int(count[0])
            # steps(n) equals n steps of one, and the Python wrapper is the same call
            out = m.generate(p, n, mode=mode, seed=seed + j, grammar=g, banned_ids=words, copy_guard=guard, **gen_kw(prm), **sk(mode))
            assert out.tolist() == ids[0].tolist(), (mode, graph, prm)
            assert m.decode_copy_guard_state() == count[0]
            if mode == "kv-slide":
                assert m.decode_slide_stats()[0] >= 3
        finally:
            attach(m, False, None)
            corpus.close()
    print("batch-1", mode, graph, "banned_columns", total)
    m.close()


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_batched_chain_draws_each_rows_masked_id(mode, graph, monkeypatch):
    monkeypatch.setenv("COMPOSER_NO_GRAPH", "0" if graph else "1")
    m = small_model()
    g = grammar()
    B, M = 5, 4
    rng = np.random.default_rng(105)
    n, seed = steps_for(mode), 57
    prompts = [rng.integers(0, V0, k).astype(np.int32) for k in (1, 3, 6, 9, 12)]      # ragged; rows 0 and 1 begin shorter than M
    prm = [ROW_PARAMS[(b + 3) % len(ROW_PARAMS)] for b in range(B)]
    words = g.pitch_range_bans(21, 108)
    kw = dict(temperature=[q[0] for q in prm], top_k=[q[1] for q in prm], top_p=[q[2] for q in prm])
    free = m.generate_batch(prompts, n, mode=mode, seed=seed, grammar=g, banned_ids=words, **kw, **sk(mode))
    corpus = make_corpus([np.concatenate([p, f]) for p, f in zip(prompts, free)], rng, g)
    guard = corpus.guard(M, transpose=1)
    try:
        ids, Z, bans, count, _, _ = run_guarded(m, True, mode, prompts, prm, seed, guard, g, words, n)
        check_against_the_masked_rows(ids, Z, bans, prm, seed, (mode, graph))
        assert all(count[b] > 0 for b in range(B) if prm[b][0] > 0), count       # (the greedy row repeats one TIME_SHIFT id)
        # a row shorter than M draws unguarded until its history holds M ids
        assert ids[0, :M - 1].tolist() == free[0, :M - 1].tolist() and ids[0].tolist() != free[0].tolist()
        out = m.generate_batch(prompts, n, mode=mode, seed=seed, grammar=g, banned_ids=words, copy_guard=guard, **kw, **sk(mode))
        assert out.tolist() == ids.tolist()
        assert [m.decode_copy_guard_state(True, b) for b in range(B)] == count.tolist()
        if mode == "kv-slide":
            assert m.decode_slide_stats(batched=True)[0] >= 3 * B
        # a row of the batch is the batch-1 chain with seed + b
        b = 3
        alone = m.generate(prompts[b], n, mode=mode, seed=seed + b, grammar=g, banned_ids=words, copy_guard=guard, **gen_kw(prm[b]), **sk(mode))
        assert alone.tolist() == ids[b].tolist() and m.decode_copy_guard_state() == count[b]
    finally:
        corpus.close()
    m.close()


# ---------------------------------------------------------------- c. with rules and a duration budget
@pytest.mark.parametrize("batched", [False, True])
def test_union_in_play_ignored_in_the_ending_and_the_sample_finishes(batched):
    from composer_amd import grammar as G
    m = small_model()
    g = grammar()
    tr = G.TimedRules(g, 130, 0)
    words = few_columns(g)
    n, seed, mode = 110, 57, "kv-slide"
    B = 3 if batched else 1
    prompts = [np.array([288 + b] * (2 * (B - 1 - b)) + [48, 60, 67, 388], np.int32) for b in range(B)]
    prm = [ROW_PARAMS[0], ROW_PARAMS[3], ROW_PARAMS[1]][:B]
    rng = np.random.default_rng(8)
    kw = dict(temperature=[q[0] for q in prm], top_k=[q[1] for q in prm], top_p=[q[2] for q in prm])
    if batched:
        free = m.generate_batch(prompts, n, mode=mode, seed=seed, grammar=g, banned_ids=words, duration_steps=130, **kw, **sk(mode))
    else:
        free = [m.generate(prompts[0], n, mode=mode, seed=seed, grammar=g, banned_ids=words, duration_steps=130, **gen_kw(prm[0]), **sk(mode))]
    corpus = make_corpus([np.concatenate([p, f]) for p, f in zip(prompts, free)], rng, g)
    guard = corpus.guard(1)                                                   # few columns are allowed: M = 1 bans often
    try:
        ids, Z, bans, count, phases, host = run_guarded(m, batched, mode, prompts, prm, seed, guard, g, words, n, tr)
        check_against_the_masked_rows(ids, Z, bans, prm, seed, ("timed", batched))
        assert (count > 0).all(), count
        for b in range(B):
            assert host[b].done_at >= 0 and m.decode_budget_state(batched, b)[2] == host[b].done_at      # the sample finished
            assert (phases[b] == G.ENDING).any() and (phases[b] == G.DONE).any()
            # a draw of the ENDING whose copy bans, had they counted, would have hit an allowed column: they were ignored
            h = list(map(int, prompts[b]))
            ignored = False
            for i in range(n):
                if phases[b, i] == G.ENDING:
                    ignored |= bool((guard.bans(h, V0) & ~bans[b, i]).any())
                h.append(int(ids[b, i]))
            print("timed", batched, b, "done_at", host[b].done_at, "an ENDING draw with ignored copy bans:", ignored)
    finally:
        corpus.close()
    m.close()


# ---------------------------------------------------------------- d. off is off
@pytest.mark.parametrize("mode", MODES)
def test_off_after_a_guarded_run_is_a_model_that_never_had_a_guard(mode):
    g = grammar(rules=0)
    rng = np.random.default_rng(5)
    n, seed = steps_for(mode), 13
    p = rng.integers(0, V0, 7).astype(np.int32)
    rows = [p, p[:2], rng.integers(0, V0, 11).astype(np.int32)]
    never = small_model()
    want1 = never.generate(p, n, mode=mode, seed=seed, **sk(mode))
    wantb = never.generate_batch(rows, n, mode=mode, seed=seed, **sk(mode))
    never.close()
    m = small_model()
    corpus = make_corpus([np.concatenate([p, want1])] + [np.concatenate([r, w]) for r, w in zip(rows, wantb)], rng, g)
    guard = corpus.guard(2)
    try:
        on1 = m.generate(p, n, mode=mode, seed=seed, copy_guard=guard, **sk(mode))
        onb = m.generate_batch(rows, n, mode=mode, seed=seed, copy_guard=guard, **sk(mode))
        assert on1.tolist() != want1.tolist() and onb.tolist() != wantb.tolist()
        assert m.decode_copy_guard_state() > 0
        off1 = m.generate(p, n, mode=mode, seed=seed, **sk(mode))
        offb = m.generate_batch(rows, n, mode=mode, seed=seed, **sk(mode))
        assert off1.tolist() == want1.tolist() and offb.tolist() == wantb.tolist()
        assert m.decode_copy_guard_state() == 0 and m.decode_copy_guard_state(True, 2) == 0
        again = m.generate(p, n, mode=mode, seed=seed, copy_guard=guard, **sk(mode))      # ... and on again
        assert again.tolist() == on1.tolist()
        corpus.close()                               # the dataset is gone: the next guarded call opens it again and re-attaches
        assert m.generate(p, n, mode=mode, seed=seed, copy_guard=guard, **sk(mode)).tolist() == on1.tolist()
    finally:
        corpus.close()
    m.close()


def test_the_greedy_goldens_after_a_guard_was_detached():
    from test_gpu_model import decode_params, load_golden, make_model
    gd, cfg, params = load_golden("gA")
    m = make_model(cfg, decode_params(gd, cfg, params), "fp32")
    g = grammar(rules=0)
    n = len(gd["greedy_kv"])
    prompt = np.asarray(gd["prompt"], np.int32)
    corpus = make_corpus([np.concatenate([prompt, gd["greedy_kv"]])], np.random.default_rng(1), g)
    try:
        guarded = m.generate(prompt, n, temperature=0.0, mode="kv", copy_guard=corpus.guard(1))
        assert guarded.tolist() != gd["greedy_kv"].tolist()                     # greedy too: the guard is no filter
        for mode, key in (("kv", "greedy_kv"), ("literal", "greedy_literal")):
            assert m.generate(prompt, n, temperature=0.0, mode=mode).tolist() == gd[key].tolist()
            assert m.generate_batch([prompt], n, temperature=0.0, mode=mode)[0].tolist() == gd[key].tolist()
    finally:
        corpus.close()
    m.close()


# ---------------------------------------------------------------- e. refusals
def test_refused_calls_leave_a_decode_in_progress_untouched():
    from composer_amd import _lib, novelty
    m = small_model()
    g = grammar(rules=0)
    rng = np.random.default_rng(2)
    p = rng.integers(0, V0, 9).astype(np.int32)
    want = m.generate(p, 16, mode="kv", seed=5)
    corpus = make_corpus([np.concatenate([p, want])], rng, g)
    bare = novelty.Corpus(corpus.ids, corpus.starts)                          # a dataset without a layout
    bare._open()
    guard = corpus.guard(2)
    try:
        guarded = m.generate(p, 16, mode="kv", seed=5, copy_guard=guard)
        assert guarded.tolist() != want.tolist()
        # a guarded decode in progress: eight ids, then every refusal, then the other eight
        begin(m, False, [p], "kv", [(1.0, 0, 1.0)], 5)
        first = np.zeros(8, np.int32)
        _lib.check(m._lib.cmp_decode_steps(m._h, 8, ptr(first)), "steps")
        ds, _ = guard.attach_args()
        for handle, o in ((ds, (0, 0, 0, 0)), (ds, (65, 0, 0, 0)), (ds, (2, -1, 0, 0)), (ds, (2, 25, 0, 0)), (ds, (2, 0, 100, 40)),
                          (ds, (2, 0, 250, 10)), (ds, (2, 0, 65530, 10)), (bare._ds, (2, 0, 0, 0))):
            oo = _lib.CopyGuardOpts(*o)
            assert m._lib.cmp_decode_copy_guard(m._h, 0, handle, C.byref(oo)) == -1, o
            assert _lib.last_error()
        assert m._lib.cmp_decode_copy_guard(m._h, 0, ds, None) == -1
        n = C.c_int64(0)
        assert m._lib.cmp_decode_copy_guard_state(m._h, 0, 1, C.byref(n)) == -1                   # a bad row
        assert m._lib.cmp_decode_copy_guard_state(m._h, 1, 0, C.byref(n)) == -4                   # the batched chain has not begun
        rest = np.zeros(8, np.int32)
        _lib.check(m._lib.cmp_decode_steps(m._h, 8, ptr(rest)), "steps")
        assert np.concatenate([first, rest]).tolist() == guarded.tolist()
        # ... and the configuration is what it was: the next begin is guarded as before
        assert m.generate(p, 16, mode="kv", seed=5, copy_guard=guard).tolist() == guarded.tolist()
    finally:
        corpus.close()
        bare.close()
    m.close()
