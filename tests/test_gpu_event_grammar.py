"""-m gpu: event-grammar decoding (include/composer_hip.h, "event-grammar decoding") against its host restatement
`composer_amd.grammar.EventGrammar`.

The contract of the draw: with N the ids banned at a step (the rules in the state of prompt ++ ids so far, ORed with the static
vector), the id equals, bit for bit, cmp_k_sample_ex on a copy of the logits row with the columns of N at -inf -- same
temperature, top_k, top_p, seed and draw counter.  Checked at kernel level (cmp_k_sample_banned, 10 000 draw counters) and in both
decode chains at every step, where the row is read back with cmp_decode_logits_get / cmp_decode_batch_logits_get and the device's
grammar state with cmp_decode_grammar_state.  Both sides of every comparison run the same device arithmetic on the same values, so
there is no undecidable top-p boundary and nothing is skipped.  The eager chain is selected with COMPOSER_NO_GRAPH=1 the way the
other decode tests select it (the variable is read by every begin call).
"""
import ctypes as C

import numpy as np
import pytest
import yaml
from click.testing import CliRunner

from test_sampling_truncation import round3_row

pytestmark = pytest.mark.gpu

V0 = 390
W_SMALL, KEEP_SMALL = 32, 12
MODES = ("literal", "kv", "kv-slide")
TEMPERATURES = (0.0, 0.7, 1.6)
KP = ((0, 1.0), (40, 1.0), (0, 0.9), (40, 0.9))
# per-row (temperature, top_k, top_p) of the batched chain, cycled over the rows (tests/test_gpu_sampling_truncation.py)
ROW_PARAMS = [(1.0, 0, 1.0), (0.7, 40, 1.0), (1.6, 0, 0.9), (1.0, 40, 0.9), (0.7, 0, 0.5), (0.0, 40, 0.9), (1.3, 5, 0.95)]


def gpu():
    import torch
    from composer_amd import _lib
    lib = _lib.load(); _lib.require_gpu()
    return torch, _lib, lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)


def grammar(rules=None, params=(10, 100, 32)):
    from composer_amd import grammar as G
    return G.EventGrammar.from_dataset_params(*params, rules=G.ALL if rules is None else rules)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def masked(z, ban):
    out = z.copy()
    out[ban] = -np.inf
    return out


def k_sample_ex(lib, _lib, stream, zd, V, t, k, p, seed, ctr0, n, out):
    _lib.check(lib.cmp_k_sample_ex(stream, C.c_void_p(zd.data_ptr()), V, t, k, p, seed, ctr0, n, C.c_void_p(out.data_ptr())))


# ---------------------------------------------------------------- 1. kernel level, bitwise
def kernel_row():
    z = round3_row(V0)
    z[[40, 41, 300]] = z.max() + 1.0                         # a three-way tie at the top
    return z


def ban_patterns(z):
    V = len(z)
    rng = np.random.default_rng(5)
    none = np.zeros(V, bool)
    note_off = none.copy(); note_off[128:256] = True
    all_but_one = np.ones(V, bool); all_but_one[301] = False
    top = none.copy(); top[[int(np.argmax(z)), 7, 199, 389]] = True           # the raw argmax (40, the lowest of the tie) is banned
    many = none.copy(); many[rng.permutation(V)[:V - 40 + 10]] = True         # more than V - top_k columns: 30 stay for top_k = 40
    return {"none": none, "every_note_off": note_off, "all_but_one": all_but_one, "raw_argmax": top, "more_than_v_minus_k": many}


@pytest.mark.parametrize("name", ["none", "every_note_off", "all_but_one", "raw_argmax", "more_than_v_minus_k"])
def test_k_sample_banned_equals_k_sample_ex_on_the_masked_row(name):
    from composer_amd import grammar as G
    torch, _lib, lib, stream = gpu()
    z = kernel_row()
    ban = ban_patterns(z)[name]
    V, n, seed = len(z), 10_000, 123
    zd = torch.from_numpy(z).cuda()
    md = torch.from_numpy(masked(z, ban)).cuda()
    wd = torch.from_numpy(G.ban_words(V, ban).view(np.int32)).cuda()
    got = torch.empty(n, dtype=torch.int32, device="cuda")
    want = torch.empty(n, dtype=torch.int32, device="cuda")
    allowed = np.flatnonzero(~ban)
    for t in TEMPERATURES:
        for k, p in KP:
            _lib.check(lib.cmp_k_sample_banned(stream, C.c_void_p(zd.data_ptr()), V, t, k, p, C.c_void_p(wd.data_ptr()), seed, 7, n,
                                               C.c_void_p(got.data_ptr())))
            k_sample_ex(lib, _lib, stream, md, V, t, k, p, seed, 7, n, want)
            torch.cuda.synchronize()
            g, w = got.cpu().numpy(), want.cpu().numpy()
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, (name, t, k, p, bad[:5], g[bad[:5]], w[bad[:5]])
            assert not ban[g].any(), (name, t, k, p)
            if name == "none":                               # nothing banned: the sampler on the row itself
                k_sample_ex(lib, _lib, stream, zd, V, t, k, p, seed, 7, n, want)
                torch.cuda.synchronize()
                assert np.array_equal(g, want.cpu().numpy()), (t, k, p)
            if t == 0.0:                                     # greedy: the argmax over the allowed columns, lowest index on ties
                assert (g == allowed[np.argmax(z[allowed])]).all(), (name, k, p, g[:4])
            if name == "all_but_one":
                assert (g == 301).all()
    if name == "raw_argmax":
        assert int(np.argmax(z)) == 40 and allowed[np.argmax(z[allowed])] == 41


def test_k_sample_banned_has_no_row_limit_with_the_filters_off():
    """V = 5000 > 4096: the ban predicate needs no LDS image of the row"""
    from composer_amd import grammar as G
    torch, _lib, lib, stream = gpu()
    V, n = 5000, 4000
    rng = np.random.default_rng(50)
    z = (rng.standard_normal(V) * 2.0).astype(np.float32)
    ban = rng.random(V) < 0.5
    ban[int(np.argmax(z))] = True
    zd = torch.from_numpy(z).cuda()
    md = torch.from_numpy(masked(z, ban)).cuda()
    wd = torch.from_numpy(G.ban_words(V, ban).view(np.int32)).cuda()
    got = torch.empty(n, dtype=torch.int32, device="cuda")
    want = torch.empty(n, dtype=torch.int32, device="cuda")
    allowed = np.flatnonzero(~ban)
    for t in (0.0, 0.7, 1.6):
        _lib.check(lib.cmp_k_sample_banned(stream, C.c_void_p(zd.data_ptr()), V, t, 0, 1.0, C.c_void_p(wd.data_ptr()), 9, 3, n,
                                           C.c_void_p(got.data_ptr())))
        k_sample_ex(lib, _lib, stream, md, V, t, 0, 1.0, 9, 3, n, want)
        torch.cuda.synchronize()
        g = got.cpu().numpy()
        assert np.array_equal(g, want.cpu().numpy()), t
        assert not ban[g].any()
        if t == 0.0:
            assert (g == allowed[np.argmax(z[allowed])]).all()
    # a filter on such a row is refused as before, naming the limit
    assert lib.cmp_k_sample_banned(stream, C.c_void_p(zd.data_ptr()), V, 1.0, 40, 1.0, C.c_void_p(wd.data_ptr()), 9, 3, n,
                                   C.c_void_p(got.data_ptr())) == -1
    assert "4096" in _lib.last_error()


# ---------------------------------------------------------------- 2. both chains, stepwise
def small_model(V=V0, W=W_SMALL, seed=4):
    from composer_amd.transformer import Transformer
    return Transformer(V, 64, W, 2, 4, attention_dropout_rate=0.0, residual_dropout_rate=0.0, dtype="fp32", seed=seed,
                       max_batch=1, max_seq=W)


def steps_for(mode):
    return {"literal": 24, "kv": 20, "kv-slide": 3 * W_SMALL}[mode]          # kv-slide: several slides of every row


def prompts_for(B, rng, V=V0):
    return [rng.integers(0, V, int(k)).astype(np.int32) for k in rng.integers(1, 13, B)]


def set_grammar(m, batched, g, words):
    from composer_amd import _lib
    cg = g.to_c() if g is not None else None
    _lib.check(m._lib.cmp_decode_grammar(m._h, 1 if batched else 0, C.byref(cg) if cg is not None else None,
                                         ptr(words) if words is not None else None), "cmp_decode_grammar")


def begin(m, batched, prompts, mode, prm, seed):
    from composer_amd import _lib
    mm = _lib.DECODE_LITERAL if mode == "literal" else _lib.DECODE_KV
    keep = KEEP_SMALL if mode == "kv-slide" else 0
    if not batched:
        (p,), (t, k, q) = prompts, prm[0]
        _lib.check(m._lib.cmp_decode_begin_ex(m._h, ptr(p), len(p), mm, keep, t, k, q, seed), "begin_ex")
        return
    B, ld = len(prompts), max(len(p) for p in prompts)
    buf = np.zeros((B, ld), np.int32)
    for b, p in enumerate(prompts):
        buf[b, :len(p)] = p
    lens = np.array([len(p) for p in prompts], np.int32)
    ta = np.array([q[0] for q in prm], np.float32)
    ka = np.array([q[1] for q in prm], np.int32)
    pa = np.array([q[2] for q in prm], np.float32)
    _lib.check(m._lib.cmp_decode_batch_begin_ex(m._h, ptr(buf), ptr(lens), B, ld, mm, keep, ptr(ta), ptr(ka), ptr(pa), seed),
               "batch_begin_ex")


def ban_of(g, state, words, V):
    from composer_amd import grammar as G
    if g is not None:
        return g.banned(state, words)
    return G.words_to_mask(V, words) if words is not None else np.zeros(V, bool)


def run_stepwise(m, batched, mode, prompts, prm, seed, g, words, n):
    """Steps one id at a time.  Returns ids [B][n], the row each id was drawn from Z [B][n][V] and the ban set of each draw
    [B][n][V] (from the host fold over the prompt and the ids so far); asserts the device state against the host fold after
    every step."""
    from composer_amd import _lib, grammar as G
    V, B = m.vocab_size, len(prompts)
    Z = np.zeros((B, n, V), np.float32)
    Z[:, 0] = np.stack([m(p.reshape(1, -1))[0][0, -1] for p in prompts])      # the first id: the prompt's last position
    set_grammar(m, batched, g, words)
    begin(m, batched, prompts, mode, prm, seed)
    host = [g.fold(p) if g is not None else G.GrammarState() for p in prompts]
    ids = np.zeros((B, n), np.int32)
    bans = np.zeros((B, n, V), bool)
    one = np.zeros((B, 1), np.int32)
    zb = np.zeros((B, V), np.float32)
    for i in range(n):
        for b in range(B):
            bans[b, i] = ban_of(g, host[b], words, V)
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
            if g is not None:
                g.step(host[b], ids[b, i])
            dev = m.decode_grammar_state(batched=batched, row=b)
            assert dev == host[b], (mode, batched, b, i, dev, host[b])
    return ids, Z, bans


def check_against_the_masked_rows(ids, Z, bans, prm, seed, what):
    """every id equals cmp_k_sample_ex on the host-masked row with the row's parameters, seed + b and draw counter i"""
    torch, _lib, lib, stream = gpu()
    B, n, V = Z.shape
    M = Z.copy()
    M[bans] = -np.inf
    md = torch.from_numpy(M).cuda()
    want = torch.empty((B, n), dtype=torch.int32, device="cuda")
    for b in range(B):
        t, k, q = prm[b]
        for i in range(n):
            k_sample_ex(lib, _lib, stream, md[b, i], V, float(t), int(k), float(q), seed + b, i, 1, want[b, i:])
    torch.cuda.synchronize()
    w = want.cpu().numpy()
    bad = w != ids
    assert not bad.any(), (what, np.argwhere(bad)[:5].tolist(), ids[bad][:5], w[bad][:5])
    assert not np.take_along_axis(bans, ids[:, :, None].astype(np.int64), 2).any(), what       # no banned id was drawn


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_batch1_chain_draws_the_masked_rows_id_and_keeps_the_state(mode, graph, monkeypatch):
    monkeypatch.setenv("COMPOSER_NO_GRAPH", "0" if graph else "1")
    m = small_model()
    g = grammar()
    rng = np.random.default_rng(21)
    n, seed = steps_for(mode), 31
    for j, (prm, words) in enumerate([(ROW_PARAMS[0], None), (ROW_PARAMS[3], g.pitch_range_bans(30, 100)), (ROW_PARAMS[5], None)]):
        p = prompts_for(1, rng)[0]
        ids, Z, bans = run_stepwise(m, False, mode, [p], [prm], seed + j, g, words, n)
        check_against_the_masked_rows(ids, Z, bans, [prm], seed + j, (mode, graph, prm))
        assert [k for k in g.ignored_events(np.concatenate([p, ids[0]])) if k >= len(p)] == []
        # steps(n) equals n steps of one, and the Python wrapper is the same call
        sk = {"slide_keep": KEEP_SMALL} if mode == "kv-slide" else {}
        out = m.generate(p, n, temperature=prm[0], top_k=prm[1], top_p=prm[2], mode=mode, seed=seed + j, grammar=g,
                         banned_ids=words, **sk)
        assert out.tolist() == ids[0].tolist(), (mode, graph, prm)
        assert m.decode_grammar_state() == g.fold(np.concatenate([p, ids[0]]))
        if mode == "kv-slide":
            assert m.decode_slide_stats()[0] >= 3                        # several slides happened
    m.close()


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_batched_chain_draws_each_rows_masked_id_and_keeps_each_rows_state(mode, graph, monkeypatch):
    monkeypatch.setenv("COMPOSER_NO_GRAPH", "0" if graph else "1")
    m = small_model()
    g = grammar()
    B = 5
    rng = np.random.default_rng(105)
    n, seed = steps_for(mode), 57
    prompts = prompts_for(B, rng)                                            # ragged: in kv-slide the rows slide (and are held) at different steps
    assert len({len(p) for p in prompts}) >= 3
    prm = [ROW_PARAMS[(b + 3) % len(ROW_PARAMS)] for b in range(B)]
    words = g.pitch_range_bans(21, 108)
    ids, Z, bans = run_stepwise(m, True, mode, prompts, prm, seed, g, words, n)
    check_against_the_masked_rows(ids, Z, bans, prm, seed, (mode, graph))
    sk = {"slide_keep": KEEP_SMALL} if mode == "kv-slide" else {}
    out = m.generate_batch(prompts, n, temperature=[q[0] for q in prm], top_k=[q[1] for q in prm], top_p=[q[2] for q in prm],
                           mode=mode, seed=seed, grammar=g, banned_ids=words, **sk)
    assert out.tolist() == ids.tolist()
    for b in range(B):
        assert m.decode_grammar_state(batched=True, row=b) == g.fold(np.concatenate([prompts[b], ids[b]]))
    if mode == "kv-slide":
        assert m.decode_slide_stats(batched=True)[0] >= 3 * B
    m.close()


def test_static_bans_alone_and_rule_subsets():
    """no layout (static vector only: the state stays empty), and each single rule bit, in the kv chain"""
    from composer_amd import grammar as G
    m = small_model()
    rng = np.random.default_rng(77)
    p = prompts_for(1, rng)[0]
    words = G.ban_words(V0, rng.random(V0) < 0.6)
    ids, Z, bans = run_stepwise(m, False, "kv", [p], [ROW_PARAMS[3]], 5, None, words, 20)
    check_against_the_masked_rows(ids, Z, bans, [ROW_PARAMS[3]], 5, "static only")
    for rules in (G.NOTE_OFF_SOUNDING, G.NOTE_ON_SILENT, G.PEDAL):
        g = grammar(rules)
        ids, Z, bans = run_stepwise(m, True, "kv", [p, p[:1]], [ROW_PARAMS[0], ROW_PARAMS[1]], 6, g, None, 20)
        check_against_the_masked_rows(ids, Z, bans, [ROW_PARAMS[0], ROW_PARAMS[1]], 6, ("rules", rules))
    m.close()


# ---------------------------------------------------------------- 3. row independence
@pytest.mark.parametrize("mode", MODES)
def test_a_batched_row_is_the_batch1_chain_and_does_not_depend_on_B(mode):
    m = small_model()
    g = grammar()
    rng = np.random.default_rng(33)
    n, seed, B = steps_for(mode), 19, 5
    prompts = prompts_for(B, rng)
    prm = [ROW_PARAMS[(b + 3) % len(ROW_PARAMS)] for b in range(B)]
    words = g.pitch_range_bans(36, 96)
    sk = {"slide_keep": KEEP_SMALL} if mode == "kv-slide" else {}
    kw = lambda rows: dict(temperature=[prm[b][0] for b in rows], top_k=[prm[b][1] for b in rows], top_p=[prm[b][2] for b in rows])
    full = m.generate_batch(prompts, n, mode=mode, seed=seed, grammar=g, banned_ids=words, **kw(range(B)), **sk)
    for b in range(B):
        t, k, q = prm[b]
        alone = m.generate(prompts[b], n, temperature=t, top_k=k, top_p=q, mode=mode, seed=seed + b, grammar=g, banned_ids=words, **sk)
        assert alone.tolist() == full[b].tolist(), (mode, b)
    two = m.generate_batch(prompts[:2], n, mode=mode, seed=seed, grammar=g, banned_ids=words, **kw(range(2)), **sk)
    assert two.tolist() == full[:2].tolist()
    m.close()


# ---------------------------------------------------------------- 4. the property the feature is for
def test_a_constrained_run_has_no_ignored_event():
    m = small_model()
    g = grammar()
    p = np.array([60, 64, 300, 388], np.int32)                # two notes on, a time shift, the pedal down: no ignored event
    n = 96
    generated = lambda ids: [i - len(p) for i in g.ignored_events(np.concatenate([p, ids])) if i >= len(p)]
    for batched in (False, True):
        if batched:
            free = m.generate_batch([p, p], n, temperature=1.0, mode="kv-slide", slide_keep=KEEP_SMALL, seed=3)
            held = m.generate_batch([p, p], n, temperature=1.0, mode="kv-slide", slide_keep=KEEP_SMALL, seed=3, grammar=g)
        else:
            free = m.generate(p, n, temperature=1.0, mode="kv-slide", slide_keep=KEEP_SMALL, seed=3)[None]
            held = m.generate(p, n, temperature=1.0, mode="kv-slide", slide_keep=KEEP_SMALL, seed=3, grammar=g)[None]
        for row_free, row_held in zip(free, held):
            assert len(generated(row_free)) >= 1              # the precondition: near-uniform logits, a third of the ids NOTE_OFF
            assert generated(row_held) == []
    m.close()


# ---------------------------------------------------------------- 5. off is off
@pytest.mark.parametrize("mode", MODES)
def test_off_after_a_constrained_run_is_a_model_that_never_had_a_grammar(mode):
    from composer_amd import _lib, grammar as G
    m, fresh = small_model(), small_model()
    g = grammar()
    rng = np.random.default_rng(8)
    n, seed = steps_for(mode), 11
    sk = {"slide_keep": KEEP_SMALL} if mode == "kv-slide" else {}
    prompts = prompts_for(5, rng)
    for t, k, q in ((1.0, 0, 1.0), (0.7, 40, 0.9), (0.0, 0, 1.0)):
        base1 = fresh.generate(prompts[0], n, temperature=t, top_k=k, top_p=q, mode=mode, seed=seed, **sk)
        baseb = fresh.generate_batch(prompts, n, temperature=t, top_k=k, top_p=q, mode=mode, seed=seed, **sk)
        on1 = m.generate(prompts[0], n, temperature=t, top_k=k, top_p=q, mode=mode, seed=seed, grammar=g, **sk)
        onb = m.generate_batch(prompts, n, temperature=t, top_k=k, top_p=q, mode=mode, seed=seed, grammar=g, **sk)
        if t == 1.0 and k == 0:                               # near-uniform draws: the grammar did change the ids
            assert on1.tolist() != base1.tolist() and onb.tolist() != baseb.tolist()
        # cmp_decode_grammar(NULL, NULL)
        _lib.check(m._lib.cmp_decode_grammar(m._h, 0, None, None), "off")
        _lib.check(m._lib.cmp_decode_grammar(m._h, 1, None, None), "off")
        assert m.generate(prompts[0], n, temperature=t, top_k=k, top_p=q, mode=mode, seed=seed, **sk).tolist() == base1.tolist()
        assert m.generate_batch(prompts, n, temperature=t, top_k=k, top_p=q, mode=mode, seed=seed, **sk).tolist() == baseb.tolist()
        # rules 0 and an all-zero static vector: the same ids
        zero = np.zeros(G.words_for(V0), np.uint32)
        assert m.generate(prompts[0], n, temperature=t, top_k=k, top_p=q, mode=mode, seed=seed, grammar=grammar(0), banned_ids=zero,
                          **sk).tolist() == base1.tolist()
        assert m.generate_batch(prompts, n, temperature=t, top_k=k, top_p=q, mode=mode, seed=seed, grammar=grammar(0),
                                banned_ids=zero, **sk).tolist() == baseb.tolist()
        # ... while the state is still kept for the caller to read
        assert m.decode_grammar_state(batched=True, row=4) == g.fold(np.concatenate([prompts[4], baseb[4]]))
    m.close(); fresh.close()


# ---------------------------------------------------------------- 6. a second layout
def test_second_layout_kv_stepwise():
    """max_time_steps = 10, velocity_bins = 4: V = 272, TIME_SHIFT at 260, the pedal at 270 / 271 -- a hard-coded offset fails here"""
    g = grammar(params=(10, 10, 4))
    assert g.vocab_size == 272
    m = small_model(V=272)
    rng = np.random.default_rng(272)
    prompts = prompts_for(3, rng, V=272)
    prm = [ROW_PARAMS[0], ROW_PARAMS[3], ROW_PARAMS[5]]
    ids, Z, bans = run_stepwise(m, True, "kv", prompts, prm, 13, g, g.pitch_range_bans(40, 90), 20)
    check_against_the_masked_rows(ids, Z, bans, prm, 13, "V=272 batched")
    ids, Z, bans = run_stepwise(m, False, "kv", prompts[:1], prm[1:2], 14, g, None, 20)
    check_against_the_masked_rows(ids, Z, bans, prm[1:2], 14, "V=272 batch-1")
    m.close()


# ---------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_configuration_alone():
    from composer_amd import _lib, grammar as G
    m = small_model()
    lib, h = m._lib, m._h
    sw, ped, ts = (C.c_uint32 * 4)(), C.c_int32(), C.c_int64()
    for batched in (0, 1):
        assert lib.cmp_decode_grammar_state(h, batched, 0, C.byref(sw), C.byref(ped), C.byref(ts)) == -4          # before begin
    g = grammar()
    words = g.pitch_range_bans(48, 84)
    p = np.array([60, 300, 388], np.int32)
    want1 = m.generate(p, 20, temperature=1.0, mode="kv", seed=2, grammar=g, banned_ids=words)
    wantb = m.generate_batch([p, p[:2]], 20, temperature=1.0, mode="kv", seed=2, grammar=g, banned_ids=words)
    assert lib.cmp_decode_grammar_state(h, 0, 1, C.byref(sw), C.byref(ped), C.byref(ts)) == -1                    # a bad row
    assert lib.cmp_decode_grammar_state(h, 1, 2, C.byref(sw), C.byref(ped), C.byref(ts)) == -1
    assert lib.cmp_decode_grammar_state(h, 1, -1, C.byref(sw), C.byref(ped), C.byref(ts)) == -1
    ok = dict(note_on0=0, note_off0=128, time_shift0=288, time_shift_n=100, sustain_on=388, sustain_off=389, rules=7)
    bad = [
        (dict(note_on0=300), "outside"), (dict(note_off0=-1), "outside"), (dict(time_shift0=300), "outside"),
        (dict(sustain_off=390), "outside"),
        (dict(note_off0=100), "overlap"), (dict(time_shift0=200), "overlap"), (dict(sustain_on=5), "overlap"),
        (dict(sustain_on=389), "overlap"),
        (dict(sustain_on=-1), "sustain"), (dict(sustain_off=-1), "sustain"),
        (dict(time_shift_n=0), "time_shift_n"),
        (dict(rules=8), "rule"), (dict(rules=-1), "rule"),
    ]
    every_shift = G.ban_words(V0, np.arange(288, 388))
    everything = G.ban_words(V0, np.ones(V0, bool))
    for batched in (0, 1):
        for change, word in bad:
            cg = _lib.EventGrammar(**dict(ok, **change))
            assert lib.cmp_decode_grammar(h, batched, C.byref(cg), None) == -1, change
            assert word in _lib.last_error(), (change, _lib.last_error())
        cg = _lib.EventGrammar(**ok)
        assert lib.cmp_decode_grammar(h, batched, C.byref(cg), ptr(every_shift)) == -1
        assert "TIME_SHIFT" in _lib.last_error()
        assert lib.cmp_decode_grammar(h, batched, None, ptr(everything)) == -1
        assert "all 390" in _lib.last_error()
    # the Python wrapper refuses the same cases from its arguments
    with pytest.raises(ValueError, match="TIME_SHIFT"):
        m.generate(p, 4, grammar=g, banned_ids=every_shift)
    with pytest.raises(ValueError, match="all 390"):
        m.generate_batch([p], 4, banned_ids=everything)
    with pytest.raises(ValueError, match="272"):
        m.generate(p, 4, grammar=grammar(params=(10, 10, 4)))
    # nothing was half applied: the next begins run under the configuration that was in force
    _lib.check(lib.cmp_decode_begin(h, ptr(p), len(p), _lib.DECODE_KV, 1.0, 2), "begin")
    out = np.zeros(20, np.int32)
    _lib.check(lib.cmp_decode_steps(h, 20, ptr(out)), "steps")
    assert out.tolist() == want1.tolist()
    buf = np.zeros((2, 3), np.int32); buf[0] = p; buf[1, :2] = p[:2]
    lens = np.array([3, 2], np.int32)
    _lib.check(lib.cmp_decode_batch_begin(h, ptr(buf), ptr(lens), 2, 3, _lib.DECODE_KV, 1.0, 2), "batch_begin")
    outb = np.zeros((2, 20), np.int32)
    _lib.check(lib.cmp_decode_batch_steps(h, 20, ptr(outb)), "batch_steps")
    assert outb.tolist() == wantb.tolist()
    m.close()


# ---------------------------------------------------------------- 8. CLI
def test_cli_constrain_and_pitch_range(tmp_path):
    from composer_amd import cli, checkpoint as ckpt, dataset as D
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
    g = grammar()
    prompt = [60, 300, 388, 64]
    r = CliRunner()
    res = r.invoke(cli.cli, ["generate", "transformer", str(run), str(tmp_path / "out.data"), "--prompt-ids", "60,300,388,64",
                             "--length", "80", "--constrain", "--pitch-range", "48:84", "--num-samples", "2",
                             "--decode-mode", "kv-slide"], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    assert "constrain on" in res.stderr and "48:84" in res.stderr
    rows = []
    for i in range(2):
        got, _ = D.read_data_file(tmp_path / ("out-%d.data" % i))
        got = got.astype(np.int64)
        assert got[:4].tolist() == prompt and len(got) == 84
        assert [k for k in g.ignored_events(got) if k >= 4] == []
        on = got[4:][(got[4:] >= g.note_on0) & (got[4:] < g.note_on0 + 128)] - g.note_on0
        assert on.size and on.min() >= 48 and on.max() <= 84
        rows.append(got.tolist())
    assert rows[0] != rows[1]
    for bad in ("84:48", "48", "0:128", "a:b"):
        res = r.invoke(cli.cli, ["generate", "transformer", str(run), str(tmp_path / "x.data"), "--prompt-ids", "60",
                                 "--pitch-range", bad])
        assert res.exit_code == 2 and "pitch-range" in res.output
