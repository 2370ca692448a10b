"""Sliding-window decode (`kv-slide`: cmp_decode_begin_slide / cmp_decode_batch_begin_slide) against the float64 oracle, on whole
logit rows, at every step, across several slides of both decode chains.

Contract (composer_amd.transformer.slide_context_length, c(n)): with s = prompt ++ ids so far and n = len(s), the next id is drawn
from the last position of a plain forward pass over s[n - c(n) : n] at positions 0 .. c(n) - 1.  The oracle side restates that
with the cheapest equivalent `past`: a full pass over the tail at a slide (n > W and c(n) == keep), one token on the presents of
the pass before it otherwise -- teacher-forced on the ids the HIP chain drew, so both sides see the same context.  The helpers
are those of tests/test_gpu_decode_logits.py, restated.

Bound (fp32 models): the project's own, max |z_hip - z64| <= 4 * floor + 1e-6 * max |z64|, floor = max |z32 - z64| of the float32
oracle on the same contexts.  A slide step's logits come out of the forward pass (cmp_decode_logits_get shows the row the id was
drawn from); the per-token steps' out of the decode chain.  bf16 model: 3e-2 * max |z| against float64 at every step; the tighter
emulated-prefill bound (emulate_bf16 applied to every re-encode) on the per-token steps only -- a slide step's logits are the
bf16 forward's own, as a begin's first id is.
`test_slide_mistakes_move_the_logits_by_ten_bounds` (CPU) keeps the bound honest: a window start off by one, ONE stale cache row
left from before the slide, or the token after a slide at position keep +- 1 each move the float64 logits by >= 10 bounds.

Cases: head sizes 16 / 32 / 64 / 128, use_layer_norm = False, the padded head (E 96 / H 4), one bf16 model; keep 1, 37, W // 2,
W - 1 spread over them; both chains; the graph and COMPOSER_NO_GRAPH=1; a ragged batch of 37 (22 rows sliding in one step,
a row with P = W, a row whose first tail reaches back into its prompt) bitwise against batches of one and against a workspace
that holds one row per forward call; the benchmark's geometry (E 512 / H 8 / L 6 / W 2048, keep 1024); a batch-1 decode with a
grammar, interrupted between two cmp_decode_steps calls by a batched decode and a forward pass, that goes on id for id.

Measured err / floor (max |z_hip - z64| over max |z32 - z64|; floors 4e-7 .. 3.5e-6 at max |z| 2.3 .. 8.6), MI355X, batch-1 chain /
batched chain (B = 5), 3 or more slides of some row in every case; the worst logit row is a slide step's in all but two cases:
  d16 keep 1       1.73 / 1.73                         d32 keep 37 (batch-1 chain without the graph)    1.00 / 1.00
  d32_noln keep 48 0.81 / 0.83 (batched: no graph)     d64 keep 95 (9 slides)                           0.93 / 0.93
  d128 keep 37     0.80 / 0.75                         pad24 keep 80 (W 160)                            1.41 / 0.80
  ragged B = 37, keep 60 (d16, 8 oracle rows)  1.01; the 37 rows bitwise a batch of one, and bitwise the one-row-per-call workspace
  c5 keep 1024     2.01 (batch-1 chain) / 1.97 (B = 64, 8 oracle rows, 8 rows per forward call; the other 56 rows bitwise a batch of one)
No geometry needs more than the factor 4.  bf16 (keep 48, both chains alike): against float64 err 1.11e-2 at a slide step (bound
3e-2 * max |z| = 1.46e-1); the per-token steps against the emulated re-encodes err 9.05e-5 where the bf16 effect is 4.3e-4 .. 9.9e-4
(bound 2.2e-4 .. 5.0e-4).
"""
import ctypes as C

import numpy as np
import pytest

from oracle import transformer_oracle as O

V = 390

# name: E, H, L, W, stddev, dtype, use_layer_norm, keep
GEOMS = {
    "d16": (64, 4, 2, 96, 0.05, "fp32", True, 1),
    "d32": (64, 2, 2, 96, 0.05, "fp32", True, 37),
    "d32_noln": (64, 2, 2, 96, 0.05, "fp32", False, 48),
    "d64": (128, 2, 2, 96, 0.05, "fp32", True, 95),
    "d128": (256, 2, 1, 96, 0.05, "fp32", True, 37),
    "pad24": (96, 4, 2, 160, 0.05, "fp32", True, 80),
    "c5": (512, 8, 6, 2048, 0.06, "fp32", True, 1024),
    "bf16": (128, 2, 2, 96, 0.05, "bf16", True, 48),
}
# err <= FACTOR * floor + 1e-6 * max|z64|; 4 unless a measured, explained ordering effect needs more on one geometry
FACTOR = {}
BF16_TOL = 3e-2

def slide_context_length(n, window, keep):
    from composer_amd.transformer import slide_context_length as f
    return f(n, window, keep)


def make_params(name):
    """O.init_params at the geometry's weight scale, cast to float32; gamma / beta / biases moved off 1 / 0"""
    E, H, L, W, s = GEOMS[name][:5]
    p = O.init_params(V, E, W, L, seed=sorted(GEOMS).index(name) + 140, stddev=s)
    rng = np.random.default_rng(7)
    for n, _, kind in O.param_specs(V, E, W, L):
        if kind == "ones":
            p[n] = p[n] + 0.05 * rng.standard_normal(p[n].shape)
        elif kind == "zeros":
            p[n] = p[n] + 0.02 * rng.standard_normal(p[n].shape)
    return {k: v.astype(np.float32) for k, v in p.items()}


def steps_for(name, slides=3):
    """per-token + slide steps so that a row starting a few tokens below the window slides `slides` times"""
    W, keep = GEOMS[name][3], GEOMS[name][7]
    return min(slides * (W - keep + 1) + 12, 330)


def make_prompts(name, B):
    """ragged rows near the window's end (the first slide comes early), one full window, one short row"""
    W = GEOMS[name][3]
    lens = [W - 5, W, W - 3, 5, W // 2, W - 1, W - 11][:B] if B <= 7 else None
    rows = []
    for b in range(B):
        rng = np.random.default_rng([sorted(GEOMS).index(name), b, 5])
        rows.append(rng.integers(0, V, lens[b]).astype(np.int32))
    return rows


def oracle_config(name):
    E, H, L, W, _, _, use_ln, _ = GEOMS[name]
    return O.Config(V, E, W, L, H, use_layer_normalization=use_ln)


def make_model(name, params, max_batch=1, max_seq=None):
    from composer_amd.transformer import Transformer
    E, H, L, W, _, dtype, use_ln, _ = GEOMS[name]
    m = Transformer(V, E, W, L, H, attention_dropout_rate=0.0, residual_dropout_rate=0.0, use_layer_normalization=use_ln,
                    dtype=dtype, seed=0, max_batch=max_batch, max_seq=W if max_seq is None else max_seq)
    m.set_weights(params)
    return m


# ---------------------------------------------------------------- the HIP side: ids [B, n + 1], logits [B, n, V]
def hip_decode_one(m, prompts, seed, keep, n, temperature=1.0):
    """the batch-1 chain (decode.hip), row b with seed + b; keep None: plain kv mode"""
    from composer_amd import _lib
    lib, h = m._lib, m._h
    ids = np.zeros((len(prompts), n + 1), np.int32)
    Z = np.zeros((len(prompts), n, V), np.float32)
    one = np.zeros(1, np.int32)
    for b, p in enumerate(prompts):
        p = np.ascontiguousarray(p, np.int32)
        if keep is None:
            _lib.check(lib.cmp_decode_begin(h, p.ctypes.data_as(C.c_void_p), len(p), _lib.DECODE_KV, temperature, seed + b), "begin")
        else:
            _lib.check(lib.cmp_decode_begin_slide(h, p.ctypes.data_as(C.c_void_p), len(p), keep, temperature, seed + b), "begin_slide")
        for k in range(n + 1):
            _lib.check(lib.cmp_decode_steps(h, 1, one.ctypes.data_as(C.c_void_p)), "steps")
            ids[b, k] = one[0]
            if k:
                _lib.check(lib.cmp_decode_logits_get(h, Z[b, k - 1].ctypes.data_as(C.c_void_p)), "logits")
    return ids, Z


def batch_begin(m, prompts, seed, keep, temperature=1.0):
    from composer_amd import _lib
    lib, h = m._lib, m._h
    B, ld = len(prompts), max(len(p) for p in prompts)
    buf = np.zeros((B, ld), np.int32)
    for b, p in enumerate(prompts):
        buf[b, :len(p)] = p
    lens = np.array([len(p) for p in prompts], np.int32)
    if keep is None:
        return lib.cmp_decode_batch_begin(h, buf.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), B, ld, _lib.DECODE_KV,
                                          temperature, seed)
    return lib.cmp_decode_batch_begin_slide(h, buf.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), B, ld, keep,
                                            temperature, seed)


def hip_decode_batch(m, prompts, seed, keep, n, temperature=1.0):
    """the batched chain (decode_batch.hip)"""
    from composer_amd import _lib
    lib, h = m._lib, m._h
    B = len(prompts)
    _lib.check(batch_begin(m, prompts, seed, keep, temperature), "begin")
    ids = np.zeros((B, n + 1), np.int32)
    Z = np.zeros((B, n, V), np.float32)
    col = np.zeros((B, 1), np.int32)
    z = np.zeros((B, V), np.float32)
    for k in range(n + 1):
        _lib.check(lib.cmp_decode_batch_steps(h, 1, col.ctypes.data_as(C.c_void_p)), "steps")
        ids[:, k] = col[:, 0]
        if k:
            _lib.check(lib.cmp_decode_batch_logits_get(h, z.ctypes.data_as(C.c_void_p)), "logits")
            Z[:, k - 1] = z
    return ids, Z


def slide_stats(m, batched):
    from composer_amd import _lib
    rs, fc = C.c_int64(-1), C.c_int64(-1)
    _lib.check(m._lib.cmp_decode_slide_stats(m._h, 1 if batched else 0, C.byref(rs), C.byref(fc)), "slide_stats")
    return rs.value, fc.value


def is_slide(P, k, W, keep):
    """id k (0-based) of a row with a P-token prompt is drawn at sequence length P + k: from a re-encode?"""
    n = P + k
    return n > W and slide_context_length(n, W, keep) == keep


def count_slides(P, n_ids, W, keep):
    return sum(is_slide(P, k, W, keep) for k in range(n_ids))


# ---------------------------------------------------------------- the oracle side
def _oracle(name, params, kind):
    if kind == "f64":
        return O.OracleTransformer(oracle_config(name), {k: v.astype(np.float64) for k, v in params.items()})
    if kind == "f32":
        return O.OracleTransformer(oracle_config(name), params, dtype=np.float32)
    return O.OracleTransformer(oracle_config(name), {k: v.astype(np.float64) for k, v in params.items()}, emulate_bf16=True)


def oracle_logits(name, params, kind, prompts, ids, keep=None):
    """[R, n, V] and the slide mask [R, n]: entry k - 1 is the logits id k of row r is drawn from, i.e. of the last position of a
    pass over s[n - c(n) : n], s = prompts[r] ++ ids[r, :k], n = len(s) -- as a full pass over the tail at a slide, as one token
    on the presents of the draw before otherwise.  kind "f64" / "f32": that float type throughout; "bf16fill": the prefill and
    every re-encode with emulate_bf16, the per-token steps in plain float64 on their presents."""
    W = GEOMS[name][3]
    keep = GEOMS[name][7] if keep is None else keep
    fill_orc = _oracle(name, params, kind)
    step_orc = _oracle(name, params, "f64") if kind == "bf16fill" else fill_orc
    out = np.zeros((len(prompts), ids.shape[1] - 1, V), np.float64)
    slid = np.zeros((len(prompts), ids.shape[1] - 1), bool)
    for r, p in enumerate(prompts):
        s = [int(t) for t in p]
        past = [np.asarray(a, step_orc.dtype) for a in fill_orc.forward(np.asarray(s)[None])[1]]
        for k in range(1, ids.shape[1]):
            s.append(int(ids[r, k - 1]))
            n = len(s)
            c = slide_context_length(n, W, keep)
            if n > W and c == keep:
                logits, pres, _ = fill_orc.forward(np.asarray(s[n - keep:])[None])
                pres = [np.asarray(a, step_orc.dtype) for a in pres]
                slid[r, k - 1] = True
            else:
                assert past[0].shape[-2] == c - 1, (n, c, past[0].shape)
                logits, pres, _ = step_orc.forward(np.array([[s[-1]]]), past=past)
            out[r, k - 1] = logits[0, -1]
            past = pres
    return out, slid


def compare(label, name, params, prompts, ids, Z, keep=None, min_slides=1):
    assert np.isfinite(Z).all(), label
    assert ids.min() >= 0 and ids.max() < V
    z64, slid = oracle_logits(name, params, "f64", prompts, ids, keep)
    z32, _ = oracle_logits(name, params, "f32", prompts, ids, keep)
    assert slid.sum(1).max() >= min_slides, (label, slid.sum(1))
    floor = float(np.abs(z32 - z64).max())
    zmax = float(np.abs(z64).max())
    d = np.abs(Z - z64)
    err = float(d.max())
    err_slide = float(d[slid].max()) if slid.any() else 0.0
    r, k = [int(t) for t in np.unravel_index(np.argmax(d.max(-1)), d.shape[:2])]
    worst = "worst at row %d (prompt %d ids) id %d (%s)" % (r, len(prompts[r]), k + 1, "slide" if slid[r, k] else "step")
    if GEOMS[name][5] == "bf16":
        bound = BF16_TOL * zmax
        zem, _ = oracle_logits(name, params, "bf16fill", prompts, ids, keep)
        st = ~slid
        err_em = float(np.abs(Z - zem)[st].max())
        effect = float(np.abs(zem - z64)[st].max())
        bound_em = 0.5 * effect + 4 * floor + 1e-6 * zmax
        extra = "; per-token steps against the emulate_bf16 re-encodes: err %.3e, bf16 effect %.3e, bound %.3e" % (err_em, effect, bound_em)
    else:
        bound = FACTOR.get(name, 4) * floor + 1e-6 * zmax
        extra = ""
    print("\n[decode-slide] %-40s slides/row max %d err %.3e (slide steps %.3e) floor %.3e err/floor %6.2f bound %.3e max|z| %.3f %s%s"
          % (label, int(slid.sum(1).max()), err, err_slide, floor, err / floor, bound, zmax, worst, extra))
    assert err <= bound, (label, err, floor, err / floor, bound, worst)
    if extra:
        assert err_em <= bound_em, (label, err_em, effect, bound_em)


CASES = [
    # geometry, chain, B, graph
    ("d16", "one", 3, True), ("d16", "batch", 5, True),
    ("d32", "one", 3, False), ("d32", "batch", 5, True),
    ("d32_noln", "one", 3, True), ("d32_noln", "batch", 5, False),
    ("d64", "one", 3, True), ("d64", "batch", 5, True),
    ("d128", "one", 3, True), ("d128", "batch", 5, True),
    ("pad24", "one", 3, True), ("pad24", "batch", 5, True),
    ("bf16", "one", 3, True), ("bf16", "batch", 5, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,chain,B,graph", CASES, ids=["%s-%s-B%d-%s" % (n, c, b, "graph" if g else "nograph")
                                                          for n, c, b, g in CASES])
def test_slide_logits_follow_the_oracle(name, chain, B, graph, monkeypatch):
    monkeypatch.setenv("COMPOSER_NO_GRAPH", "0" if graph else "1")
    params = make_params(name)
    prompts = make_prompts(name, B)
    keep = GEOMS[name][7]
    m = make_model(name, params)
    n = steps_for(name)
    ids, Z = (hip_decode_one if chain == "one" else hip_decode_batch)(m, prompts, 11, keep, n)
    rs, fc = slide_stats(m, chain == "batch")
    m.close()
    W = GEOMS[name][3]
    want = [count_slides(len(p), n + 1, W, keep) for p in prompts]
    assert rs == (want[-1] if chain == "one" else sum(want)), (rs, want)       # the batch-1 chain counts since ITS last begin
    assert 1 <= fc <= rs
    compare("%s %s B=%d keep=%d%s" % (name, chain, B, keep, "" if graph else " nograph"), name, params, prompts, ids, Z, min_slides=3)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", ["one", "batch"])
def test_before_the_first_slide_the_mode_is_kv_itself(chain):
    """same kernels, same bits: ids and logits of kv-slide equal plain kv's up to the last step that fits the window"""
    name = "d32"
    W, keep = GEOMS[name][3], GEOMS[name][7]
    params = make_params(name)
    prompts = [p[:q] for p, q in zip(make_prompts(name, 3), (60, 50, 7))]
    n = W - 60                      # the longest row's last step consumes position W - 1
    m = make_model(name, params)
    dec = hip_decode_one if chain == "one" else hip_decode_batch
    ids_kv, Z_kv = dec(m, prompts, 5, None, n)
    ids_sl, Z_sl = dec(m, prompts, 5, keep, n)
    assert slide_stats(m, chain == "batch") == (0, 0)
    m.close()
    assert ids_kv.tolist() == ids_sl.tolist()
    assert np.array_equal(Z_kv.view(np.uint32), Z_sl.view(np.uint32))


RAGGED_W, RAGGED_KEEP, RAGGED_STEPS = 96, 60, 120


def ragged_prompts():
    """B = 37: rows 0 .. 21 share P = 60 (22 rows slide in the same step: more than one 16-row tile); row 22 has P = W (its second
    id already comes from a slide); row 23 has P = W - 3 (its first tail, keep = 60 >= 8, holds prompt and generated ids); the
    others slide at steps of their own."""
    lens = [60] * 22 + [RAGGED_W, RAGGED_W - 3] + [61 + 2 * i for i in range(13)]
    assert len(lens) == 37
    return [np.random.default_rng([99, b]).integers(0, V, n).astype(np.int32) for b, n in enumerate(lens)]


@pytest.mark.gpu
def test_ragged_batch_rows_are_independent_and_packing_is_bitwise_neutral():
    name = "d16"
    assert GEOMS[name][3] == RAGGED_W
    W, keep, n = RAGGED_W, RAGGED_KEEP, RAGGED_STEPS
    params = make_params(name)
    prompts = ragged_prompts()
    B = len(prompts)
    want = [count_slides(len(p), n + 1, W, keep) for p in prompts]
    assert want[0] >= 3 and is_slide(W, 1, W, keep) and is_slide(W - 3, 4, W, keep)
    # (A) a workspace that packs every row of a slide into one forward call
    m = make_model(name, params, max_batch=B, max_seq=W)
    ids, Z = hip_decode_batch(m, prompts, 21, keep, n)
    rs, fc = slide_stats(m, True)
    assert rs == sum(want), (rs, want)
    assert fc < rs, (fc, rs)
    assert np.isfinite(Z).all()
    for b in range(B):                                   # bitwise a batch of one with seed + b
        ids1, Z1 = hip_decode_batch(m, [prompts[b]], 21 + b, keep, n)
        assert ids1[0].tolist() == ids[b].tolist(), b
        assert np.array_equal(Z1[0].view(np.uint32), Z[b].view(np.uint32)), b
    m.close()
    # (B) max_batch = 1, max_seq = keep: the workspace is the first call's W tokens < 2 * keep, exactly one row per forward call
    m = make_model(name, params, max_batch=1, max_seq=keep)
    ids_b, Z_b = hip_decode_batch(m, prompts, 21, keep, n)
    rs_b, fc_b = slide_stats(m, True)
    m.close()
    assert (rs_b, fc_b) == (rs, rs)
    assert ids_b.tolist() == ids.tolist()
    assert np.array_equal(Z_b.view(np.uint32), Z.view(np.uint32))
    rows = [0, 15, 16, 21, 22, 23, 24, 36]
    compare("d16 ragged batch B=37 keep=60 (8 oracle rows)", name, params, [prompts[b] for b in rows], ids[rows], Z[rows], keep=keep,
            min_slides=3)


@pytest.mark.gpu
def test_a_workspace_too_small_for_keep_is_refused_before_any_id():
    from composer_amd import _lib
    name = "d32"
    params = make_params(name)
    m = make_model(name, params, max_batch=1, max_seq=8)
    p = np.array([5, 6, 7, 8], np.int32)
    first = m.generate(p, 4, temperature=1.0, mode="kv", seed=3).tolist()        # sizes the workspace: 8 tokens
    first_b = m.generate_batch([p, p[:2]], 4, temperature=1.0, mode="kv", seed=3).tolist()
    for batched in (False, True):
        if batched:
            rc = batch_begin(m, [p, p[:2]], 3, 48)
        else:
            rc = m._lib.cmp_decode_begin_slide(m._h, p.ctypes.data_as(C.c_void_p), 4, 48, 1.0, 3)
        assert rc != 0
        msg = _lib.last_error()
        assert "max_batch" in msg and "max_seq" in msg, msg
    with pytest.raises(Exception, match="max_seq"):
        m.generate(p, 8, mode="kv-slide", slide_keep=48)
    assert m.generate(p, 4, temperature=1.0, mode="kv", seed=3).tolist() == first
    assert m.generate_batch([p, p[:2]], 4, temperature=1.0, mode="kv", seed=3).tolist() == first_b
    # keep outside [1, W - 1]: CMP_ERR_INVALID, the message names the range
    for keep in (0, GEOMS[name][3]):
        assert m._lib.cmp_decode_begin_slide(m._h, p.ctypes.data_as(C.c_void_p), 4, keep, 1.0, 3) == -1
        assert "window_size - 1" in _lib.last_error()
        assert batch_begin(m, [p], 3, keep) == -1 and "window_size - 1" in _lib.last_error()
    m.close()


@pytest.mark.gpu
def test_generate_goes_on_past_the_window_and_steps_n_equals_n_steps_of_one():
    from composer_amd import _lib
    name = "d32"
    W, keep = GEOMS[name][3], GEOMS[name][7]
    params = make_params(name)
    m = make_model(name, params)
    p = make_prompts(name, 1)[0][:10]
    with pytest.raises(IndexError):
        m.generate(p, 3 * W, temperature=1.0, mode="kv", seed=4)
    out = m.generate(p, 3 * W, temperature=1.0, mode="kv-slide", slide_keep=keep, seed=4)
    assert out.shape == (3 * W,) and out.min() >= 0 and out.max() < V
    assert m.decode_slide_stats() == (count_slides(10, 3 * W, W, keep),) * 2
    assert count_slides(10, 3 * W, W, keep) >= 3
    ids1, _ = hip_decode_one(m, [p], 4, keep, 3 * W - 1)
    assert out.tolist() == ids1[0].tolist()              # one call spanning the slides == one step per call
    # the default keep is W // 2
    a = m.generate(p, 2 * W, temperature=1.0, mode="kv-slide", seed=4)
    b = m.generate(p, 2 * W, temperature=1.0, mode="kv-slide", slide_keep=W // 2, seed=4)
    assert a.tolist() == b.tolist()
    # the batched chain: steps(n) spanning slides == n steps of one; rows equal the batch-1 chain's first ids' contract
    prompts = [p, make_prompts(name, 2)[1]]
    ob = m.generate_batch(prompts, 2 * W, temperature=1.0, mode="kv-slide", slide_keep=keep, seed=4)
    rs, fc = m.decode_slide_stats(batched=True)
    assert rs == sum(count_slides(len(q), 2 * W, W, keep) for q in prompts) and 1 <= fc <= rs
    idsb, _ = hip_decode_batch(m, prompts, 4, keep, 2 * W - 1)
    assert ob.tolist() == idsb.tolist()
    with pytest.raises(IndexError):
        m.generate_batch(prompts, 2 * W, temperature=1.0, mode="kv", seed=4)
    # the id capacity per begin stays refused as before
    _lib.check(m._lib.cmp_decode_begin_slide(m._h, np.ascontiguousarray(p).ctypes.data_as(C.c_void_p), len(p), keep, 1.0, 4))
    big = np.zeros(65537, np.int32)
    assert m._lib.cmp_decode_steps(m._h, 65537, big.ctypes.data_as(C.c_void_p)) != 0
    m.close()


@pytest.mark.gpu
def test_the_batch1_chain_survives_a_batched_decode_between_its_steps():
    """tests/test_gpu_decode_batch.py::test_state_isolation_and_continuation in the other direction.  Both chains prefill, slide and
    read back through the same functions, each on its own state: a batch-1 kv-slide decode with a grammar, interrupted by a batched
    kv-slide decode with another grammar and by a forward pass, goes on as if nothing had run in between -- ids, grammar state
    and slide counters.  Integer equality throughout."""
    from composer_amd import _lib, grammar as G
    name = "d32"
    W, keep = GEOMS[name][3], GEOMS[name][7]
    n_ids, cut = 130, 60
    m = make_model(name, make_params(name), max_batch=4)
    lib, h = m._lib, m._h
    p = np.ascontiguousarray(make_prompts(name, 1)[0][:10])
    gram, bans = G.EventGrammar(V, 0, 128, 288, 100, 388, 389, rules=G.ALL), [3, 140, 300, 301]
    other, other_bans = G.EventGrammar(V, 128, 0, 256, 120, rules=G.NOTE_ON_SILENT), [7, 290]
    slides = count_slides(10, n_ids, W, keep)
    assert slides >= 1 and count_slides(10, cut, W, keep) == 0       # the cache fills after W - 10 ids: the cut lies before it

    def begin():
        m._set_decode_grammar(0, gram, bans)
        _lib.check(lib.cmp_decode_begin_slide(h, p.ctypes.data_as(C.c_void_p), len(p), keep, 1.0, 4), "begin_slide")

    def steps(n):
        out = np.empty(n, np.int32)
        _lib.check(lib.cmp_decode_steps(h, n, out.ctypes.data_as(C.c_void_p)), "steps")
        return out

    begin()
    ref = steps(n_ids)
    begin()
    a = steps(cut)
    ragged = [r[:q] for r, q in zip(make_prompts(name, 3), (60, 50, 7))]
    ob = m.generate_batch(ragged, 2 * W, temperature=1.0, mode="kv-slide", slide_keep=keep, seed=9, grammar=other,
                          banned_ids=other_bans)                     # the batched chain in between, with its own grammar
    assert m.decode_slide_stats(batched=True)[0] == sum(count_slides(len(q), 2 * W, W, keep) for q in ragged)
    m(np.asarray(ragged[2], np.int32)[None])                         # and a forward pass
    b = steps(n_ids - cut)
    ids = np.concatenate([a, b])
    assert ids.tolist() == ref.tolist()
    assert not set(ids.tolist()) & set(bans)
    assert m.decode_grammar_state(batched=False) == gram.fold(p.tolist() + ids.tolist())
    assert m.decode_grammar_state(batched=True, row=2) == other.fold(ragged[2].tolist() + ob[2].tolist())
    assert m.decode_slide_stats() == (slides,) * 2
    m.close()


C5_STEPS = 40


def c5_prompts(B):
    W = GEOMS["c5"][3]
    rows = []
    for b in range(B):
        rng = np.random.default_rng([77, b])
        n = W - 20 if b % 8 != 5 else W - 20 - int(rng.integers(1, 9))     # most rows end 20 steps before the window's end
        rows.append(rng.integers(0, V, n).astype(np.int32))
    return rows


@pytest.mark.gpu
def test_c5_batch1_chain_slides_at_the_benchmark_size():
    name = "c5"
    keep = GEOMS[name][7]
    params = make_params(name)
    prompts = c5_prompts(2)[:1]
    m = make_model(name, params)
    ids, Z = hip_decode_one(m, prompts, 11, keep, C5_STEPS)
    assert slide_stats(m, False) == (1, 1)
    m.close()
    compare("c5 one keep=1024", name, params, prompts, ids, Z)


@pytest.mark.gpu
def test_c5_batch64_slides_at_the_benchmark_size():
    name = "c5"
    W, keep = GEOMS[name][3], GEOMS[name][7]
    params = make_params(name)
    prompts = c5_prompts(64)
    m = make_model(name, params, max_batch=4)            # 4 * W tokens: 8 rows of keep = 1024 per forward call
    ids, Z = hip_decode_batch(m, prompts, 11, keep, C5_STEPS)
    rs, fc = slide_stats(m, True)
    assert rs == 64 and fc < rs, (rs, fc)
    oracle_rows = [0, 5, 15, 16, 31, 32, 47, 63]
    for b in range(64):
        if b in oracle_rows:
            continue
        ids1, Z1 = hip_decode_batch(m, [prompts[b]], 11 + b, keep, C5_STEPS)
        assert ids1[0].tolist() == ids[b].tolist(), b
        assert np.array_equal(Z1[0].view(np.uint32), Z[b].view(np.uint32)), b
    m.close()
    compare("c5 batch B=64 keep=1024 (8 oracle rows)", name, params, [prompts[b] for b in oracle_rows], ids[oracle_rows], Z[oracle_rows])


# ---------------------------------------------------------------- CLI
NEAR_TIE = 1e-3     # logit units, as tests/test_gpu_cli.py: under it the oracle's top-2 margin counts as a tie the last bits may flip


def oracle_slide_greedy(orc, prompt, n_ids, W, keep):
    s = [int(t) for t in prompt]
    out = []
    for _ in range(n_ids):
        c = slide_context_length(len(s), W, keep)
        z = np.asarray(orc.forward(np.asarray(s[len(s) - c:])[None])[0])[0, -1]
        out.append(int(np.argmax(z)))
        s.append(out[-1])
    return out


def assert_greedy_identity(orc, prompt, ids, want, W, keep, what):
    """tests/test_gpu_cli.py's rule on the sliding context: identical position by position, with ONE checked exception -- at the
    first mismatch the oracle's own top-2 margin on the shared context is below NEAR_TIE and the HIP id is its runner-up."""
    assert len(ids) == len(want), (what, ids, want)
    for i, (a, b) in enumerate(zip(ids, want)):
        if a == b:
            continue
        s = list(prompt) + list(want[:i])
        c = slide_context_length(len(s), W, keep)
        z = np.asarray(orc.forward(np.asarray(s[len(s) - c:], dtype=np.int64)[None])[0])[0, -1]
        order = np.argsort(-z, kind="stable")
        margin = float(z[order[0]] - z[order[1]])
        assert int(order[0]) == b, (what, i)
        assert margin < NEAR_TIE and a == int(order[1]), (what, "first mismatch at position %d: HIP %d, oracle %d, margin %.3e"
                                                          % (i, a, b, margin))
        return i
    return len(ids)


@pytest.mark.gpu
def test_cli_generate_kv_slide(tmp_path):
    import yaml
    from click.testing import CliRunner
    from composer_amd import cli, dataset as D, checkpoint as ckpt
    W, keep, E, L, H = 32, 13, 64, 2, 4
    cfg = yaml.safe_load(open(cli.get_default_config()))
    cfg["transformer"]["model"].update(window_size=W, embedding_size=E, attention_head_count=H, decoder_layers_count=L,
                                       attention_dropout_rate=0.0, residual_dropout_rate=0.0, initializer_stddev=0.1)
    cfg["transformer"]["runtime"] = {"dtype": "fp32", "seed": 5}
    run = tmp_path / "run"
    run.mkdir()
    (run / "config.yml").write_text(yaml.safe_dump(cfg))
    params = {k: v.astype(np.float32) for k, v in O.init_params(V, E, W, L, seed=5, stddev=0.1).items()}
    ckpt.CheckpointManager(run).save({"model/" + k: v for k, v in params.items()}, {})
    D.write_synthetic_data_file(tmp_path / "p.data", 40, seed=22)
    prompt = D.read_data_file(tmp_path / "p.data")[0][:6].astype(int).tolist()
    orc = O.OracleTransformer(O.Config(V, E, W, L, H), params)
    r = CliRunner()
    base = ["generate", "transformer", str(run), str(tmp_path / "out.data"), "--prompt-data", str(tmp_path / "p.data"),
            "--prompt-length", "6", "--length", str(3 * W), "--temperature", "0", "--decode-mode", "kv-slide", "--slide-keep", str(keep)]
    res = r.invoke(cli.cli, base, catch_exceptions=False)
    assert res.exit_code == 0, res.output
    ids = [int(t) for t in res.output.strip().split("\n")[-1].split(",")]
    assert len(ids) == 3 * W
    assert_greedy_identity(orc, prompt, ids, oracle_slide_greedy(orc, prompt, 3 * W, W, keep), W, keep, "kv-slide")
    got_ids, _ = D.read_data_file(tmp_path / "out.data")
    assert got_ids.tolist() == prompt + ids
    res = r.invoke(cli.cli, base + ["--num-samples", "3"], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    lines = [l for l in res.output.strip().split("\n") if "," in l][-3:]
    for i in range(3):
        got_ids, _ = D.read_data_file(tmp_path / ("out-%d.data" % i))
        assert got_ids.tolist() == prompt + [int(t) for t in lines[i].split(",")]
        assert len(got_ids) == 6 + 3 * W
    # kv-cache still refuses what does not fit
    res = r.invoke(cli.cli, base[:-4] + ["--decode-mode", "kv-cache"])
    assert res.exit_code == 2


# ---------------------------------------------------------------- CPU: the bound is far below what a slide mistake does
FP32_SMALL = [n for n in GEOMS if GEOMS[n][5] == "fp32" and n != "c5"]
SENS_KEEPS = {"d16": (1, 48), "d32": (37,), "d32_noln": (48,), "d64": (95, 8), "d128": (37,), "pad24": (80, 159, 8)}


@pytest.mark.parametrize("name", FP32_SMALL)
def test_slide_mistakes_move_the_logits_by_ten_bounds(name):
    """Teacher-forced on random ids around the first slide of a full window, float64: the GPU test's bound (FACTOR * floor +
    1e-6 * max|z64|, the floor taken over the same logits) against the change of the logits when (a) the re-encoded tail starts one
    token early or late, (b) ONE cache row j < keep still holds the key / value position j had before the slide (j = 0, keep // 2,
    keep - 1; one step and (W - keep) // 2 steps after the slide), (c) the token consumed after the slide is given position
    keep - 1 or keep + 1.  Each must be at least 10x the bound; if one is not, the weight scale is wrong for this test."""
    params = make_params(name)
    W = GEOMS[name][3]
    o64, o32 = _oracle(name, params, "f64"), _oracle(name, params, "f32")
    rng = np.random.default_rng(3)
    for keep in SENS_KEEPS[name]:
        later = max(1, (W - keep) // 2)
        s = rng.integers(0, V, W + 1 + later).tolist()       # s[:W + 1]: the sequence at the first slide; then the ids fed after it
        n = W + 1
        tail = s[n - keep:n]

        def run(orc, tail, stale=None, pos_shift=0, nsteps=later):
            """logits of the slide, then of `nsteps` per-token steps on its presents"""
            z, past, _ = orc.forward(np.asarray(tail)[None])
            outs = [z[0, -1]]
            past = [np.array(a) for a in past]
            if stale is not None:
                old = orc.forward(np.asarray(s[:W])[None])[1]
                for a, b in zip(past, old):
                    a[:, :, :, stale, :] = b[:, :, :, stale, :]
            for i in range(nsteps):
                T = past[0].shape[-2]
                z, past, _ = orc.forward(np.array([[s[n + i]]]), past=past, position_ids=np.array([[T + (pos_shift if i == 0 else 0)]]))
                outs.append(z[0, -1])
            return np.stack(outs)

        ref = run(o64, tail)
        floor = float(np.abs(run(o32, tail).astype(np.float64) - ref).max())
        bound = FACTOR.get(name, 4) * floor + 1e-6 * float(np.abs(ref).max())
        ratios = {}
        for d in (-1, 1):                                    # (a) the window start off by one
            if keep - d < 1 or keep - d > W:
                continue
            ratios["start%+d" % d] = float(np.abs(run(o64, s[n - keep + d:n], nsteps=0)[0] - ref[0]).max()) / bound
        for j in sorted({0, keep // 2, keep - 1}):           # (b) one stale cache row
            z = run(o64, tail, stale=j)
            ratios["stale%d@1" % j] = float(np.abs(z[1] - ref[1]).max()) / bound
            ratios["stale%d@%d" % (j, later)] = float(np.abs(z[later] - ref[later]).max()) / bound
        for d in (-1, 1):                                    # (c) the token after the slide at position keep +- 1
            if keep + d > W - 1 or keep + d < 0:
                continue
            ratios["pos%+d" % d] = float(np.abs(run(o64, tail, pos_shift=d, nsteps=1)[1] - ref[1]).max()) / bound
        print("\n[decode-slide sensitivity] %-9s keep %3d floor %.3e bound %.3e change/bound %s"
              % (name, keep, floor, bound, {k: round(v, 1) for k, v in ratios.items()}))
        assert len(ratios) >= 8 or keep in (1, W - 1)
        assert min(ratios.values()) >= 10.0, (name, keep, floor, bound, ratios)
