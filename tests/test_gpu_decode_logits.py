"""Both per-token decode chains (decode.hip: dec_gemv2_kernel / dec_gemv_kernel / dec_attn2_kernel; decode_batch.hip:
decb_proj_kernel / decb_attn_kernel) against the float64 oracle, on whole logit rows, at every step, at long contexts.

The observable is cmp_decode_logits_get / cmp_decode_batch_logits_get: the logits the latest per-token step drew its id from.
One helper (`run_case`) decodes at temperature 1.0 with a fixed seed one step at a time, reads the logits after every step,
feeds the ids the HIP chain produced to `OracleTransformer.forward(..., past=...)` row by row (teacher forcing, so both sides see
the same context) and compares all V logits of every step of every row.

Bound (fp32 models).  floor = max |z32 - z64| of the float32 restatement of the oracle against the float64 oracle on the very
contexts of the case; the HIP logits must satisfy max |z_hip - z64| <= 4 * floor + 1e-6 * max |z64|.  Two correct fp32
evaluations with different summation orders each sit about one floor from float64, and the MFMA k-split, the split-key merge and
expf differ from numpy's order; the absolute term keeps a lucky, tiny floor from failing a correct kernel.
`test_a_dropped_key_moves_the_logits_by_ten_bounds` (CPU) keeps that bound honest: on every fp32 geometry, at the weight scale
used here, deleting ONE cached key (the newest, key 0, one in the middle) or 32 contiguous keys from the float64 oracle's `past`
moves the logits by at least 10x the bound -- so a kernel that drops a key, a wave's pass or a split's tail fails, where the
argmax ids of the older decode tests do not notice.  The weight scale (stddev 0.05; 0.06 on C5) keeps attention diffuse enough
for that; LayerNorm gains / offsets and the biases are perturbed away from 1 / 0 so that they matter.

bf16 model.  The per-token chain is fp32 on the fp32 master weights; only the caches hold bf16-rounded prefill K/V.  Two
references, both asserted.  (1) The plain float64 oracle at the project's bf16 logits tolerance, 3e-2 * max |z|
(test_gpu_model.py).  With diffuse attention that bound is some hundred times what the bf16 caches do to the logits, so
(2) the oracle with `emulate_bf16=True` for the prefill and plain float64 steps on its `past`.  It rounds where the forward pass
rounds, so it lines up except where an fp32-order difference in front of a rounding point flips a bf16 ulp of a cache entry --
too much for the fp32 bound, a fraction of the rounding itself.  Its bound is written from the two oracles alone:
effect = max |z_emulated - z64| is what bf16 caches do to these logits; a chain that fills its caches from the bf16 qkv must sit
closer to the emulation than half of that: err <= 0.5 * effect + (4 * floor + 1e-6 * max |z64|).

What each case is for (starting contexts: 1 -> three of the four key splits empty, -inf records through the combine; 12;
125 -> crosses chunk 32 -> 36, wave 1 gets its first keys: the cross-wave merge; 505 -> crosses pos + 1 = 512, wave 0 starts a
second pass: the online rescale; 1000; every row runs 40 consecutive steps, so every residue of pos + 1 mod 16 is met):
  d16, d32, d64, d128      the four attention instantiations of both chains (D = 128 had never run)
  d32_noln                 use_layer_norm = False in fp32: the IN = 0 projection prologue
  pad24                    E 96 / H 4: Dl 24 padded to D 32, Ea 128 != E; combine + c_proj at K = Ea
  e320                     K = 320: five 64-blocks over four waves in decb_proj; K = 1280: dec_gemv2's KI = 12 form
  e1024                    K = 4096: the dec_gemv_kernel fall-back in two passes; 16 k-blocks per wave in decb_proj
  c5                       E 512 / H 8 / L 6 / W 2048 (the benchmark's model; dec_gemv2's CW = 2 form), contexts up to the window's
                           end (the last step consumes position W - 1); B = 64: the oracle follows rows 0, 15, 16, 31, 32, 47, 48, 63
                           (both ends of every 16-row tile boundary), every other row is compared bitwise (ids and logits) with a
                           batch-of-one decode of the same prompt and seed + b
  bf16, bf16_noln          the caches filled from bf16 qkv
  B = 37                   three 16-row tiles, the last one partial; B = 1 and B = 5: one partial tile
  literal                  one token at position 0 per step, against generate_literal's contexts

Measured err / floor (max |z_hip - z64| over max |z32 - z64|; floors 3e-7 .. 5e-6 at max |z| 2.3 .. 14.7), MI355X, batch-1 chain /
batched chain:
  d16      1.26 (graph and no graph) / 1.42 (B = 37), 1.75 (B = 5, no graph)      d32      1.00 / 1.95
  d32_noln 0.93 / 1.32                                                             d64      1.17 / 1.12 (both without the graph)
  d128     1.23 / 1.40 (B = 5), 1.05 (B = 1)                                       pad24    1.26 / 1.26
  e320     0.66 / 1.06 (B = 37)                                                    e1024    0.95 / 1.15
  c5       0.72 (4 rows) / 1.88 (B = 64, 8 oracle rows; the other 56 rows bitwise a batch of one)
  literal  1.02 / 1.14
No geometry needs more than the factor 4.  bf16 (both chains alike): against float64 err 1.08e-3 with LayerNorm, 6.9e-4 without
(bound 3e-2 * max |z| = 1.4e-1 / 1.2e-1); against the emulated prefill err 1.5e-4 where the bf16 effect is 1.08e-3 (bound 5.5e-4)
with LayerNorm, 4.7e-5 where it is 6.9e-4 (bound 3.5e-4) without.
Mutation check (a scratch build, not kept): decb_attn_kernel's merge skipping wave 1's partial -> err / floor 28000 .. 36000 on
every batched case whose context passes 128 keys (d16, d32), while all of tests/test_gpu_decode_batch.py still passed.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import transformer_oracle as O

V = 390
STEPS = 40          # per-token steps per row: ids 1 .. 40 (id 0 is drawn from the prefill's logits)
CTX5 = (1, 12, 125, 505, 1000)
C5_ORACLE_ROWS = (0, 15, 16, 31, 32, 47, 48, 63)
C5_ORACLE_CTX = (1, 1500, 125, 505, 12, 1000, 2000, 2048 - STEPS)      # row 63: its last step consumes position W - 1

# name: E, H, L, W, stddev, dtype, use_layer_norm
GEOMS = {
    "d16": (64, 4, 2, 1088, 0.05, "fp32", True),
    "d32": (64, 2, 2, 1088, 0.05, "fp32", True),
    "d32_noln": (64, 2, 2, 1088, 0.05, "fp32", False),
    "d64": (128, 2, 2, 1088, 0.05, "fp32", True),
    "d128": (256, 2, 1, 1088, 0.05, "fp32", True),
    "pad24": (96, 4, 2, 1088, 0.05, "fp32", True),
    "e320": (320, 5, 1, 1088, 0.05, "fp32", True),
    "e1024": (1024, 8, 1, 1088, 0.05, "fp32", True),
    "c5": (512, 8, 6, 2048, 0.06, "fp32", True),
    "bf16": (128, 2, 2, 1088, 0.05, "bf16", True),
    "bf16_noln": (128, 2, 2, 1088, 0.05, "bf16", False),
}
# err <= FACTOR * floor + 1e-6 * max|z64|; 4 unless a measured, explained ordering effect needs more on one geometry
FACTOR = {}
BF16_TOL = 3e-2


def make_params(name):
    """O.init_params at the geometry's weight scale, cast to float32; gamma / beta / biases moved off 1 / 0"""
    E, H, L, W, s, _, _ = GEOMS[name]
    p = O.init_params(V, E, W, L, seed=sorted(GEOMS).index(name) + 40, stddev=s)
    rng = np.random.default_rng(7)
    for n, _, kind in O.param_specs(V, E, W, L):
        if kind == "ones":
            p[n] = p[n] + 0.05 * rng.standard_normal(p[n].shape)
        elif kind == "zeros":
            p[n] = p[n] + 0.02 * rng.standard_normal(p[n].shape)
    return {k: v.astype(np.float32) for k, v in p.items()}


def make_prompts(name, B):
    """ragged rows: a row's key-split geometry differs from its neighbours'"""
    W = GEOMS[name][3]
    if name == "c5":
        lens = {b: c for b, c in zip(C5_ORACLE_ROWS, C5_ORACLE_CTX)}
        bands = ((1, 4), (8, 17), (120, 141), (500, 531), (960, 1041), (1480, 1521), (1990, W - STEPS + 1))
    else:
        lens = {b: c for b, c in enumerate(CTX5)} if B > 1 else {0: 505}
        bands = ((1, 4), (8, 17), (120, 141), (500, 531), (960, 1041))
    rows = []
    for b in range(B):
        rng = np.random.default_rng([sorted(GEOMS).index(name), b])
        lo, hi = bands[b % len(bands)]
        n = lens.get(b, int(rng.integers(lo, hi)))
        rows.append(rng.integers(0, V, n).astype(np.int32))
    return rows


def oracle_config(name):
    E, H, L, W, _, _, use_ln = GEOMS[name]
    return O.Config(V, E, W, L, H, use_layer_normalization=use_ln)


# ---------------------------------------------------------------- the HIP side: ids [B, STEPS + 1], logits [B, STEPS, V]
def hip_decode_one(m, prompts, seed, mode, n=STEPS):
    """the batch-1 chain (decode.hip), row b with seed + b"""
    from composer_amd import _lib
    lib, h = m._lib, m._h
    ids = np.zeros((len(prompts), n + 1), np.int32)
    Z = np.zeros((len(prompts), n, V), np.float32)
    one = np.zeros(1, np.int32)
    for b, p in enumerate(prompts):
        p = np.ascontiguousarray(p, np.int32)
        _lib.check(lib.cmp_decode_begin(h, p.ctypes.data_as(C.c_void_p), len(p), mode, 1.0, seed + b), "begin")
        for k in range(n + 1):
            _lib.check(lib.cmp_decode_steps(h, 1, one.ctypes.data_as(C.c_void_p)), "steps")
            ids[b, k] = one[0]
            if k:
                _lib.check(lib.cmp_decode_logits_get(h, Z[b, k - 1].ctypes.data_as(C.c_void_p)), "logits")
    return ids, Z


def hip_decode_batch(m, prompts, seed, mode, n=STEPS):
    """the batched chain (decode_batch.hip)"""
    from composer_amd import _lib
    lib, h = m._lib, m._h
    B, ld = len(prompts), max(len(p) for p in prompts)
    buf = np.zeros((B, ld), np.int32)
    for b, p in enumerate(prompts):
        buf[b, :len(p)] = p
    lens = np.array([len(p) for p in prompts], np.int32)
    _lib.check(lib.cmp_decode_batch_begin(h, buf.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), B, ld, mode, 1.0,
                                          seed), "begin")
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


def make_model(name, params):
    from composer_amd.transformer import Transformer
    E, H, L, W, _, dtype, use_ln = GEOMS[name]
    m = Transformer(V, E, W, L, H, attention_dropout_rate=0.0, residual_dropout_rate=0.0, use_layer_normalization=use_ln,
                    dtype=dtype, seed=0, max_batch=1, max_seq=W)
    m.set_weights(params)
    return m


# ---------------------------------------------------------------- the oracle side
_PREFILL = {}       # (geometry, oracle kind, prompt) -> past; the cases of one geometry share prompts


def _oracle(name, params, kind):
    if kind == "f64":
        return O.OracleTransformer(oracle_config(name), {k: v.astype(np.float64) for k, v in params.items()})
    if kind == "f32":
        return O.OracleTransformer(oracle_config(name), params, dtype=np.float32)
    return O.OracleTransformer(oracle_config(name), {k: v.astype(np.float64) for k, v in params.items()}, emulate_bf16=True)


def oracle_logits(name, params, kind, prompts, ids, literal=False):
    """[R, STEPS, V]: step k of row r consumes ids[r, k] (the id the HIP chain drew) after prompts[r] + ids[r, :k].
    kind "f64" / "f32": that float type throughout; "bf16fill": prefill with emulate_bf16, the steps in plain float64."""
    if _PREFILL and next(iter(_PREFILL))[0] != name:
        _PREFILL.clear()
    step_orc = _oracle(name, params, "f64" if kind == "bf16fill" else kind)
    out = np.zeros((len(prompts), ids.shape[1] - 1, V), np.float64)
    for r, p in enumerate(prompts):
        past = None
        if not literal:
            key = (name, kind, tuple(int(t) for t in p))
            if key not in _PREFILL:
                _PREFILL[key] = _oracle(name, params, kind).forward(np.asarray(p)[None])[1]
            past = [np.asarray(a, step_orc.dtype) for a in _PREFILL[key]]
        for k in range(ids.shape[1] - 1):
            logits, pres, _ = step_orc.forward(np.array([[int(ids[r, k])]]), past=past)
            out[r, k] = logits[0, -1]
            if not literal:
                past = pres
    return out


def compare(label, name, params, prompts, ids, Z, literal=False):
    assert np.isfinite(Z).all(), label
    assert ids.min() >= 0 and ids.max() < V
    z64 = oracle_logits(name, params, "f64", prompts, ids, literal)
    z32 = oracle_logits(name, params, "f32", prompts, ids, literal)
    floor = float(np.abs(z32 - z64).max())
    zmax = float(np.abs(z64).max())
    d = np.abs(Z - z64)
    err = float(d.max())
    r, k = [int(t) for t in np.unravel_index(np.argmax(d.max(-1)), d.shape[:2])]
    worst = "worst at row %d (prompt %d ids) step %d" % (r, len(prompts[r]), k + 1)
    if GEOMS[name][5] == "bf16":
        bound = BF16_TOL * zmax
        zem = oracle_logits(name, params, "bf16fill", prompts, ids, literal)
        err_em = float(np.abs(Z - zem).max())
        effect = float(np.abs(zem - z64).max())             # what bf16 caches do to the logits, from the two oracles alone
        bound_em = 0.5 * effect + 4 * floor + 1e-6 * zmax
        extra = "; against the emulate_bf16 prefill: err %.3e, bf16 effect %.3e, bound %.3e" % (err_em, effect, bound_em)
    else:
        bound = FACTOR.get(name, 4) * floor + 1e-6 * zmax
        extra = ""
    print("\n[decode-logits] %-34s err %.3e floor %.3e err/floor %6.2f bound %.3e max|z| %.3f %s%s"
          % (label, err, floor, err / floor, bound, zmax, worst, extra))
    assert err <= bound, (label, err, floor, err / floor, bound, worst)
    if extra:
        assert err_em <= bound_em, (label, err_em, effect, bound_em)


def run_case(monkeypatch, name, chain, B, graph=True, literal=False, seed=11):
    from composer_amd import _lib
    monkeypatch.setenv("COMPOSER_NO_GRAPH", "0" if graph else "1")
    params = make_params(name)
    prompts = make_prompts(name, B)
    m = make_model(name, params)
    mode = _lib.DECODE_LITERAL if literal else _lib.DECODE_KV
    ids, Z = (hip_decode_one if chain == "one" else hip_decode_batch)(m, prompts, seed, mode)
    m.close()
    label = "%s %s B=%d%s%s" % (name, chain, B, "" if graph else " nograph", " literal" if literal else "")
    compare(label, name, params, prompts, ids, Z, literal)


CASES = [
    # geometry, chain, B, graph
    ("d16", "one", 5, True), ("d16", "one", 5, False), ("d16", "batch", 37, True), ("d16", "batch", 5, False),
    ("d32", "one", 5, True), ("d32", "batch", 5, True),
    ("d32_noln", "one", 5, True), ("d32_noln", "batch", 5, True),
    ("d64", "one", 5, False), ("d64", "batch", 5, False),
    ("d128", "one", 5, True), ("d128", "batch", 5, True), ("d128", "batch", 1, True),
    ("pad24", "one", 5, True), ("pad24", "batch", 5, True),
    ("e320", "one", 5, True), ("e320", "batch", 37, True),
    ("e1024", "one", 5, True), ("e1024", "batch", 5, True),
    ("bf16", "one", 5, True), ("bf16", "batch", 5, True),
    ("bf16_noln", "one", 5, True), ("bf16_noln", "batch", 5, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,chain,B,graph", CASES, ids=["%s-%s-B%d-%s" % (n, c, b, "graph" if g else "nograph")
                                                          for n, c, b, g in CASES])
def test_logits_follow_the_oracle(name, chain, B, graph, monkeypatch):
    run_case(monkeypatch, name, chain, B, graph)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", ["one", "batch"])
def test_literal_mode_logits_follow_the_oracle(chain, monkeypatch):
    """mode literal: every step feeds ONE token at position 0 without a cache (generate_literal's contexts)"""
    run_case(monkeypatch, "d16", chain, 5, literal=True)


@pytest.mark.gpu
def test_c5_batch64_logits_follow_the_oracle(monkeypatch):
    from composer_amd import _lib
    name = "c5"
    params = make_params(name)
    prompts = make_prompts(name, 64)
    assert max(len(p) for p in prompts) == 2048 - STEPS
    m = make_model(name, params)
    seed = 11
    ids, Z = hip_decode_batch(m, prompts, seed, _lib.DECODE_KV)
    rest = [b for b in range(64) if b not in C5_ORACLE_ROWS]
    for b in rest:                                   # the row-independence contract: bitwise a batch of one with seed + b
        ids1, Z1 = hip_decode_batch(m, [prompts[b]], seed + b, _lib.DECODE_KV)
        assert ids1[0].tolist() == ids[b].tolist(), b
        assert np.array_equal(Z1[0].view(np.uint32), Z[b].view(np.uint32)), b
    m.close()
    rows = list(C5_ORACLE_ROWS)
    compare("c5 batch B=64 (8 oracle rows)", name, params, [prompts[b] for b in rows], ids[rows], Z[rows])


@pytest.mark.gpu
def test_c5_batch1_chain_logits_follow_the_oracle(monkeypatch):
    """the benchmark's chain at the benchmark's size and beyond: contexts 505, 1000, 1500 and the end of the window"""
    from composer_amd import _lib
    name = "c5"
    params = make_params(name)
    allp = make_prompts(name, 64)
    rows = [31, 47, 15, 63]
    prompts = [allp[b] for b in rows]
    assert [len(p) for p in prompts] == [505, 1000, 1500, 2048 - STEPS]
    m = make_model(name, params)
    ids, Z = hip_decode_one(m, prompts, 11, _lib.DECODE_KV)
    m.close()
    compare("c5 one (4 rows)", name, params, prompts, ids, Z)


@pytest.mark.gpu
def test_accessors_refuse_before_the_first_step_and_keep_the_last_steps_logits():
    from composer_amd import _lib
    name = "d16"
    m = make_model(name, make_params(name))
    lib, h = m._lib, m._h
    z = np.zeros(V, np.float32)
    zb = np.zeros((2, V), np.float32)
    one = np.zeros(4, np.int32)
    assert lib.cmp_decode_logits_get(h, z.ctypes.data_as(C.c_void_p)) == -4 and "begin" in _lib.last_error()
    assert lib.cmp_decode_batch_logits_get(h, zb.ctypes.data_as(C.c_void_p)) == -4 and "begin" in _lib.last_error()
    p = np.array([5, 6, 7], np.int32)
    _lib.check(lib.cmp_decode_begin(h, p.ctypes.data_as(C.c_void_p), 3, _lib.DECODE_KV, 1.0, 3))
    assert lib.cmp_decode_logits_get(h, z.ctypes.data_as(C.c_void_p)) == -4 and "step" in _lib.last_error()
    _lib.check(lib.cmp_decode_steps(h, 1, one.ctypes.data_as(C.c_void_p)))      # the prefill's id: still no per-token step
    assert lib.cmp_decode_logits_get(h, z.ctypes.data_as(C.c_void_p)) == -4
    buf = np.array([[5, 6, 7], [8, 9, 0]], np.int32)
    lens = np.array([3, 2], np.int32)
    _lib.check(lib.cmp_decode_batch_begin(h, buf.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), 2, 3, _lib.DECODE_KV,
                                          1.0, 3))
    assert lib.cmp_decode_batch_logits_get(h, zb.ctypes.data_as(C.c_void_p)) == -4 and "step" in _lib.last_error()
    # steps(n) leaves the logits of its last step, and the Python wrappers read the same rows
    ids1, Z1 = hip_decode_one(m, [p], 3, _lib.DECODE_KV, n=3)
    assert m.generate(p, 4, temperature=1.0, mode="kv", seed=3).tolist() == ids1[0].tolist()
    assert np.array_equal(m.decode_logits(), Z1[0, 2])
    idsb, Zb = hip_decode_batch(m, [buf[0], buf[1, :2]], 3, _lib.DECODE_KV, n=3)
    assert m.generate_batch([buf[0], buf[1, :2]], 4, temperature=1.0, mode="kv", seed=3).tolist() == idsb.tolist()
    assert np.array_equal(m.decode_batch_logits(), Zb[:, 2])
    assert idsb[0].tolist() != idsb[1].tolist()
    # ... and they are the logits the ids were drawn from: the chain's sampler on them (seed + b, draw counter k) returns the ids
    import torch
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    got = torch.empty(1, dtype=torch.int32, device="cuda")
    for Zs, idss in ((Z1, ids1), (Zb, idsb)):
        for b in range(len(idss)):
            for k in range(1, 4):
                zd = torch.from_numpy(Zs[b, k - 1]).cuda()
                _lib.check(lib.cmp_k_sample(stream, C.c_void_p(zd.data_ptr()), V, 1.0, 3 + b, k, 1, C.c_void_p(got.data_ptr())))
                torch.cuda.synchronize()
                assert int(got[0]) == int(idss[b, k]), (b, k)
    m.close()


# ---------------------------------------------------------------- CPU: the bound is far below what a dropped key does
FP32_GEOMS = [n for n in GEOMS if GEOMS[n][5] == "fp32"]


@pytest.mark.parametrize("name", FP32_GEOMS)
def test_a_dropped_key_moves_the_logits_by_ten_bounds(name):
    """At the geometry's longest starting context, teacher-forced on random ids for a few steps: the GPU test's bound
    (FACTOR * floor + 1e-6 * max|z64|, the floor taken over those steps) against the change of the float64 logits when `past`
    loses (a) the newest cached key, (b) key 0, (c) one key in the middle, (d) 32 contiguous keys -- the new token keeps its
    position.  Each must be at least 10x the bound; if one is not, the weight scale is wrong for this test, not the condition."""
    params = make_params(name)
    ctx = 2048 - STEPS if name == "c5" else 1000
    nsteps = 8
    rng = np.random.default_rng(3)
    prompt = rng.integers(0, V, ctx)
    ids = rng.integers(0, V, (1, nsteps + 1)).astype(np.int32)
    z64 = oracle_logits(name, params, "f64", [prompt], ids)
    z32 = oracle_logits(name, params, "f32", [prompt], ids)
    _PREFILL.clear()
    floor = float(np.abs(z32 - z64).max())
    bound = FACTOR.get(name, 4) * floor + 1e-6 * float(np.abs(z64).max())
    orc = _oracle(name, params, "f64")
    past = orc.forward(np.concatenate([prompt, ids[0, :nsteps - 1]])[None])[1]
    T = past[0].shape[-2]
    assert T == ctx + nsteps - 1
    tok, pos = np.array([[int(ids[0, nsteps - 1])]]), np.array([[T]])
    full = orc.forward(tok, past=past, position_ids=pos)[0][0, -1]
    assert np.abs(full - z64[0, nsteps - 1]).max() <= 1e-9
    mid = (T // 2) & ~31
    ratios = {}
    for what, gone in (("newest", [T - 1]), ("key 0", [0]), ("middle", [T // 2 + 5]), ("32 keys", list(range(mid, mid + 32)))):
        keep = np.setdiff1d(np.arange(T), gone)
        cut = orc.forward(tok, past=[a[:, :, :, keep, :] for a in past], position_ids=pos)[0][0, -1]
        ratios[what] = float(np.abs(cut - full).max()) / bound
    print("\n[decode-logits sensitivity] %-9s floor %.3e bound %.3e change/bound %s"
          % (name, floor, bound, {k: round(v, 1) for k, v in ratios.items()}))
    assert min(ratios.values()) >= 10.0, (name, floor, bound, ratios)
