"""-m gpu: global-norm gradient clipping and gradient accumulation of the train step (cmp_train_options), at kernel level and through
the Transformer class, against the float64 oracle.

Contract (include/composer_hip.h): N ranks, k = accum_steps; G = the flat fp32 gradient buffer after the last micro-batch of an
optimiser step and after the all-reduce (the SUM over micro-batches and ranks); gscale = 1/(k*N); norm = gscale * sqrt(sum G^2) in
float64; scale = 1 if norm <= clip_norm else clip_norm / norm; Adam multiplies every gradient element by factor = gscale * scale.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from oracle import golden, transformer_oracle as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CMP_ERR_INVALID = -1


def load_golden(name):
    g = golden.load(os.path.join(HERE, "golden", "transformer_%s.npz" % name))
    V, E, H, L, W, T, B = [int(v) for v in g["cfg"]]
    params = {k[6:]: g[k] for k in g.files if k.startswith("param:")}
    return g, (V, E, H, L, W, T, B), params


def make_model(cfg, params, dtype, p_attn=0.0, p_resid=0.0, seed=0, use_ln=True, max_batch=None):
    from composer_amd.transformer import Transformer
    V, E, H, L, W, T, B = cfg
    m = Transformer(V, E, W, L, H, attention_dropout_rate=p_attn, residual_dropout_rate=p_resid,
                    use_layer_normalization=use_ln, dtype=dtype, seed=seed, max_batch=max_batch or B, max_seq=W)
    m.set_weights(params)
    return m


@pytest.fixture(scope="module")
def lib():
    from composer_amd import _lib
    l = _lib.load()
    _lib.require_gpu()
    return l


def ck(lib, rc):
    assert rc == 0, lib.cmp_last_error().decode()


def P(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def grad_clip(lib, g_dev, gscale, clip):
    """cmp_k_grad_clip on a device tensor -> (norm float64, scale float32, factor float32, the 8 norm bytes)"""
    n = g_dev.numel()
    ws = torch.empty(max(1, lib.cmp_k_grad_clip_ws(n) // 8), dtype=torch.float64, device="cuda")
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    ck(lib, lib.cmp_k_grad_clip(stream(), P(g_dev), n, gscale, clip, P(ws), P(out)))
    torch.cuda.synchronize()
    raw = out.cpu().numpy().tobytes()
    return (np.frombuffer(raw[:8], np.float64)[0], np.frombuffer(raw[8:12], np.float32)[0], np.frombuffer(raw[12:16], np.float32)[0],
            raw[:8])


def norm_ref(g, gscale):
    return gscale * math.sqrt(float((g.astype(np.float64) ** 2).sum()))


# ------------------------------------------------------------------------------------------------ 1. kernels against float64
@pytest.mark.parametrize("n", [4, 8, 1020, 65540, 1000004])
def test_norm_kernel_against_float64(lib, n):
    """norm against gscale * sqrt(sum g^2) in float64 to n * 2^-52 relative: the rounding bound for ANY order of a sum of n
    non-negative doubles (each fma and each add rounds once), so derived, not measured.  A second call returns the same bytes."""
    g = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    gd = torch.as_tensor(g).cuda()
    ref = norm_ref(g, 0.25)
    norm, scale, factor, raw = grad_clip(lib, gd, 0.25, math.inf)
    print("n", n, "norm", norm, "ref", ref, "rel", abs(norm - ref) / ref)
    assert abs(norm - ref) <= n * 2.0 ** -52 * ref
    assert scale == np.float32(1.0) and factor == np.float32(0.25)
    assert grad_clip(lib, gd, 0.25, math.inf)[3] == raw


def test_norm_kernel_where_an_fp32_accumulation_fails(lib):
    n = 1024
    tiny = np.full(n, 1e-30, np.float32)                    # the squares underflow in fp32
    norm = grad_clip(lib, torch.as_tensor(tiny).cuda(), 1.0, math.inf)[0]
    ref = norm_ref(tiny, 1.0)
    print("tiny norm", norm, "ref", ref)
    assert abs(ref - 3.2e-29) <= 1e-6 * 3.2e-29 and abs(norm - ref) <= n * 2.0 ** -52 * ref
    big = np.full(n, 3e19, np.float32)                      # the sum of squares passes the fp32 maximum
    big[1::2] *= -1
    norm = grad_clip(lib, torch.as_tensor(big).cuda(), 1.0, math.inf)[0]
    ref = norm_ref(big, 1.0)
    print("big norm", norm, "ref", ref)
    assert math.isfinite(norm) and abs(norm - ref) <= n * 2.0 ** -52 * ref


def test_clip_scale_and_factor(lib):
    from composer_amd.transformer import clip_scale
    g = np.random.default_rng(3).standard_normal(65540).astype(np.float32)
    gd = torch.as_tensor(g).cuda()
    gscale = 0.25
    norm = grad_clip(lib, gd, gscale, math.inf)[0]
    n2, scale, factor, _ = grad_clip(lib, gd, gscale, float(np.float32(2 * norm)))           # clip above the norm
    assert n2 == norm and scale == np.float32(1.0) and factor == np.float32(gscale)
    clip = float(np.float32(0.5 * norm))                                                      # clip below it
    n3, scale, factor, _ = grad_clip(lib, gd, gscale, clip)
    want = np.float32(clip / norm)
    assert n3 == norm and abs(float(scale) - float(want)) <= float(np.spacing(want))
    assert abs(float(scale) - clip_scale(norm, clip)) <= 2 * float(np.spacing(want))
    assert factor == np.float32(gscale) * scale


def test_adam_with_a_device_factor_equals_adam_with_grad_scale(lib):
    n = 4096
    rng = np.random.default_rng(11)
    f = np.float32(0.1234567)
    base = [torch.as_tensor(rng.standard_normal(n).astype(np.float32)).cuda() for _ in range(2)]       # p, g
    base += [torch.as_tensor(np.abs(rng.standard_normal(n)).astype(np.float32) * 1e-2).cuda() for _ in range(2)]   # m, v
    fd = torch.as_tensor(np.array([f], np.float32)).cuda()
    res = []
    for dev in (False, True):
        p, g, m, v = [t.clone() for t in base]
        sh = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
        if dev:
            ck(lib, lib.cmp_k_adam_dev(stream(), P(p), P(g), P(m), P(v), P(sh), n, 1e-3, 0.9, 0.999, 1e-7, 3, P(fd)))
        else:
            ck(lib, lib.cmp_k_adam(stream(), P(p), P(g), P(m), P(v), P(sh), n, 1e-3, 0.9, 0.999, 1e-7, 3, float(f)))
        torch.cuda.synchronize()
        res.append([t.cpu().numpy().tobytes() for t in (p, m, v)] + [sh.view(torch.int16).cpu().numpy().tobytes()])
    assert res[0] == res[1]
    assert res[0][0] != base[0].cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ oracle restatement
def oracle_for(cfg, params, **kw):
    V, E, H, L, W, T, B = cfg
    return O.OracleTransformer(O.Config(V, E, W, L, H, **kw), {k: v.astype(np.float64) for k, v in params.items()})


def global_norm(G):
    return math.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in G.values()))


def oracle_clipped_step(orc, x, y, lr, clip):
    """loss, norm, scale of one clipped step; the oracle's state advances"""
    from composer_amd.transformer import clip_scale
    loss, acc, G, _ = orc.loss_and_grads(x, y, training=False, step=orc.iterations)
    norm = global_norm(G)
    scale = clip_scale(norm, clip)
    orc.adam_step({k: v * scale for k, v in G.items()}, lr)
    return loss, norm, scale


_ORACLE_RUNS = {}


def oracle_run(name, clip, steps):
    """computed once, shared, never modified: per step (loss, norm, scale), the Adam slots after step 1, the parameters after step 3"""
    key = (name, clip, steps)
    if key not in _ORACLE_RUNS:
        g, cfg, params = load_golden(name)
        orc = oracle_for(cfg, params)
        rec, m1, v1, p3 = [], None, None, None
        for s in range(steps):
            rec.append(oracle_clipped_step(orc, g["x"][s], g["y"][s], float(g["lr"]), clip))
            if s == 0:
                m1, v1 = {k: v.copy() for k, v in orc.m.items()}, {k: v.copy() for k, v in orc.v.items()}
            if s == 2:
                p3 = {k: v.copy() for k, v in orc.p.items()}
        _ORACLE_RUNS[key] = (rec, m1, v1, p3)
    return _ORACLE_RUNS[key]


# ------------------------------------------------------------------------------------------------ 2. clipped steps
@pytest.mark.parametrize("name, clip", [("gA", 0.7), ("gB", 0.7), ("gC", 0.5)])
def test_clipped_steps_match_the_oracle(name, clip):
    """The oracle's norms over three clipped steps are 1.387-1.401 (gA), 1.400-1.415 (gB), 1.032-1.057 (gC): the clip binds on every
    step with about 2x margin.  Adam's first parameter update barely depends on the gradient's scale, so it is m (5e-4 of its
    largest entry, the gradient tolerance) and v (1e-3: quadratic) after step 1 that catch a missing or wrong scale."""
    from composer_amd import _lib
    g, cfg, params = load_golden(name)
    rec, m1, v1, p3 = oracle_run(name, clip, 3)
    m = make_model(cfg, params, "fp32")
    m.set_train_options(clip_norm=clip)
    assert m.train_options() == {"clip_norm": pytest.approx(clip), "accumulate_steps": 1, "pending_micro_steps": 0}
    for s in range(3):
        loss, _ = m.train_step(g["x"][s], g["y"][s], float(g["lr"]))
        norm, scale = m.grad_stats()
        oloss, onorm, oscale = rec[s]
        print(name, "step", s, "loss", loss, oloss, "norm", norm, onorm, "scale", scale, oscale)
        assert oscale < 1.0
        assert abs(loss - oloss) <= 1e-4 * abs(oloss)
        assert norm is not None and abs(norm - onorm) <= 2e-4 * onorm
        assert abs(scale - oscale) <= 3e-4 * oscale
        if s == 0:
            for n in m.parameter_names:
                am, av = m.get_parameter(n, _lib.KIND_ADAM_M), m.get_parameter(n, _lib.KIND_ADAM_V)
                assert np.abs(am - m1[n]).max() <= 5e-4 * np.abs(m1[n]).max() + 1e-12, n
                assert np.abs(av - v1[n]).max() <= 1e-3 * np.abs(v1[n]).max() + 1e-15, n
    for n in m.parameter_names:
        assert np.abs(m.get_parameter(n) - p3[n]).max() <= 2e-5, n
    assert m.iterations == 3
    m.close()


# ------------------------------------------------------------------------------------------------ 3. the branch
def test_clip_binds_on_some_steps_only():
    """gB at clip 1.406: the oracle's norms are 1.41121, 1.40022, 1.41516, 1.41425 -- steps 0, 2, 3 bind, step 1 does not, each at
    least 0.37 % from the clip (18x the 2e-4 norm tolerance)."""
    g, cfg, params = load_golden("gB")
    rec, _, _, p3 = oracle_run("gB", 1.406, 4)
    assert [r[2] < 1.0 for r in rec] == [True, False, True, True]
    assert all(abs(r[1] - 1.406) >= 0.0037 * 1.406 for r in rec)
    m = make_model(cfg, params, "fp32")
    m.set_train_options(clip_norm=1.406)
    for s in range(4):
        m.train_step(g["x"][s], g["y"][s], float(g["lr"]))
        norm, scale = m.grad_stats()
        print("step", s, "norm", norm, rec[s][1], "scale", scale, rec[s][2])
        assert abs(norm - rec[s][1]) <= 2e-4 * rec[s][1]
        if s == 1:
            assert scale == 1.0
        else:
            assert scale < 1.0 and abs(scale - rec[s][2]) <= 3e-4 * rec[s][2]
        if s == 2:
            for n in m.parameter_names:
                assert np.abs(m.get_parameter(n) - p3[n]).max() <= 2e-5, n
    m.close()


# ------------------------------------------------------------------------------------------------ 4. a clip that never binds
def test_a_clip_that_never_binds_changes_no_bit(monkeypatch):
    """COMPOSER_DETERMINISTIC=1 (no float atomics: bitwise reproducible steps), bf16, gB, three steps: clip_norm = inf multiplies by the
    same factor from device memory that the default step passes by value.  The norm it reports is within 3e-2 of the oracle's
    (the bf16 tolerance of the loss checks)."""
    from composer_amd import _lib
    monkeypatch.setenv("COMPOSER_DETERMINISTIC", "1")
    g, cfg, params = load_golden("gB")
    orc = oracle_for(cfg, params)
    onorms = [oracle_clipped_step(orc, g["x"][s], g["y"][s], float(g["lr"]), math.inf)[1] for s in range(3)]
    state = []
    for clip in (math.inf, 0.0):
        m = make_model(cfg, params, "bf16")
        if clip:
            m.set_train_options(clip_norm=clip)
        for s in range(3):
            m.train_step(g["x"][s], g["y"][s], float(g["lr"]))
            norm, scale = m.grad_stats()
            if clip:
                print("step", s, "norm", norm, onorms[s])
                assert norm is not None and math.isfinite(norm) and abs(norm - onorms[s]) <= 3e-2 * onorms[s] and scale == 1.0
            else:
                assert norm is None and scale == 1.0
        state.append({(n, k): m.get_parameter(n, k).tobytes() for n in m.parameter_names
                      for k in (_lib.KIND_VALUE, _lib.KIND_ADAM_M, _lib.KIND_ADAM_V)})
        m.close()
    assert state[0] == state[1]


# ------------------------------------------------------------------------------------------------ 5. accumulation
ACC_CFG = (390, 64, 4, 2, 40, 40)          # V, E, H, L, W, T


def accum_setup(seed, B):
    V, E, H, L, W, T = ACC_CFG
    params = {k: v.astype(np.float32) for k, v in O.init_params(V, E, W, L, seed=seed).items()}
    rng = np.random.default_rng(seed + 1)
    for k in params:
        if k.endswith(("gamma", "beta", "bias")):
            params[k] = (params[k] + 0.05 * rng.standard_normal(params[k].shape)).astype(np.float32)
    x, y = O.synthetic_batch(rng, V, 2 * B, T)
    return params, np.ascontiguousarray(x.astype(np.int32)), np.ascontiguousarray(y.astype(np.int32))


def snapshot(m):
    from composer_amd import _lib
    return {(n, k): m.get_parameter(n, k).tobytes() for n in m.parameter_names for k in (_lib.KIND_VALUE, _lib.KIND_ADAM_M, _lib.KIND_ADAM_V)}


def test_accumulated_step_matches_the_oracle_on_the_whole_batch():
    from composer_amd import _lib
    V, E, H, L, W, T = ACC_CFG
    B = 3
    params, x, y = accum_setup(31, B)
    cfg = (V, E, H, L, W, T, B)
    orc = oracle_for(cfg, params)
    oloss, _, OG, _ = orc.loss_and_grads(x, y, training=False, step=0)
    m = make_model(cfg, params, "fp32")
    m.set_train_options(accumulate_steps=2)
    before = snapshot(m)
    l1, _ = m.train_step(x[:B], y[:B], 1e-3)
    assert m.iterations == 0 and snapshot(m) == before
    assert m.train_options()["pending_micro_steps"] == 1 and m.grad_stats() == (None, 1.0)
    l2, _ = m.train_step(x[B:], y[B:], 1e-3)
    assert m.iterations == 1 and m.train_options()["pending_micro_steps"] == 0
    assert abs(0.5 * (l1 + l2) - oloss) <= 1e-5 * abs(oloss)
    for n in m.parameter_names:
        big = np.abs(OG[n]).max()
        G = m.get_parameter(n, _lib.KIND_GRAD).astype(np.float64)
        assert np.abs(0.5 * G - OG[n]).max() <= 5e-4 * big + 1e-12, n
        assert np.abs(m.get_parameter(n, _lib.KIND_ADAM_M) - 0.1 * OG[n]).max() <= 5e-4 * 0.1 * big + 1e-12, n
    # inside a group every micro-step has the shape of the first
    m.train_step(x[:B], y[:B], 1e-3)
    assert m.train_options()["pending_micro_steps"] == 1
    xs, ys = np.ascontiguousarray(x[:2]), np.ascontiguousarray(y[:2])
    loss, acc = C.c_float(), C.c_float()
    rc = m._lib.cmp_train_step(m._h, xs.ctypes.data_as(C.c_void_p), ys.ctypes.data_as(C.c_void_p), 2, T, 1e-3, C.byref(loss), C.byref(acc))
    assert rc == CMP_ERR_INVALID and "shape" in _lib.last_error()
    xt, yt = np.ascontiguousarray(x[:B, :T - 8]), np.ascontiguousarray(y[:B, :T - 8])
    tk = C.c_int64()
    rc = m._lib.cmp_train_step_async(m._h, xt.ctypes.data_as(C.c_void_p), yt.ctypes.data_as(C.c_void_p), B, T - 8, 1e-3, C.byref(tk))
    assert rc == CMP_ERR_INVALID
    assert m.train_options()["pending_micro_steps"] == 1 and m.iterations == 1
    m.set_train_options(accumulate_steps=2)                   # discards the pending group
    assert m.train_options()["pending_micro_steps"] == 0
    # bad options are refused
    for clip, k in ((-1.0, 1), (math.nan, 1), (0.0, 0)):
        assert m._lib.cmp_train_options(m._h, clip, k) == CMP_ERR_INVALID
    assert m.train_options() == {"clip_norm": 0.0, "accumulate_steps": 2, "pending_micro_steps": 0}
    m.close()


# ------------------------------------------------------------------------------------------------ 6. accumulation masks
@pytest.mark.parametrize("dtype, geom, B, tol", [("fp32", ACC_CFG, 3, 2e-5), ("bf16", (390, 512, 8, 2, 256, 256), 2, 2e-3)])
def test_micro_steps_draw_the_masks_of_a_k_rank_job(dtype, geom, B, tol):
    """Dropout 0.1: micro-step j of a group of k draws the masks of mask rank r * k + j, so G after two micro-steps is the sum of two
    cmp_loss_and_grads calls taken with mask ranks 0 and 1 on the two halves (fp32: 2e-5 of each tensor's largest entry; bf16: 2e-3,
    the tolerance between two summation orders of the same bf16 gradients)."""
    from composer_amd import _lib
    V, E, H, L, W, T = geom
    params = {k: v.astype(np.float32) for k, v in O.init_params(V, E, W, L, seed=7).items()}
    x, y = O.synthetic_batch(np.random.default_rng(17), V, 2 * B, T)
    m = make_model((V, E, H, L, W, T, B), params, dtype, p_attn=0.1, p_resid=0.1, seed=5)
    want = {}
    for r in (0, 1):
        m.set_mask_rank(r)
        m.loss_and_grads(x[r * B:(r + 1) * B], y[r * B:(r + 1) * B])
        for n in m.parameter_names:
            want[n] = want.get(n, 0.0) + m.get_parameter(n, _lib.KIND_GRAD).astype(np.float64)
    m.set_mask_rank(0)
    m.set_train_options(accumulate_steps=2)
    m.train_step(x[:B], y[:B], 1e-3)
    m.train_step(x[B:], y[B:], 1e-3)
    assert m.iterations == 1
    worst = 0.0
    for n in m.parameter_names:
        G = m.get_parameter(n, _lib.KIND_GRAD).astype(np.float64)
        worst = max(worst, np.abs(G - want[n]).max() / (np.abs(want[n]).max() + 1e-30))
    print(dtype, "worst", worst)
    assert worst <= tol
    # ... and not the masks of rank 0 twice
    m.loss_and_grads(x[B:], y[B:])
    n = "decoder_blocks/0/mlp/c_fc/weight"
    g0 = m.get_parameter(n, _lib.KIND_GRAD).astype(np.float64)
    m.set_mask_rank(1)
    m.loss_and_grads(x[B:], y[B:])
    g1 = m.get_parameter(n, _lib.KIND_GRAD).astype(np.float64)
    assert np.abs(g0 - g1).max() > 100 * tol * np.abs(g1).max()
    m.close()


# ------------------------------------------------------------------------------------------------ 7. communicator
def test_one_rank_communicator_clipped_accumulated_steps():
    """With a communicator the buckets' sums of squares follow their all-reduces on the communication stream and ONE Adam launch
    updates the whole buffer behind the last: three steps of (clip 0.7, k = 2) match the run without a communicator (the norm
    differs by float64 summation order only)."""
    from composer_amd.transformer import Transformer
    g, cfg, params = load_golden("gA")
    L = cfg[3]
    runs = []
    for dp in (False, True):
        m = make_model(cfg, params, "fp32")
        if dp:
            m.init_data_parallel(0, 1, Transformer.new_unique_id())
        m.set_train_options(clip_norm=0.7, accumulate_steps=2)
        norms = []
        for s in range(6):
            m.train_step(g["x"][s], g["y"][s], float(g["lr"]))
            norm, scale = m.grad_stats()
            if s % 2 == 1:
                norms.append(norm)
                assert scale < 1.0
            else:
                assert norm is None
        assert m.iterations == 3
        if dp:
            st = m.dp_stats()
            assert st["steps"] == 3 and st["buckets"] == L + 3
        runs.append((norms, {n: m.get_parameter(n) for n in m.parameter_names}))
        m.close()
    print("norms", runs[0][0], runs[1][0])
    for a, b in zip(runs[0][0], runs[1][0]):
        assert abs(a - b) <= 1e-6 * a
    for n in runs[0][1]:
        assert np.abs(runs[0][1][n] - runs[1][1][n]).max() <= 2e-6, n
    # the defaults under the communicator: every bucket all-reduced and updated as before
    m = make_model(cfg, params, "fp32")
    m.init_data_parallel(0, 1, Transformer.new_unique_id())
    loss, _ = m.train_step(g["x"][0], g["y"][0], float(g["lr"]))
    assert abs(loss - g["losses"][0]) <= 1e-4 * abs(g["losses"][0])
    assert m.dp_stats()["buckets"] == L + 3 and m.grad_stats() == (None, 1.0)
    m.close()


# ------------------------------------------------------------------------------------------------ 8. launch counts
def test_launch_counts():
    from composer_amd import _lib
    g, cfg, params = load_golden("gA")
    V, E, H, L, W, T, B = cfg
    m = make_model(cfg, params, "fp32")
    x, y = np.ascontiguousarray(g["x"][0].astype(np.int32)), np.ascontiguousarray(g["y"][0].astype(np.int32))
    xd, yd = torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda()
    m.train_step(x, y, 1e-3)

    def count():
        nk, no = C.c_int(0), C.c_int(0)
        _lib.check(m._lib.cmp_train_step_launches(m._h, P(xd), P(yd), x.shape[0], x.shape[1], C.byref(nk), C.byref(no)))
        return nk.value, no.value
    base = count()
    m.set_train_options(0.0, 1)
    assert count() == base
    m.set_train_options(1.0, 1)
    clipped = count()
    print("launches", base, clipped)
    assert base[0] < clipped[0] <= base[0] + 2
    m.set_train_options(0.0, 2)                   # the FINAL micro-step: no memset of G, Adam as at k = 1
    assert count() == (base[0], base[1] - 1)
    assert m.train_options()["pending_micro_steps"] == 0 and m.iterations == 1
    m.close()
