"""-m gpu: the optimiser, bounded per element from the kernel to the model, and every derived weight copy behind it.

A. cmp_k_adam / cmp_k_adam_dev against `kernel_arena.adam_reference` (float64) inside `kernel_arena.adam_bounds` (one-ulp fp32
   primitives, margin 2) on `kernel_arena.adam_inputs`: segments that put the placement of eps, the first step, pure decay, an
   untouched element and large gradients in view, at steps from 1 to 2^31 + 5, three factors, lr = 0, and once at a size where
   the grid-stride loop takes a second trip.  tests/test_kernel_checks_host.py proves on the CPU that the same check rejects
   ten wrong kernels and writes down what the older assertions let through.
B. One optimiser step of a small model is Adam of the stored moments: (p1, m1, v1) of EVERY element of EVERY parameter against the
   same reference and bound, fed with the gradient the device itself consumed (kind 3), so no gradient tolerance enters -- fp32 and
   bf16, clipped, accumulated, under a 1-rank communicator (one launch per bucket), and with lr = 0.
C. Every derived copy follows the weights: a model that lives through a history of train steps, parameter writes, checkpoint
   loads and passes on other batch sizes gives bitwise the logits of a fresh model that only ever received its current weights.

Measured on an MI355X (each test prints its figures; worst error / limit):
   A  all steps, factors and both kernels: p 0.50, m 0.31, v 0.38 (factor 1/3; v 0.24 at factor 0.5); the grid-stride case p 0.50, m 0.32, v 0.24
   B  see `test_train_step_is_adam_of_the_stored_moments`
   C  every path repeats bitwise: the spread between two passes of the fresh model is 0 in all four histories
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import kernel_arena as KA
from kernel_arena import Arena
from oracle import transformer_oracle as O

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-7
STEPS = [1, 2, 7, 1000, 10 ** 6, 2 ** 31 + 5]          # the last two: beta^t underflows (alpha = lr), the int64 step survives the ABI
FACTORS = [1.0, 0.5, 1.0 / 3.0]
GRID_STRIDE_N = 8192 * 1024 + 1028                      # grid = min(cdiv(n / 4, 256), 8192): from here a thread takes a second f32x4


@pytest.fixture(scope="module")
def lib():
    from composer_amd import _lib
    l = _lib.load()
    _lib.require_gpu()
    return l


def ck(lib, rc):
    assert rc == 0, lib.cmp_last_error().decode()


def P(slot):
    return C.c_void_p(slot.ptr()) if slot is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------ A. the kernel pair
def launch_adam(lib, inp, step, factor, dev, lr=LR, arena_bytes=1 << 20):
    """One launch with all five arrays (and the device factor) flush against guards -> (p, m, v, shadow) read back."""
    n = inp["p0"].numel()
    ar = Arena("cuda", arena_bytes, big=arena_bytes > 64 << 20)
    p, m, v = (ar.vector(inp[k], F32, name=k[0], kind="acc") for k in ("p0", "m0", "v0"))
    g = ar.vector(inp["g"], F32, name="g")
    sh = ar.output(BF, 1, n, n, name="shadow")
    fac = ar.vector(torch.tensor([factor], dtype=F32), F32, name="factor")
    ar.arm()
    if dev:
        ck(lib, lib.cmp_k_adam_dev(stream(), P(p), P(g), P(m), P(v), P(sh), n, lr, B1, B2, EPS, step, P(fac)))
    else:
        ck(lib, lib.cmp_k_adam(stream(), P(p), P(g), P(m), P(v), P(sh), n, lr, B1, B2, EPS, step, float(np.float32(factor))))
    ar.check()
    return p.host()[0], m.host()[0], v.host()[0], sh.host()[0]


@pytest.mark.parametrize("step", STEPS)
def test_adam_kernels_within_the_bound(lib, step):
    """Both kernels, three factors, one step count per case: every element of p, m and v inside the bound, segment f untouched, the
    shadow the RNE image of p, guards intact -- and the two kernels bitwise equal on these inputs.
    Measured, worst error / limit over all cases: p 0.496 (t = 1000, factor 0.5), m 0.302 and v 0.372 (factor 1/3, every t)."""
    for factor in FACTORS:
        inp, seg = KA.adam_inputs(factor)
        assert inp["p0"].numel() % 1024 != 0
        res = []
        for dev in (False, True):
            p, m, v, sh = launch_adam(lib, inp, step, factor, dev)
            worst = KA.adam_check(inp, seg, p, m, v, sh, LR, B1, B2, EPS, step, factor, "adam_dev" if dev else "adam")
            print("step", step, "factor %.4g" % factor, "dev" if dev else "arg", "worst error/limit", {k: round(x, 3) for k, x in worst.items()})
            res.append((p, m, v, sh))
        for a, b, name in zip(res[0], res[1], "pmvs"):
            assert np.array_equal(a.view(torch.int16).numpy(), b.view(torch.int16).numpy()), "the two kernels differ in %s" % name


@pytest.mark.parametrize("dev", [False, True])
def test_adam_with_lr_zero_moves_the_moments_only(lib, dev):
    inp, seg = KA.adam_inputs(0.5)
    p, m, v, sh = launch_adam(lib, inp, 7, 0.5, dev, lr=0.0)
    KA.adam_check(inp, seg, p, m, v, sh, 0.0, B1, B2, EPS, 7, 0.5, "adam lr = 0")      # (asserts p bitwise unchanged, m and v moved)


_GRID_STRIDE = {}


def grid_stride_case():
    """inputs, reference and limits of the large case: computed once, shared by both kernels, never modified"""
    if not _GRID_STRIDE:
        inp, seg = KA.adam_inputs(0.5, seed=11, n_generic=GRID_STRIDE_N - sum(k for _, k in KA.ADAM_EDGE_SEGMENTS))
        args = (inp["p0"], inp["g"], inp["m0"], inp["v0"], LR, B1, B2, EPS, 7, 0.5)
        _GRID_STRIDE["case"] = (inp, seg, KA.adam_reference(*args), KA.adam_bounds(*args))
    return _GRID_STRIDE["case"]


@pytest.mark.parametrize("dev", [False, True])
def test_adam_grid_stride_loop(lib, dev):
    """n = 8192 * 1024 + 1028: the launch is capped at 8192 blocks, so 257 threads take a second trip through the loop (both full-size
    configurations are that large).  The edge segments sit at the end, across the trip boundary.  Same per-element bound over the
    whole arrays, shadow, guards.  Measured worst error / limit, both kernels: p 0.499, m 0.312, v 0.231."""
    inp, seg, ref, lim = grid_stride_case()
    n = inp["p0"].numel()
    assert n == GRID_STRIDE_N and n // 4 > 8192 * 256 and n % 1024 != 0
    p, m, v, sh = launch_adam(lib, inp, 7, 0.5, dev, arena_bytes=18 * n + (1 << 20))
    worst = KA.adam_check(inp, seg, p, m, v, sh, LR, B1, B2, EPS, 7, 0.5, "adam grid-stride", ref_lim=(ref, lim))
    print("grid-stride", "dev" if dev else "arg", "worst error/limit", {k: round(x, 3) for k, x in worst.items()})


# ------------------------------------------------------------------------------------------ B. a train step is Adam of the stored moments
V, E, H, L, W, T, B = 390, 64, 2, 2, 32, 32, 2


def small_model(dtype, p_drop=0.1, seed=3):
    from composer_amd.transformer import Transformer
    m = Transformer(V, E, W, L, H, attention_dropout_rate=p_drop, residual_dropout_rate=p_drop, dtype=dtype, seed=seed, max_batch=B, max_seq=W)
    rng = np.random.default_rng(seed + 100)
    for n in m.parameter_names:                                      # LayerNorm parameters and biases away from (1, 0, 0)
        if n.endswith(("gamma", "beta", "bias")):
            m.set_parameter(n, m.get_parameter(n) + 0.05 * rng.standard_normal(m.parameter_shape(n)).astype(np.float32))
    return m


def batches(count, seed=5):
    rng = np.random.default_rng(seed)
    return [O.synthetic_batch(rng, V, B, T) for _ in range(count)]


def read_state(m):
    from composer_amd import _lib
    return {k: {n: m.get_parameter(n, k) for n in m.parameter_names} for k in (_lib.KIND_VALUE, _lib.KIND_ADAM_M, _lib.KIND_ADAM_V)}


def state_bytes(st):
    return {(k, n): a.tobytes() for k, d in st.items() for n, a in d.items()}


def hold_step(m, before, lr, k, nranks, label):
    """After ONE optimiser step: every element of every parameter against Adam of the snapshot `before` and the device's own G."""
    from composer_amd import _lib
    after = read_state(m)
    t = m.iterations
    norm, scale = m.grad_stats()
    gscale = np.float32(1.0) / np.float32(k * nranks)                # 1.0f / (float)(nranks * accum_steps)
    factor = gscale * np.float32(scale)                              # fp32 product, as grad_clip_finish_kernel forms it
    assert factor.dtype == np.float32
    worst, G = {"p": 0.0, "m": 0.0, "v": 0.0}, {}
    for n in m.parameter_names:
        G[n] = m.get_parameter(n, _lib.KIND_GRAD)
        args = (before[_lib.KIND_VALUE][n].ravel(), G[n].ravel(), before[_lib.KIND_ADAM_M][n].ravel(), before[_lib.KIND_ADAM_V][n].ravel(),
                lr, B1, B2, EPS, t, factor)
        ref, lim = KA.adam_reference(*args), KA.adam_bounds(*args)
        for name, kind, r, l in (("m", _lib.KIND_ADAM_M, ref[1], lim[1]), ("v", _lib.KIND_ADAM_V, ref[2], lim[2]), ("p", _lib.KIND_VALUE, ref[0], lim[0])):
            w = KA.assert_within(torch.from_numpy(after[kind][n].ravel()), torch.from_numpy(r), torch.from_numpy(l), False,
                                 "%s: %s of %s (flat index within the parameter) at t = %d" % (label, name, n, t))
            worst[name] = max(worst[name], w)
    print(label, "t", t, "factor", float(factor), "norm", norm, "scale", scale, "worst error/limit", {k_: round(x, 3) for k_, x in worst.items()})
    return after, G, norm, scale, gscale


STEP_CASES = ["fp32", "bf16", "bf16-clip", "fp32-accum3", "fp32-comm", "fp32-comm-clip", "fp32-lr0"]


@pytest.mark.parametrize("case", STEP_CASES)
def test_train_step_is_adam_of_the_stored_moments(case):
    """Two warm-up steps (non-zero moments), a snapshot of every value, m and v, ONE optimiser step, then (p1, m1, v1) of every element
    of every parameter inside adam_bounds of adam_reference(p0, G, m0, v0, t = iterations after the step, factor), G the SUM the
    device's Adam consumed, factor = float32(gscale) * float32(scale).  Nothing is left out: the reference is fed the device's own
    gradient, so neither the gradient's tolerance nor the sign of a noisy element enters, in bf16 mode either.
    Clipped cases: the clip is half the norm a measure-only step reported on the same batch, and the reported norm is
    gscale * sqrt(sum G^2) (float64 over the read-back G, the tied wte once) to 2^-23 relative: the cast to float in cmp_train_grad_stats.
    Measured worst error / limit (p, m, v): fp32 0.488 0.302 0.295; bf16 0.484 0.311 0.289; bf16-clip 0.495 0.370 0.441 (norm 1.4019383 against
    1.40193837 in float64, scale 0.4958); fp32-accum3 0.490 0.359 0.457; fp32-comm 0.488 0.293 0.292; fp32-comm-clip 0.485 0.362 0.472 (norm
    1.4038473 against 1.40384737); fp32-lr0 0 0.284 0.288."""
    from composer_amd.transformer import Transformer
    dtype = case.split("-")[0]
    clip, comm = "clip" in case, "comm" in case
    k = 3 if "accum3" in case else 1
    lr = 0.0 if "lr0" in case else LR
    data = batches(2 + k)
    m = small_model(dtype)
    try:
        if comm:
            m.init_data_parallel(0, 1, Transformer.new_unique_id())
        if clip:
            m.set_train_options(clip_norm=math.inf)                   # measure only
        m.train_step(*data[0], LR)
        m.train_step(*data[2], LR)                                    # the batch of the step under test
        if clip:
            measured, s = m.grad_stats()
            assert measured is not None and math.isfinite(measured) and measured > 0 and s == 1.0
            m.set_train_options(clip_norm=0.5 * measured)
        if k > 1:
            m.set_train_options(accumulate_steps=k)
        assert m.iterations == 2
        before = read_state(m)
        for j in range(k - 1):                                        # micro-steps 1 .. k - 1 move nothing
            m.train_step(*data[2 + j], lr)
            assert m.iterations == 2 and state_bytes(read_state(m)) == state_bytes(before), "micro-step %d changed the optimiser's state" % (j + 1)
        m.train_step(*data[2 + k - 1], lr)
        assert m.iterations == 3
        after, G, norm, scale, gscale = hold_step(m, before, lr, k, 1, case)
        if comm:
            assert m.dp_stats()["buckets"] == L + 3                   # one all-reduce (and, unclipped, one Adam launch) per bucket
        if clip:
            assert scale < 1.0 and norm is not None
            want = float(gscale) * math.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in G.values()))
            print(case, "norm", norm, "float64 of the read-back G", want, "measure-only step", measured)
            assert abs(norm - want) <= 2.0 ** -23 * want
            assert 0.4 < scale < 0.6                                  # half the measured norm, one update later
        else:
            assert norm is None and scale == 1.0
        sb, sa = state_bytes(before), state_bytes(after)
        moved = {kind: sum(sb[(kind, n)] != sa[(kind, n)] for n in m.parameter_names) for kind in before}
        if lr == 0.0:
            assert moved[0] == 0, "lr = 0 changed a parameter value"
        else:
            assert moved[0] == len(m.parameter_names)
        assert moved[1] == moved[2] == len(m.parameter_names)
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ C. every derived copy follows the weights
def _fused(m):
    from composer_amd import _lib
    f, n = C.c_int(-1), C.c_int64(-1)
    _lib.check(_lib.load().cmp_model_path_info(m._h, C.byref(f), C.byref(n)))
    return f.value


def logits_of(m, x):
    return np.asarray(m(x, training=False)[0]).copy()


HISTORIES = {   # name: (dtype, E, H, L, T, B of the fixed batch, COMPOSER_LN_FUSED, fused on the fixed batch)
    "fp32-small": ("fp32", 64, 2, 2, 32, 4, None, 0),               # no shadow, no ST: the control
    "bf16-small": ("bf16", 64, 2, 2, 32, 4, None, 0),               # the plain path: S and the plain ST
    # ln_fused_ok (model.hip): bf16, E a multiple of 256 in [512, 768], tokens a multiple of 256 with (tokens / 256) * (E / 256) >= 192
    # -- at E = 512, T = 256 the smallest batch is B = 96.  The train step takes the plain ST, the inference pass the folded set.
    "bf16-fused": ("bf16", 512, 8, 2, 256, 96, None, 1),
    "bf16-fused-train": ("bf16", 512, 8, 2, 256, 96, "3", 1),       # the train step itself takes the folded set
}


@pytest.mark.parametrize("name", list(HISTORIES))
def test_derived_copies_follow_the_weights(name, monkeypatch):
    """Model A lives through: forward; train step; two forwards; set_parameter of one ln_1/gamma and of ln_f/beta; loss_and_grads;
    an evaluate on a small batch; load_state_dict of a perturbed state; an accumulated step of two micro-steps (COMPOSER_LN_FUSED=3
    refuses accumulation, by name: there the refusal is asserted and one plain step follows).  Wherever the weights
    changed, A's inference logits on a fixed batch are BITWISE those of a fresh model F, created for that comparison, that received
    A.get_weights() and nothing else; wherever they did not, A's logits are bitwise the previous pass's.  Covers the bf16 shadow S,
    the transposed shadow ST in both of its states (plain / folded: asserted through cmp_model_path_info, fused on the fixed batch and
    not on the small one), the fold vectors and wte_lnf.  A stale copy moves logits by the relative size of an update (1e-3), a stale
    gamma by far more.
    Measured: all four histories repeat bitwise (two passes of F differ by 0); no tolerance is used."""
    from composer_amd import _lib
    from composer_amd.transformer import Transformer
    dtype, E_, H_, L_, T_, B_, mode, fused = HISTORIES[name]
    if mode is None:
        monkeypatch.delenv("COMPOSER_LN_FUSED", raising=False)
    else:
        monkeypatch.setenv("COMPOSER_LN_FUSED", mode)                 # read once per model, at creation

    def make():
        return Transformer(V, E_, T_, L_, H_, attention_dropout_rate=0.1, residual_dropout_rate=0.1, dtype=dtype, seed=3, max_batch=B_, max_seq=T_)
    rng = np.random.default_rng(E_ + B_)
    x, y = O.synthetic_batch(rng, V, B_, T_)
    xs, ys = O.synthetic_batch(rng, V, 2, T_)
    A = make()
    state = {"last": None, "compares": 0}

    def forward_A(expect=None):
        z = logits_of(A, x)
        assert _fused(A) == fused
        if expect is not None:
            assert np.array_equal(z, expect), "%s: a pass without a parameter change differs from the previous pass (max |d| %g)" % (name, np.abs(z - expect).max())
        state["last"] = z
        return z

    def compare(what):
        Fm = make()
        try:
            Fm.set_weights(A.get_weights())
            f1, f2 = logits_of(Fm, x), logits_of(Fm, x)
            assert _fused(Fm) == fused
        finally:
            Fm.close()
        assert np.isfinite(f1).all()
        assert np.array_equal(f1, f2), "%s: two passes of the fresh model differ by %g" % (name, np.abs(f1 - f2).max())
        z = forward_A()
        if "prev_fresh" in state:
            assert not np.array_equal(f1, state["prev_fresh"]), "%s: %s did not change the logits at all" % (name, what)
        d = np.abs(z - f1)
        assert np.array_equal(z, f1), ("%s after %s: the model's logits differ from a fresh model's with the same weights: max |d| %g (%g of max |z|), "
                                       "%d of %d elements, first at %s" % (name, what, d.max(), d.max() / np.abs(f1).max(), int((d > 0).sum()), d.size,
                                                                           tuple(int(i) for i in np.argwhere(d > 0)[0])))
        state["prev_fresh"] = f1
        state["compares"] += 1
        return z

    try:
        forward_A()                                                   # 1. derived copies of the initial weights exist
        compare("creation")
        A.train_step(x, y, LR)                                        # 2.
        z = compare("a train step")
        forward_A(z); forward_A(z)                                    # 3.
        g1 = "decoder_blocks/1/ln_1/gamma"                            # 4. the fold vectors depend on gamma / beta, not only on matrices
        A.set_parameter(g1, A.get_parameter(g1) * 1.25 + 0.1 * rng.standard_normal(E_).astype(np.float32))
        A.set_parameter("ln_f/beta", A.get_parameter("ln_f/beta") + 0.2 * rng.standard_normal(E_).astype(np.float32))
        z = compare("set_parameter of ln_1/gamma and ln_f/beta")
        A.loss_and_grads(x, y)                                        # 5. a training pass that moves no parameter
        forward_A(z)
        A.evaluate([(xs, ys)])                                        # 6. a small batch: the unfused path, the plain ST
        assert _fused(A) == 0
        forward_A(z)
        sd = A.state_dict()                                           # 7.
        for key in sd:
            if key.startswith("model/"):
                sd[key] = (sd[key] * (1 + 0.02 * rng.standard_normal(sd[key].shape))).astype(np.float32)
        A.load_state_dict(sd)
        z = compare("load_state_dict of a perturbed state")
        it = A.iterations                                             # 8.
        if mode == "3":
            with pytest.raises(_lib.HipLibraryError, match="COMPOSER_LN_FUSED=3"):
                A.set_train_options(accumulate_steps=2)
            assert A.train_options()["accumulate_steps"] == 1
        else:
            A.set_train_options(accumulate_steps=2)
            A.train_step(x, y, LR)
            assert A.iterations == it
            forward_A(z)
        A.train_step(x, y, LR)
        assert A.iterations == it + 1
        compare("an accumulated train step" if mode != "3" else "a plain train step after the refused accumulation")
        assert state["compares"] == 5
    finally:
        A.close()
