"""-m gpu: the bias gradients of the decoder blocks taken from the blocks' grouped weight-gradient launches (model.hip: backward,
`carry`; gemm.hip: WgProb::bias; by default those of c_fc and c_attn, with COMPOSER_BIAS_WGRAD=15 all four) against the producers'
own column sums (COMPOSER_BIAS_WGRAD=0: the LayerNorm backward kernels, the GELU' dgrad epilogue, the attention backward kernels)
and against the float64 oracle.

The model is the smallest bf16 one whose step carries: the grouped launch needs a token count that is a multiple of 32 and four
problems whose plan (cmp_wgrad_group_plan) takes the launch -- E = 64, 2 x 48 = 96 tokens; 2 x 47 tokens do not fit and do not
carry.  Gradients are compared as tests/test_gpu_model.py compares them (its model builder; per parameter the largest difference
over the largest reference magnitude, bf16 bound 8e-2 as in test_dropout_training_step_matches_oracle)."""
import ctypes as C

import numpy as np
import pytest

from oracle import transformer_oracle as O
from test_gpu_model import make_model

pytestmark = pytest.mark.gpu

V, E, H, L, W, T, B = 390, 64, 4, 2, 48, 48, 2
CFG = (V, E, H, L, W, T, B)
BF16_GRAD_TOL = 8e-2           # tests/test_gpu_model.py: test_dropout_training_step_matches_oracle, bf16


def carried(m):
    from composer_amd import _lib
    c = C.c_int(-1)
    _lib.check(_lib.load().cmp_model_bias_path(m._h, C.byref(c)), "cmp_model_bias_path")
    return c.value


def plan_takes(E_, tokens):
    """The plan of a block's four problems (dWpr, dWfc, dWproj, dWattn) at this token count: (fits, taken)."""
    from composer_amd import _lib
    shapes = [(4 * E_, E_), (E_, 4 * E_), (E_, E_), (E_, 3 * E_)]
    ip = C.c_int * 4
    info = _lib.WgradPlanInfo()
    Ms, Ns = ip(*[s[0] for s in shapes]), ip(*[s[1] for s in shapes])
    _lib.check(_lib.load().cmp_wgrad_group_plan(4, None, Ms, None, Ns, Ms, Ns, tokens, 0, 0, C.byref(info), None, 0), "cmp_wgrad_group_plan")
    return bool(info.fits), bool(info.taken)


def worst(a, b, names):
    """Per parameter: largest |a - b| over largest |b| (the measure of tests/test_gpu_model.py); returns the worst and its name."""
    w = {n: np.abs(a[n] - b[n]).max() / (np.abs(b[n]).max() + 1e-12) for n in names}
    n = max(w, key=w.get)
    return w[n], n


def bias_names(m):
    names = [n for n in m.parameter_names if "decoder_blocks" in n and n.endswith("bias")]
    assert len(names) == 4 * L, names               # c_attn, c_proj, mlp c_fc, mlp c_proj of every block (block 0 and the last one included)
    return names


@pytest.fixture(scope="module")
def setup():
    params = {k: v.astype(np.float32) for k, v in O.init_params(V, E, W, L, seed=21).items()}
    rng = np.random.default_rng(8)
    for k in params:
        if k.endswith(("gamma", "beta", "bias")):
            params[k] = (params[k] + 0.05 * rng.standard_normal(params[k].shape)).astype(np.float32)
    x, y = O.synthetic_batch(rng, V, B, T)
    x2, y2 = O.synthetic_batch(rng, V, B, T)
    oracle = {}
    for p in (0.1, 0.0):
        orc = O.OracleTransformer(O.Config(V, E, W, L, H, attention_dropout_rate=p, residual_dropout_rate=p), params, seed=99)
        oracle[p] = orc.loss_and_grads(x, y, training=True, step=0)
    return params, (x, y), (x2, y2), oracle


def grads_of(m):
    from composer_amd import _lib
    return {n: m.get_parameter(n, _lib.KIND_GRAD).astype(np.float64) for n in m.parameter_names}


def run_once(monkeypatch, params, batch, p, switch, dp=False, env=None):
    """loss, gradients and the reported path of one loss_and_grads call; switch: COMPOSER_BIAS_WGRAD (None: unset)."""
    monkeypatch.delenv("COMPOSER_BIAS_WGRAD", raising=False)
    if switch is not None:
        monkeypatch.setenv("COMPOSER_BIAS_WGRAD", switch)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    m = make_model(CFG, params, "bf16", p_attn=p, p_resid=p, seed=99)
    try:
        if dp:
            from composer_amd.transformer import Transformer
            m.init_data_parallel(0, 1, Transformer.new_unique_id())
        assert carried(m) == 0                      # no backward pass yet
        loss, _ = m.loss_and_grads(*batch)
        return loss, grads_of(m), carried(m), bias_names(m), list(m.parameter_names)
    finally:
        m.close()
        for k in (env or {}):
            monkeypatch.delenv(k, raising=False)


def test_the_smallest_carrying_shape_is_what_the_plan_says():
    assert plan_takes(E, B * T) == (True, True)
    assert plan_takes(E, B * 47) == (False, False)          # 94 tokens: no multiple of 32
    assert plan_takes(E, 32) == (True, True)                # one k-step still carries; 96 tokens give every tile three k-steps


@pytest.mark.parametrize("switch", [None, "15"])
@pytest.mark.parametrize("p", [0.1, 0.0])
def test_carried_bias_gradients_match_the_producers_and_the_oracle(monkeypatch, setup, p, switch):
    """The default (c_fc and c_attn biases carried) and COMPOSER_BIAS_WGRAD=15 (all four: also the two whose B operand is dmo / dao).
    Dropout 0.1: dmo / dao are the masked copies the LayerNorm backward kernels write; dropout 0: they are dx / dr themselves."""
    params, batch, _, oracle = setup
    l0, g0, c0, bn, names = run_once(monkeypatch, params, batch, p, "0")
    l1, g1, c1, _, _ = run_once(monkeypatch, params, batch, p, switch)
    assert (c0, c1) == (0, 1)
    wb, nb = worst(g1, g0, bn)
    wa, na = worst(g1, g0, names)
    print("p=%.1f carried vs producers: worst bias gradient %.3g (%s), worst of all %.3g (%s)" % (p, wb, nb, wa, na))
    assert wb <= BF16_GRAD_TOL and wa <= BF16_GRAD_TOL
    assert abs(l1 - l0) <= 1e-6 * abs(l0)                   # the forward pass is the same code
    loss, _, G, _ = oracle[p]
    for tag, l, g in (("producers", l0, g0), ("carried", l1, g1)):
        assert abs(l - loss) <= 3e-2 * abs(loss), tag
        w, n = worst(g, G, names)
        print("p=%.1f %s vs oracle: worst %.3g (%s)" % (p, tag, w, n))
        assert w <= BF16_GRAD_TOL, (tag, n, w)


def test_unaligned_token_count_does_not_carry(monkeypatch, setup):
    params, (x, y), _, _ = setup
    monkeypatch.delenv("COMPOSER_BIAS_WGRAD", raising=False)
    m = make_model(CFG, params, "bf16", seed=99)
    m.loss_and_grads(x[:, :47], y[:, :47])
    assert carried(m) == 0
    m.loss_and_grads(x, y)
    assert carried(m) == 1
    m.close()


def test_accumulation_and_clipping_see_complete_bias_gradients(monkeypatch, setup):
    """accumulate_steps = 2 with clipping on: the second micro-step ADDS to what G holds; the accumulated bias gradients and the
    reported global norm of both paths agree."""
    params, b1, b2, _ = setup
    out = {}
    for switch in ("0", "15"):
        monkeypatch.delenv("COMPOSER_BIAS_WGRAD", raising=False)
        if switch is not None:
            monkeypatch.setenv("COMPOSER_BIAS_WGRAD", switch)
        m = make_model(CFG, params, "bf16", p_attn=0.1, p_resid=0.1, seed=99)
        m.set_train_options(clip_norm=0.05, accumulate_steps=2)
        m.train_step(*b1, 1e-3)
        assert m.train_options()["pending_micro_steps"] == 1
        m.train_step(*b2, 1e-3)
        norm, scale = m.grad_stats()
        out[switch] = (grads_of(m), norm, scale, carried(m), bias_names(m), list(m.parameter_names))
        m.close()
    (g0, n0, s0, c0, bn, names), (g1, n1, s1, c1, _, _) = out["0"], out["15"]
    assert (c0, c1) == (0, 1)
    assert n0 is not None and n1 is not None and s0 < 1.0 and s1 < 1.0          # clipping was on and bit
    wb, nb = worst(g1, g0, bn)
    wa, na = worst(g1, g0, names)
    print("accumulated: worst bias gradient %.3g (%s), worst of all %.3g (%s); norms %.6g / %.6g" % (wb, nb, wa, na, n1, n0))
    assert wb <= BF16_GRAD_TOL and wa <= BF16_GRAD_TOL
    assert abs(n1 - n0) <= BF16_GRAD_TOL * n0 and abs(s1 - s0) <= BF16_GRAD_TOL * s0
    # the accumulated sum is not one micro-step's: the second one added
    single = run_once(monkeypatch, params, b2, 0.1, "15")[1]
    assert worst(g1, single, bn)[0] > 1e-3


def test_deterministic_mode_does_not_carry_and_still_matches(monkeypatch, setup):
    params, batch, _, oracle = setup
    l, g, c, bn, names = run_once(monkeypatch, params, batch, 0.1, None, env={"COMPOSER_DETERMINISTIC": "1"})
    assert c == 0
    loss, _, G, _ = oracle[0.1]
    assert abs(l - loss) <= 3e-2 * abs(loss)
    assert worst(g, G, names)[0] <= BF16_GRAD_TOL


def test_one_rank_communicator_carries_too(monkeypatch, setup):
    """With a communicator the persistent GEMM kernels claim their items dynamically (and the gradient buckets are handed to the
    all-reduce behind each block): the carried sums must not depend on which workgroup runs which item."""
    params, batch, _, oracle = setup
    l0, g0, c0, bn, names = run_once(monkeypatch, params, batch, 0.1, "0", dp=True)
    l1, g1, c1, _, _ = run_once(monkeypatch, params, batch, 0.1, "15", dp=True)
    assert (c0, c1) == (0, 1)
    assert worst(g1, g0, names)[0] <= BF16_GRAD_TOL
    assert worst(g1, oracle[0.1][2], names)[0] <= BF16_GRAD_TOL


def test_fused_block_training_path_does_not_carry(monkeypatch):
    """COMPOSER_LN_FUSED=3 at the smallest shape whose training pass takes the fused block path (tests/test_gpu_ln_fused.py): the
    raw-row order stores rstd-scaled operands, so it keeps the producers' sums (carried == 0).  The default order of the same
    shape carries -- 2048-row problems: eight tile rows -- and the bias gradients of both agree as that file's fused / unfused
    comparison asks (3e-2)."""
    from composer_amd import _lib
    from composer_amd.transformer import Transformer
    E_, H_, L_, T_, B_ = 512, 8, 2, 256, 96
    assert plan_takes(E_, B_ * T_) == (True, True)
    params = {k: v.astype(np.float32) for k, v in O.init_params(V, E_, T_, L_, seed=E_, stddev=0.05).items()}
    rng = np.random.default_rng(E_ + L_)
    x, y = O.synthetic_batch(rng, V, B_, T_)
    res = {}
    for mode in ("3", None, "all", "off"):
        monkeypatch.delenv("COMPOSER_LN_FUSED", raising=False)
        monkeypatch.delenv("COMPOSER_BIAS_WGRAD", raising=False)
        if mode == "3":
            monkeypatch.setenv("COMPOSER_LN_FUSED", "3")
        if mode in ("off", "all"):
            monkeypatch.setenv("COMPOSER_BIAS_WGRAD", "0" if mode == "off" else "15")
        m = Transformer(V, E_, T_, L_, H_, attention_dropout_rate=0.1, residual_dropout_rate=0.1, dtype="bf16", seed=3, max_batch=B_, max_seq=T_)
        m.set_weights(params)
        m.loss_and_grads(x, y)
        f = C.c_int(-1)
        _lib.check(_lib.load().cmp_model_path_info(m._h, C.byref(f), None))
        names = [n for n in m.parameter_names if "decoder_blocks" in n and n.endswith("bias")]
        res[mode] = (f.value, carried(m), {n: m.get_parameter(n, _lib.KIND_GRAD).astype(np.float64) for n in names}, names)
        m.close()
    monkeypatch.delenv("COMPOSER_LN_FUSED", raising=False)
    monkeypatch.delenv("COMPOSER_BIAS_WGRAD", raising=False)
    assert res["3"][:2] == (1, 0) and res[None][:2] == (0, 1) and res["all"][:2] == (0, 1) and res["off"][:2] == (0, 0)
    names = res[None][3]
    for mode in (None, "all"):
        w, n = worst(res[mode][2], res["off"][2], names)
        print("E=512, 24576 tokens: carried (%s) vs producers, worst bias gradient %.3g (%s)" % (mode or "default", w, n))
        assert w <= 3e-2
    assert worst(res["3"][2], res["off"][2], names)[0] <= 3e-2
