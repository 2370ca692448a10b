"""-m gpu: the grouped weight-gradient launch (cmp_k_wgrad_group_bias -> gemm_wgrad_group_kernel, and gemm_wgrad_group_la_kernel under
COMPOSER_WGRAD_TAIL=la -- the form COMPOSER_DETERMINISTIC=1 trains with) with SEVERAL items per workgroup, and the last-arriver fold
held to its stated order bit for bit.  Tables, operands, references, emulations: tests/wgrad_items_cases.py; that every row reaches
what it names and that every check here can fail: tests/test_wgrad_items_host.py.

All of it in the pattern of test_gpu_wgrad_group_bias.test_wgrad_group_bias_guarded: guard-banded arena, every leading dimension
8 / 16 / 8 elements wider than the row and as narrow as the launch allows, NaN padding columns in A and B, non-zero start values in
C and in the bias vectors, ar.check() after every launch, kernel_arena's gemm_bound / colsum_bound per element.  The one-shot
cmp_gemm_grid_next(cap, 0) in front of the launch makes the plan's workgroup count the cap.

A  P8 (34 tiles) at 1 .. 5 k-steps on 8, 16 and 24 workgroups, static and dynamic items: one K range per tile, so every element of C
   receives one addition -- C is BITWISE the same across the caps, the item modes, the stride regimes, the float-atomic and the
   last-arriver form (and the uncapped launch where that has one range per tile: K = 32); a bias vector receives one atomic per
   column: bitwise too; vectors of problems without a bias untouched; the last-arriver form refuses a bias and writes nothing.
B  S3 cut into several K ranges (5 each; 2 and 3; tiles with and without slots in one launch; none): the last-arriver result equals
   fl(C0 + fl(.. fl(p_0 + p_1) .. + p_last)) with every p_q taken from a single-range launch of that range's rows alone; two operand
   sets of the same shapes launched X, Y, X on one thread through the same table, slots and ticket counters (a slot read stale
   shows); table and workspace rebuilt 10 -> 55 -> 10 slots; the float-atomic form with bias on the same rows by bound.
C  the hook: armed once it caps one grouped launch, reaches no later cmp_k_gemm, and caps 1 .. 7 are refused by name.
D  one model: bf16, E = 320, one block, 96 tokens, a one-rank communicator with 8 CUs for the GEMMs -- 32 tiles on 8 workgroups.

Measured on an MI355X (2026-10-21), worst error / limit (-s prints them per test; reported, not asserted -- the limits are
kernel_arena's):
    A  K = 32 / 64 / 96 / 128 / 160, one range per tile:  C 0.124 / 0.180 / 0.154 / 0.134 / 0.151   bias 0.125 / 0.125 / 0.156 / 0.149 / 0.092
       uncapped with two ranges per tile (K >= 64):       C 0.188 / 0.200 / 0.110 / 0.103           bias 0.125 / 0.125 / 0.125 / 0.131
    B  K1024-nocap  la C 0.038 (its fold emulation 0.038)   float-atomic C 0.061, bias 0.125   X Y X: C 0.086
       K256-cap24   la C 0.065 (0.065)                      float-atomic C 0.069, bias 0.129   X Y X: C 0.096
       K96-cap16    la C 0.157 (0.157)                      float-atomic C 0.200, bias 0.156   X Y X: C 0.194   rebuild 10 / 55 / 10 slots: C 0.157
       K96-cap8     la C 0.154 (0.154)                      float-atomic C 0.154, bias 0.156
    D  worst gradient 8.0e-3 of the largest against the oracle (wpe), 2.0e-7 against the uncapped model (limit 8e-2)
Every bitwise comparison held, the fold emulation exactly (no element, no range differs).  A test function takes 0.03 to 0.5 s, the
model case 4.7 s (two models of E = 320 and the float64 oracle).
"""
import ctypes as C
import threading

import numpy as np
import pytest

import gemm_items_bounds as IB
import wgrad_items_cases as W
from test_gpu_kernel_guards import ck, lib, stream  # noqa: F401  (lib: the module's fixture)

pytestmark = pytest.mark.gpu

_PART = {}          # (K, seed, scale, kt0, kt1) -> the partial of that K range of every problem of S3, from a single-range launch
X_SET, Y_SET = (0, 1.0), (1, 4.0)            # (seed, scale): independent draws, Y at four times X's scale


def on_fresh_thread(fn):
    """Run fn on a thread of its own: the entry point's item table, slot workspace and armed state are per thread, so the thread
    starts without any of them (they are small and stay allocated when it ends)."""
    box = []

    def run():
        try:
            fn()
        except BaseException as e:          # noqa: B902  (handed to the test's thread)
            box.append(e)
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if box:
        raise box[0]


def set_form(monkeypatch, form, mode):
    monkeypatch.setenv("COMPOSER_GEMM_ITEMS", mode)
    if form == "la":
        monkeypatch.setenv("COMPOSER_WGRAD_TAIL", "la")
    else:
        monkeypatch.delenv("COMPOSER_WGRAD_TAIL", raising=False)


def go(lib, st, cap=0, bias=True):
    st.ar.arm()
    ck(lib, W.launch(lib, st, stream(), cap, bias))
    st.ar.check()
    return W.c_of(st)


def same_bits(got, base, what):
    for i, (a, b) in enumerate(zip(got, base)):
        diff = W.first_difference(a, b)
        assert diff is None, "%s: problem %d differs from the first launch of this case: %s" % (what, i, diff)


def gpu_partials(lib, monkeypatch, K, opset, pr):
    """Per problem of S3 the partial of each of its K ranges: rows 32 kt0 .. 32 kt1 of A and B staged as operands of their own, C
    zero, the float-atomic form on SUB_CAP workgroups -- one K range per tile (asserted), so C receives fl(0 + acc) = acc."""
    ops = W.operands("S3", K, *opset)
    out = [[None] * len(p) for p in pr]
    for k0, k1 in sorted({rng for p in pr for rng in p}):
        key = (K, opset, k0, k1)
        if key not in _PART:
            depth = 32 * (k1 - k0)
            ds, rs = W.plan(lib, W.S3, depth, W.SUB_CAP)
            assert W.ranges_histogram(rs) == {1: 11} and ds["nslots"] == 0
            set_form(monkeypatch, "atomic", "static")
            st = W.stage(W.sub_operands(ops, k0, k1), depth, False)
            _PART[key] = go(lib, st, W.SUB_CAP, bias=False)
        for i, p in enumerate(pr):
            if (k0, k1) in p:
                out[i][p.index((k0, k1))] = _PART[key][i]
    return out


def fold_of(lib, monkeypatch, K, cap, opset):
    """The last-arriver result the plan of (S3, K, cap) must give for this operand set, with the partials it was folded from."""
    _, rows = W.plan(lib, W.S3, K, cap)
    pr = W.problem_ranges(rows, len(W.S3))
    parts = gpu_partials(lib, monkeypatch, K, opset, pr)
    return [W.fold(o[2], p) for o, p in zip(W.operands("S3", K, *opset), parts)], parts, pr


def assert_fold(got, emu, parts, pr, what):
    for i, (c, e) in enumerate(zip(got, emu)):
        diff = np.argwhere(np.asarray(c, np.float32) != e)
        if diff.size:
            at = tuple(int(x) for x in diff[0])
            raise AssertionError("%s: C of problem %d at %s is %r, the fold in the kernel's order gives %r (%d of %d elements differ); partials of "
                                 "the K ranges %s there: %s" % (what, i, at, float(c[at]), float(e[at]), len(diff), e.size, pr[i],
                                                                [float(p[at]) for p in parts[i]]))


# ------------------------------------------------------------------------------------------ A: several items per workgroup
@pytest.mark.parametrize("K", W.DEPTHS)
def test_several_items_of_different_problems_per_workgroup(lib, monkeypatch, K):
    ops, refs = W.operands("P8", K), W.references("P8", K)
    worst = {"C": 0.0, "bias": 0.0, "C several ranges": 0.0, "bias several ranges": 0.0}
    base_c = base_b = None
    for padded in (True, False):
        st = W.stage(ops, K, padded, W.P8_BIAS)
        for mode in W.ITEM_MODES:
            for cap in W.CAPS + (0,):
                d, rows = W.plan(lib, W.P8, K, cap)
                one = W.ranges_histogram(rows) == {1: 34}
                assert one or cap == 0
                for form in ("atomic", "la"):
                    what = "P8 K=%d %s %s cap %d %s" % (K, "padded" if padded else "exact", mode, cap, form)
                    set_form(monkeypatch, form, mode)
                    W.refill(st, ops)
                    c = go(lib, st, cap, bias=form == "atomic")
                    v = W.bias_of(st)
                    tag = "" if one else " several ranges"
                    worst["C" + tag] = max(worst["C" + tag], W.check_c(c, refs, what))
                    # (the last-arriver form was given no bias: every vector is still its start value)
                    worst["bias" + tag] = max(worst["bias" + tag], W.check_bias(v, refs, ops, W.P8_BIAS if form == "atomic" else (), what))
                    if one:
                        if base_c is None:
                            base_c = c
                        same_bits(c, base_c, what)
                        if form == "atomic":
                            if base_b is None:
                                base_b = v
                            same_bits(v, base_b, what + " bias")
        # the last-arriver form refuses a bias, and the refused call wrote nothing (and used up the armed cap)
        set_form(monkeypatch, "la", "static")
        W.refill(st, ops)
        st.ar.arm()
        assert W.launch(lib, st, stream(), 8, bias=True) != 0 and b"last-arriver" in lib.cmp_last_error()
        st.ar.check()
        same_bits(W.c_of(st), [o[2].float().numpy() for o in ops], "refused launch, C")
        W.check_bias(W.bias_of(st), refs, ops, (), "refused launch")
    print(" WGRAD_ITEMS A K=%d | worst error / limit: %s" % (K, " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


# ------------------------------------------------------------------------------------------ B: the last-arriver fold
@pytest.mark.parametrize("rid", W.S3_ROW_IDS)
def test_last_arriver_fold_bit_for_bit(lib, monkeypatch, rid):
    r = W.row_of(rid)
    K, cap = r["K"], r["cap"]
    ops, refs = W.operands("S3", K, *X_SET), W.references("S3", K, *X_SET)
    emu, parts, pr = fold_of(lib, monkeypatch, K, cap, X_SET)
    d, _ = W.plan(lib, W.S3, K, cap)
    assert d["nslots"] == r["slots"]
    worst = {"la C": 0.0, "atomic C": 0.0, "atomic bias": 0.0, "fold emulation": W.check_c(emu, refs, "S3 %s fold emulation" % rid)}
    for padded in (True, False):
        st = W.stage(ops, K, padded, W.S3_BIAS)
        for mode in W.ITEM_MODES:
            what = "S3 %s %s %s" % (rid, "padded" if padded else "exact", mode)
            set_form(monkeypatch, "la", mode)
            W.refill(st, ops)
            c = go(lib, st, cap, bias=False)
            worst["la C"] = max(worst["la C"], W.check_c(c, refs, what + " la"))
            W.check_bias(W.bias_of(st), refs, ops, (), what + " la")
            assert_fold(c, emu, parts, pr, what + " la")
            # the float-atomic form with the bias sums riding on the same rows: one atomic per K range per element / column -- by bound
            set_form(monkeypatch, "atomic", mode)
            W.refill(st, ops)
            ca = go(lib, st, cap, bias=True)
            worst["atomic C"] = max(worst["atomic C"], W.check_c(ca, refs, what + " atomic"))
            worst["atomic bias"] = max(worst["atomic bias"], W.check_bias(W.bias_of(st), refs, ops, W.S3_BIAS, what + " atomic"))
            if r["slots"] == 0:             # one range per tile: no slot, a null workspace, and the float-atomic form's bits
                same_bits(c, ca, what + " la against the float-atomic form")
    print(" WGRAD_ITEMS B %s | worst error / limit: %s" % (rid, " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("rid", [r["id"] for r in W.MULTI_ROWS])
def test_a_stale_slot_shows(lib, monkeypatch, rid):
    """X, Y, X through one item table, one set of slots and one set of ticket counters: every result its own fold, bit for bit."""
    r = W.row_of(rid)
    K, cap = r["K"], r["cap"]
    sets = {s: (W.operands("S3", K, *s), W.references("S3", K, *s)) + fold_of(lib, monkeypatch, K, cap, s) for s in (X_SET, Y_SET)}
    worst = [0.0]

    def body():
        for padded in (True, False):
            st = W.stage(sets[X_SET][0], K, padded)
            for modes in (("static",) * 3, ("dynamic",) * 3, ("static", "dynamic", "static")):
                got = []
                for n, (s, mode) in enumerate(zip((X_SET, Y_SET, X_SET), modes)):
                    ops, refs, emu, parts, pr = sets[s]
                    what = "S3 %s %s launch %d of X Y X (%s)" % (rid, "padded" if padded else "exact", n, " ".join(modes))
                    set_form(monkeypatch, "la", mode)
                    W.refill(st, ops, operands_too=True)
                    c = go(lib, st, cap, bias=False)
                    worst[0] = max(worst[0], W.check_c(c, refs, what))
                    assert_fold(c, emu, parts, pr, what)
                    got.append(c)
                same_bits(got[2], got[0], "S3 %s: the third launch against the first" % rid)
    on_fresh_thread(body)
    print(" WGRAD_ITEMS B stale %s | worst error / limit: C %.3f" % (rid, worst[0]))


def test_table_and_workspace_rebuilt_in_both_directions(lib, monkeypatch):
    """On one fresh thread: S3 at K = 96 on 16 workgroups (10 slots), K = 1024 uncapped (55: the workspace grows), K = 96 again."""
    small, big = W.row_of("K96-cap16"), W.row_of("K1024-nocap")
    emu = {r["id"]: fold_of(lib, monkeypatch, r["K"], r["cap"], X_SET) for r in (small, big)}
    for r in (small, big):
        assert W.plan(lib, W.S3, r["K"], r["cap"])[0]["nslots"] == r["slots"]
    worst = [0.0]

    def body():
        for padded in (True, False):
            sts = {r["id"]: W.stage(W.operands("S3", r["K"], *X_SET), r["K"], padded) for r in (small, big)}
            got = []
            for n, r in enumerate((small, big, small)):
                ops, refs = W.operands("S3", r["K"], *X_SET), W.references("S3", r["K"], *X_SET)
                what = "rebuild %s launch %d (%s)" % ("padded" if padded else "exact", n, r["id"])
                set_form(monkeypatch, "la", "static")
                W.refill(sts[r["id"]], ops)
                c = go(lib, sts[r["id"]], r["cap"], bias=False)
                worst[0] = max(worst[0], W.check_c(c, refs, what))
                assert_fold(c, *emu[r["id"]], what)
                got.append(c)
            same_bits(got[2], got[0], "rebuild: the third launch against the first")
    on_fresh_thread(body)
    print(" WGRAD_ITEMS B rebuild | worst error / limit: C %.3f" % worst[0])


# ------------------------------------------------------------------------------------------ C: the hook
def test_the_hook_caps_one_grouped_launch_and_reaches_no_gemm(lib, monkeypatch):
    """P8 at K = 64 in the last-arriver form: capped at 8 every tile has one K range, uncapped two -- fl(C0 + acc) against
    fl(C0 + fl(p_0 + p_1)), both reproducible, different in some element.  So: armed, unarmed, unarmed, armed."""
    K = 64
    ops, refs = W.operands("P8", K), W.references("P8", K)
    assert W.ranges_histogram(W.plan(lib, W.P8, K, 8)[1]) == {1: 34} and W.ranges_histogram(W.plan(lib, W.P8, K, 0)[1]) == {2: 34}
    set_form(monkeypatch, "la", "static")
    st = W.stage(ops, K, False)
    got = []
    for cap in (8, 0, 0, 8):
        W.refill(st, ops)
        got.append(go(lib, st, cap, bias=False))
        W.check_c(got[-1], refs, "hook cap %d" % cap)
    same_bits(got[3], got[0], "both capped launches")
    same_bits(got[2], got[1], "both launches behind a consumed cap")
    assert any(W.first_difference(a, b) is not None for a, b in zip(got[0], got[1])), "the launch behind the armed one was capped too"

    # a cap (and rev) armed before a grouped launch does not reach the next cmp_k_gemm: its plan is the unarmed one
    from composer_amd import _lib
    case = next(c for c in IB.CASES if c["id"] == "A-bias-K64")
    gst = IB.stage(case, IB.operands(case), False, device="cpu")

    def grid_of_next_gemm():
        info = _lib.GemmPlanInfo()
        ck(lib, lib.cmp_gemm_plan(*gst.args, C.byref(info)))
        return info.grid_x
    free = grid_of_next_gemm()
    ck(lib, lib.cmp_gemm_grid_next(8, 1))
    assert grid_of_next_gemm() == 8 and free > 8           # (the hook does reach a cmp_k_gemm that follows it directly)
    ck(lib, lib.cmp_gemm_grid_next(8, 1))
    W.refill(st, ops)
    same_bits(go(lib, st, 0, bias=False), got[0], "armed by hand with (8, 1)")
    assert grid_of_next_gemm() == free
    # ... nor does the cap of a refused grouped launch
    st.ar.arm()
    assert W.launch(lib, st, stream(), 5, bias=False) != 0
    st.ar.check()
    assert grid_of_next_gemm() == free


@pytest.mark.parametrize("form", ["atomic", "la"])
def test_caps_that_leave_no_workgroup_are_refused_by_name(lib, monkeypatch, form):
    ops = W.operands("S3", 96, *X_SET)
    set_form(monkeypatch, form, "static")
    st = W.stage(ops, 96, True, W.S3_BIAS if form == "atomic" else ())
    start = [o[2].float().numpy() for o in ops]
    for cap in range(1, 8):
        st.ar.arm()
        assert W.launch(lib, st, stream(), cap) != 0
        msg = lib.cmp_last_error().decode()
        assert "cap of %d workgroups" % cap in msg and "cmp_gemm_grid_next" in msg, msg
        st.ar.check()
        same_bits(W.c_of(st), start, "refused cap %d, C" % cap)
        W.check_bias(W.bias_of(st), W.references("S3", 96, *X_SET), ops, (), "refused cap %d" % cap)
    go(lib, st, 8)                                           # 8 is the smallest grid, and nothing of the refusals is left behind
    W.check_c(W.c_of(st), W.references("S3", 96, *X_SET), "cap 8 after the refusals")


# ------------------------------------------------------------------------------------------ D: one model
def test_model_block_with_more_tiles_than_workgroups(monkeypatch):
    """bf16, one block of E = 320 (H = 5): its four weight-gradient problems have 32 tiles; 96 tokens; a one-rank communicator that
    leaves the GEMMs 8 CUs.  The grouped launch is taken with four items per workgroup and carries the bias gradients; every
    gradient against the float64 oracle and against the same model without the cap."""
    from composer_amd import _lib
    from composer_amd.transformer import Transformer
    from oracle import transformer_oracle as O
    from test_gpu_bias_from_wgrad import BF16_GRAD_TOL, carried, grads_of, worst
    from test_gpu_model import make_model
    V, E, H, L, Wn, T, B = 390, 320, 5, 1, 48, 48, 2
    shapes = [(4 * E, E), (E, 4 * E), (E, E), (E, 3 * E)]
    ip = C.c_int * 4
    info = _lib.WgradPlanInfo()
    Ms, Ns = ip(*[s[0] for s in shapes]), ip(*[s[1] for s in shapes])
    _lib.check(_lib.load().cmp_wgrad_group_plan(4, None, Ms, None, Ns, Ms, Ns, B * T, 8, 0, C.byref(info), None, 0), "cmp_wgrad_group_plan")
    assert info.fits and info.taken and info.tiles == 32 and info.grid == 8 and info.nitems > info.grid, (info.tiles, info.grid, info.nitems)
    monkeypatch.delenv("COMPOSER_BIAS_WGRAD", raising=False)
    monkeypatch.delenv("COMPOSER_WGRAD_TAIL", raising=False)
    monkeypatch.delenv("COMPOSER_GEMM_ITEMS", raising=False)
    params = {k: v.astype(np.float32) for k, v in O.init_params(V, E, Wn, L, seed=23).items()}
    rng = np.random.default_rng(11)
    for k in params:
        if k.endswith(("gamma", "beta", "bias")):
            params[k] = (params[k] + 0.05 * rng.standard_normal(params[k].shape)).astype(np.float32)
    x, y = O.synthetic_batch(rng, V, B, T)
    p = 0.1
    orc = O.OracleTransformer(O.Config(V, E, Wn, L, H, attention_dropout_rate=p, residual_dropout_rate=p), params, seed=99)
    loss, _, G, _ = orc.loss_and_grads(x, y, training=True, step=0)
    res = {}
    for cus in (8, None):
        m = make_model((V, E, H, L, Wn, T, B), params, "bf16", p_attn=p, p_resid=p, seed=99)
        try:
            m.init_data_parallel(0, 1, Transformer.new_unique_id(), gemm_cus=cus)
            l, _ = m.loss_and_grads(x, y)
            res[cus] = (l, grads_of(m), carried(m), list(m.parameter_names))
        finally:
            m.close()
    (l8, g8, c8, names), (l0, g0, c0, _) = res[8], res[None]
    assert (c8, c0) == (1, 1)
    assert abs(l8 - loss) <= 3e-2 * abs(loss) and abs(l8 - l0) <= 1e-6 * abs(l0)
    wo, no = worst(g8, G, names)
    wc, nc = worst(g8, g0, names)
    print(" WGRAD_ITEMS D E=320, 96 tokens, 8 CUs: worst gradient against the oracle %.3g (%s), against the uncapped model %.3g (%s)" % (wo, no, wc, nc))
    assert wo <= BF16_GRAD_TOL, (no, wo)
    assert wc <= BF16_GRAD_TOL, (nc, wc)
