"""The assertions of tests/kernel_arena.py can fail: CPU "kernels" written in torch, indexing a CPU arena through flat pointers the
way device code does, one correct and six wrong in the ways hand-written tile kernels go wrong.  Each wrong one must be rejected by
the check it targets (the arena for stores / loads outside the logical window and unwritten elements, the per-element bound for
arithmetic).  To see that a class of error is caught, edit a copy of `fake_gemm` below -- not the library.
The same for the optimiser: `fake_adam`, a numpy-fp32 statement of the Adam kernels, correct and wrong in ten ways, against
`kernel_arena.adam_check`, plus the record of what the older Adam assertions let through."""
import numpy as np
import pytest
import torch

import kernel_arena as KA
from kernel_arena import Arena

BF, F32 = torch.bfloat16, torch.float32


def operands(M, N, K, seed, lda_pad=8, ldb_pad=16, ldc_pad=8, out_dtype=F32, bias=False, arena_bytes=4 << 20):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(BF)
    b = torch.randn(K, N, generator=g).to(BF)
    ar = Arena("cpu", arena_bytes)
    A = ar.operand(a, BF, M, K, K + lda_pad, name="A")
    B = ar.operand(b, BF, K, N, N + ldb_pad, name="B")
    Cs = ar.output(out_dtype, M, N, N + ldc_pad, name="C")
    bv = ar.vector(torch.randn(N, generator=g).sign() * (1 + 0.1 * torch.rand(N, generator=g)), F32, name="bias") if bias else None
    return ar, A, B, Cs, bv, a.double(), b.double()


def fake_gemm(A, B, Cs, M, N, K, bias=None, bug=None, splitk=1):
    """C[M, N] = A[M, K] . B[K, N] (+ bias) on flat memory: element (i, j) of an operand is mem[i * ld + j], as in a kernel.
    bug: None | 'row_past' | 'col_past' | 'pad_a' | 'unwritten' | 'drop_last_k' | 'bf16_partials' | 'no_bias'."""
    a, b, c = A.mem(), B.mem(), Cs.mem()
    ar = torch.arange
    kk = K + 1 if bug == "pad_a" else (K - 1 if bug == "drop_last_k" else K)      # pad_a: the k-loop runs one column into A's padding
    av = a[ar(M)[:, None] * A.ld + ar(kk)[None, :]].float()
    bv = b[ar(kk).clamp_max(K - 1)[:, None] * B.ld + ar(N)[None, :]].float()
    per = -(-kk // splitk)
    acc = torch.zeros(M, N, dtype=F32)
    for s in range(splitk):                                 # fp32 accumulation, k in order, split-K partials added in order
        part = torch.zeros(M, N, dtype=F32)
        for k in range(s * per, min(kk, (s + 1) * per)):
            part += av[:, k:k + 1] * bv[k:k + 1, :]
        acc += part.to(BF).float() if bug == "bf16_partials" else part
    if bias is not None and bug != "no_bias":
        acc += bias.vec[None, :]
    idx = ar(M)[:, None] * Cs.ld + ar(N)[None, :]
    vals = acc.to(Cs.dtype)
    if bug == "unwritten":
        keep = torch.ones(M, N, dtype=torch.bool); keep[M // 2, N - 1] = False
        idx, vals = idx[keep], vals[keep]
    c[idx] = vals
    if bug == "row_past":
        c[M * Cs.ld] = 1.0           # (row M, column 0): the first element behind the window
    if bug == "col_past":
        c[(M - 1) * Cs.ld + N] = 1.0  # column N of the last row: in-row padding of a padded C


def run(M, N, K, seed, out_dtype=F32, bias=False, **kw):
    ar, A, B, Cs, bv, a, b = operands(M, N, K, seed, out_dtype=out_dtype, bias=bias)
    ar.arm()
    fake_gemm(A, B, Cs, M, N, K, bias=bv, **kw)
    ar.check()
    extra = bv.vec.double().abs()[None, :] if bias else None
    ref, S, f = KA.gemm_bound(a, b, extra)
    if bias:
        ref = ref + bv.vec.double()[None, :]
    return KA.assert_within(Cs.host(), ref, f * S, out_dtype == BF, "fake gemm")


@pytest.mark.parametrize("out_dtype", [F32, BF])
@pytest.mark.parametrize("K", [64, 512, 4096])
def test_correct_fake_gemm_passes(K, out_dtype):
    assert run(48, 48, K, K, out_dtype=out_dtype) <= 1.0
    assert run(40, 24, K, K + 1, out_dtype=out_dtype, bias=True) <= 1.0
    if out_dtype == F32:
        assert run(48, 48, K, K, splitk=8) <= 1.0             # fp32 partials: another summation order, inside the margin


def test_store_behind_the_last_row_is_rejected_by_the_guard():
    with pytest.raises(AssertionError, match=r"guard band overwritten.*AFTER the window of 'C', its element \(row 48, column 0\)"):
        run(48, 48, 64, 1, bug="row_past")


def test_store_into_column_n_of_a_padded_c_is_rejected_by_the_padding_check():
    with pytest.raises(AssertionError, match=r"'C': in-row padding was overwritten at \(row 47, column 48\)"):
        run(48, 48, 64, 1, bug="col_past")


def test_product_over_a_padding_column_of_a_is_rejected():
    with pytest.raises(AssertionError, match=r"'C': element \(row 0, column 0\) is nan: padding"):
        run(48, 48, 64, 1, bug="pad_a")


def test_unwritten_element_is_rejected():
    with pytest.raises(AssertionError, match=r"'C': element \(row 24, column 47\) was never written"):
        run(48, 48, 64, 1, bug="unwritten")


def test_dropped_last_k_at_4096_with_bf16_output_is_rejected_by_the_bound():
    with pytest.raises(AssertionError, match=r"fake gemm: element .* > limit"):
        run(48, 48, 4096, 4096, out_dtype=BF, bug="drop_last_k")


@pytest.mark.parametrize("K", [64, 512, 4096])
def test_bf16_split_k_partials_are_rejected_by_the_bound(K):
    with pytest.raises(AssertionError, match=r"fake gemm: element .* > limit"):
        run(48, 48, K, K, splitk=8, bug="bf16_partials")


@pytest.mark.parametrize("out_dtype", [F32, BF])
def test_omitted_bias_is_rejected_by_the_bound(out_dtype):
    with pytest.raises(AssertionError, match=r"fake gemm: element .* > limit"):
        run(40, 24, 512, 513, out_dtype=out_dtype, bias=True, bug="no_bias")


def test_old_metric_would_have_passed_bf16_partials():
    """What the global max-norm (max|d| / max|ref| < 1.2e-2) could not see: bf16-rounded split-K partials pass it at every K."""
    for K in (64, 512, 4096):
        ar, A, B, Cs, _, a, b = operands(48, 48, K, K)
        fake_gemm(A, B, Cs, 48, 48, K, splitk=8, bug="bf16_partials")
        ref = a @ b
        assert ((Cs.host().double() - ref).abs().max() / ref.abs().max()).item() < 1.2e-2


def comparator(K, seed=None):
    g = torch.Generator().manual_seed(K if seed is None else seed)
    a = torch.randn(48, K, generator=g).to(BF).double()
    b = torch.randn(K, 48, generator=g).to(BF).double()
    q, ref, S = KA.q_seq_of(a, b)
    per = K // 8
    bfp = sum(KA.seq_fp32_matmul(a[:, s * per:(s + 1) * per], b[s * per:(s + 1) * per]).to(BF).double() for s in range(8))
    q_bf = ((bfp - ref).abs() / S).max().item()
    # other fp32 summation orders: blocked (torch's fp32 matmul), reversed, split-K 8 with fp32 partials
    others = [(a.float() @ b.float()).double(), KA.seq_fp32_matmul(a.flip(1), b.flip(0)),
              sum(KA.seq_fp32_matmul(a[:, s * per:(s + 1) * per], b[s * per:(s + 1) * per]).float() for s in range(8)).double()]
    q_other = max(((o - ref).abs() / S).max().item() for o in others)
    return q, q_bf, q_other


def test_comparator_constant():
    """q_seq = max |seq - ref| / (|A|.|B|) of the strictly sequential fp32 dot product, randn operands rounded to bf16, M = N = 48:

        K      q_seq     other fp32 orders   split-K 8, bf16 partials    cap (K + 8) 2^-24
        64     7.7e-08   8.3e-08             1.2e-03                     4.3e-06
        512    7.1e-08   1.0e-07             5.6e-04                     3.1e-05
        4096   1.0e-07   1.3e-07             1.6e-04                     2.4e-04

    (values of this test's seeds; the assertion message prints them).  The bound's factor 8 * q_seq covers every other fp32 order
    measured here, stays below the worst-case cap, and is more than two orders of magnitude below the bf16-partials error."""
    rows = []
    for K in (64, 512, 4096):
        q, q_bf, q_other = comparator(K)
        rows.append((K, q, q_other, q_bf, (K + 8) * KA.EPS24))
        assert 0 < q <= 1.2e-7, rows                           # fp32 accumulation: at most about one ulp of S
        assert q_other <= KA.SEQ_MARGIN * q, rows              # other orders sit inside the margin
        assert KA.acc_factor(q, K) <= (K + 8) * KA.EPS24, rows
        assert 100 * KA.SEQ_MARGIN * q < q_bf, rows            # ... which still separates bf16 partials by > 100x
    print(rows)


def test_store_before_the_first_row_is_rejected_by_the_front_guard():
    ar, A, B, Cs, _, a, b = operands(48, 48, 64, 1)
    ar.arm()
    fake_gemm(A, B, Cs, 48, 48, 64)
    ar.buf[Cs.start - 8:Cs.start - 4] = 0            # one fp32 store two elements in front of C[0, 0]
    with pytest.raises(AssertionError, match=r"AFTER the window of 'B'.* 8 bytes BEFORE the window of 'C': 2 element\(s\) before \(row 0, column 0\)"):
        ar.check()


def test_gemm_case_tables_are_pairwise_covering():
    """The explicit GEMM case tables of tests/test_gpu_kernel_guards.py, each against the valid set of the families that run it
    (rows_of): every pair of values of (layout, M, N, K, epilogue) that the family can run together occurs in some row, and a forced
    family's rows all qualify for the launcher's `fast` dispatch (restated here; tests/test_gemm_plan_host.py asserts the planned
    family itself).  fp32 runs no CMP_GEMM_KPAD_ZERO rows and has its own table."""
    import test_gpu_kernel_guards as G

    def ks(lay, kind):
        if kind == "forced":
            return [(64, 0), (72, 0), (160, 0), (200, 0)] if lay == (1, 0) else [(64, 0), (200, 1)]
        return [(64, 0), (160, 0), (200, 0)] + ([(200, 1)] if kind == "free" else []) + ([(72, 0)] if lay == (1, 0) else [])

    def pairs(c):
        return {((i, c[i]), (j, c[j])) for i in range(5) for j in range(i + 1, 5)}
    assert G.rows_of(G.FP32, 0) is G.FP32_ROWS and G.rows_of(G.BF16, 0) is G.FREE_ROWS and G.rows_of(G.BF16, 2) is G.FREE_ROWS
    assert all(G.rows_of(G.BF16, f) is G.FORCED_ROWS for f in (4, 8, 16, 48))
    assert sorted(G.FAMILIES) == sorted([(G.FP32, 0)] + [(G.BF16, f) for f in (0, 2, 4, 8, 16, 48)])
    for kind, table in (("free", G.FREE_ROWS), ("fp32", G.FP32_ROWS), ("forced", G.FORCED_ROWS)):
        rows = [((ta, tb), M, N, (K, kz), epi) for ta, tb, M, N, K, kz, epi in table]
        valid = [(l, m, n, k, e) for l in G.LAYOUTS for m in (8, 136, 264) for n in (8, 136, 264) for k in ks(l, kind) for e in G.EPILOGUES]
        assert set(rows) <= set(valid), kind
        need = set().union(*[pairs(c) for c in valid])
        assert not need - set().union(*[pairs(c) for c in rows]), kind
        if kind == "forced":
            for (ta, tb), M, N, (K, kz), epi in rows:
                assert K % 64 == 0 or (ta and not tb) or kz


# ------------------------------------------------------------------------------------------ Adam: the bound can fail
# A numpy-fp32 statement of adam_kernel / adam_dev_kernel (csrc/elementwise.hip), unfused: every product, sum, quotient and square
# root rounds once to fp32, in the kernel's order.  It runs on a CPU arena like the GPU cases do, with the arrays flush against
# guards, and is held by KA.adam_check -- the very function tests/test_gpu_adam_update.py applies to the device's results.
ADAM_HYPER = (1e-3, 0.9, 0.999, 1e-7)
ADAM_BUGS = ["step+1", "step-1", "eps_in_sqrt", "eps_scaled", "no_eps", "factor_m_only", "v_beta1", "m0_update", "shadow_truncated", "f_touched"]


def fake_adam(p, g, m, v, sh, n, lr, beta1, beta2, eps, step, factor, bug=None, f_range=None):
    f32 = np.float32
    lr, b1, b2, eps, fac = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(factor)
    t = float(step + {"step+1": 1, "step-1": -1}.get(bug, 0))
    with np.errstate(all="ignore"):
        corr2 = np.sqrt(1.0 - np.power(float(b2), t))
        alpha = f32(float(lr) * corr2 / (1.0 - np.power(float(b1), t)))           # the host wrapper: float64, rounded once
        pv, gv, mv, vv = (s.mem()[:n].numpy().copy() for s in (p, g, m, v))
        gg = gv * fac
        m1 = b1 * mv + (f32(1) - b1) * gg
        gq = gv if bug == "factor_m_only" else gg
        v1 = (b1 if bug == "v_beta1" else b2) * vv + (f32(1) - b2) * gq * gq
        if bug == "eps_in_sqrt":
            den = np.sqrt(v1 + eps)
        elif bug == "eps_scaled":
            den = np.sqrt(v1) + f32(float(eps) * corr2)
        elif bug == "no_eps":
            den = np.sqrt(v1)
        else:
            den = np.sqrt(v1) + eps
        p1 = pv - alpha * (mv if bug == "m0_update" else m1) / den
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    if bug == "f_touched":                                   # one ulp: far inside the bound, only the bitwise claim sees it
        p1[f_range] = np.nextafter(p1[f_range], f32(np.inf))
    for s, a in ((p, p1), (m, m1), (v, v1)):
        s.mem()[:n] = torch.from_numpy(a)
    pt = torch.from_numpy(p1)
    sh.mem()[:n] = KA.bf16_truncated(pt) if bug == "shadow_truncated" else pt.to(BF)


def run_adam(step, factor, bug=None, lr=ADAM_HYPER[0], inputs=None):
    inp, seg = inputs or KA.adam_inputs(factor)
    n = inp["p0"].numel()
    ar = Arena("cpu", 1 << 20)
    p, m, v = (ar.vector(inp[k], F32, name=k[0], kind="acc") for k in ("p0", "m0", "v0"))
    g = ar.vector(inp["g"], F32, name="g")
    sh = ar.output(BF, 1, n, n, name="shadow")
    ar.arm()
    fake_adam(p, g, m, v, sh, n, lr, *ADAM_HYPER[1:], step, factor, bug=bug, f_range=seg["f"])
    ar.check()
    return KA.adam_check(inp, seg, p.host()[0], m.host()[0], v.host()[0], sh.host()[0], lr, *ADAM_HYPER[1:], step, factor, "fake adam")


def test_adam_inputs_are_what_the_cases_need():
    inp, seg = KA.adam_inputs(1.0 / 3.0)
    n = inp["p0"].numel()
    assert n % 4 == 0 and n % 1024 != 0 and n // 4 > 256 and all((s.stop - s.start) % 4 == 0 for s in seg.values())
    assert sum(s.stop - s.start for s in seg.values()) == n
    _, _, v1 = KA.adam_reference(inp["p0"], inp["g"], inp["m0"], inp["v0"], *ADAM_HYPER, 1, 1.0 / 3.0)
    sq = np.sqrt(v1[seg["d"]])
    assert sq.min() < 0.03e-7 and (sq < 1e-7).sum() > 100 and (sq > 1e-7).sum() > 100 and 10e-7 < sq.max() <= 32e-7   # both sides of eps, up to 30 eps
    gf = np.abs(inp["g"][seg["d"]].double().numpy() * float(np.float32(1.0 / 3.0)))
    assert 0.99e-9 <= gf.min() < 1e-8 and 1e-5 < gf.max() <= 1.01e-4
    assert inp["g"][seg["g"]].abs().max() > 1e3


@pytest.mark.parametrize("factor", [1.0, 0.5, 1.0 / 3.0])
def test_correct_fake_adam_passes(factor):
    """The numbers `adam_bounds` quotes: worst error / limit of the unfused numpy-fp32 statement over t = 1, 7, 1000 (and the two
    steps at which beta^t underflows) -- p 0.50, m 0.31, v 0.38 at most (the run prints them per factor)."""
    worst = {}
    for step in (1, 2, 7, 1000, 10 ** 6, 2 ** 31 + 5):
        w = run_adam(step, factor)
        worst = {k: max(worst.get(k, 0.0), x) for k, x in w.items()}
    print("factor", factor, "worst error/limit", worst)
    assert all(0 < x <= 1.0 for x in worst.values())
    run_adam(7, factor, lr=0.0)                                  # p bitwise unchanged, m and v moved


@pytest.mark.parametrize("step", [1, 7, 1000])
@pytest.mark.parametrize("bug", ADAM_BUGS)
def test_wrong_fake_adam_is_rejected(bug, step):
    """Every variant at every step: by the per-element bound (on p, or on v for the two that spoil v), by the arena's non-finite
    check (no eps: 0 / 0 in segment f; step - 1 at t = 1: alpha = 0 / 0), by the shadow's bitwise claim, or by segment f's."""
    match = {"shadow_truncated": "round-to-nearest-even image", "f_touched": "g = m = v = 0 was touched"}.get(bug, r"> limit|is nan|is inf|is -inf")
    with pytest.raises(AssertionError, match=match):
        run_adam(step, 0.5, bug=bug)


def test_old_metric_would_have_passed_a_wrong_eps_and_a_wrong_step():
    """The gap, written down.  The older Adam assertions (test_adam_keras_formulation, test_adam_guarded: max|d| / max|ref| < 1e-6 for
    m, v and p with max|p| about 4, the shadow equal to the rounded p) on their own inputs (v0 ~ U(0, 0.01): sqrt(v) >> eps
    everywhere) pass eps scaled by sqrt(1 - beta2^t) and no eps at all at t = 1, 7 and 1000, and a step count off by one in either
    direction at t = 1000."""
    n = 4096 + 8
    gen = torch.Generator().manual_seed(9)
    p0, gr = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1
    m0, v0 = torch.randn(n, generator=gen) * 0.01, torch.rand(n, generator=gen) * 0.01
    inputs = ({"p0": p0, "g": gr, "m0": m0, "v0": v0}, {"f": slice(0, 0)})

    def rel_err(a, b):
        return ((a.double() - b).abs().max() / (b.abs().max() + 1e-30)).item()
    for step, bugs in ((1, ("eps_scaled", "no_eps")), (7, ("eps_scaled", "no_eps")), (1000, ("eps_scaled", "no_eps", "step+1", "step-1"))):
        g64 = gr.double() * 0.5
        m1 = 0.9 * m0.double() + 0.1 * g64
        v1 = 0.999 * v0.double() + 0.001 * g64 * g64
        alpha = 1e-3 * (1 - 0.999 ** step) ** 0.5 / (1 - 0.9 ** step)
        p1 = p0.double() - alpha * m1 / (v1.sqrt() + 1e-7)
        for bug in bugs:
            ar = Arena("cpu", 1 << 20)
            p, m, v = (ar.vector(t, F32, name=nm, kind="acc") for t, nm in ((p0, "p"), (m0, "m"), (v0, "v")))
            g = ar.vector(gr, F32, name="g")
            sh = ar.output(BF, 1, n, n, name="shadow")
            fake_adam(p, g, m, v, sh, n, *ADAM_HYPER, step, 0.5, bug=bug)
            assert rel_err(m.host()[0], m1) < 1e-6 and rel_err(v.host()[0], v1) < 1e-6 and rel_err(p.host()[0], p1) < 1e-6, (step, bug)
            assert torch.equal(sh.host()[0], p.host()[0].to(BF))
            # ... and the new bound sees each of them on the same old inputs?  Only the wrong step: eps needs the new segments.
            if bug.startswith("step"):
                with pytest.raises(AssertionError, match="> limit"):
                    KA.adam_check(inputs[0], inputs[1], p.host()[0], m.host()[0], v.host()[0], None, *ADAM_HYPER, step, 0.5, "old inputs")
