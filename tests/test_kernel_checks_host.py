"""The assertions of tests/kernel_arena.py can fail: CPU "kernels" written in torch, indexing a CPU arena through flat pointers the
way device code does, one correct and six wrong in the ways hand-written tile kernels go wrong.  Each wrong one must be rejected by
the check it targets (the arena for stores / loads outside the logical window and unwritten elements, the per-element bound for
arithmetic).  To see that a class of error is caught, edit a copy of `fake_gemm` below -- not the library."""
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
    family's rows all qualify for gemm_run's `fast` dispatch.  fp32 runs no CMP_GEMM_KPAD_ZERO rows and has its own table."""
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
