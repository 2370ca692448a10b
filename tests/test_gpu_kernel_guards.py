"""-m gpu: every kernel-level entry point of the training path inside a guard-banded arena (tests/kernel_arena.py), at the smallest
shapes that still have a ragged edge in every tiled dimension, with leading dimensions wider than the logical rows, and -- for the
GEMMs, the grouped weight-gradient launch and the column sums -- a per-element error bound derived from fp32 accumulation instead of
one global max-norm.  tests/test_kernel_checks_host.py shows on the CPU that each of these assertions can fail.

What a case proves beyond the value comparison: no byte outside an output's logical window changed (guards before and behind every
operand, in-row padding), no input changed, every element of a fully written output was written, and neither NaN padding nor a
neighbour's bytes reached a stored value.  Padding that feeds nothing the kernel stores (columns m >= M of a transposed A, n >= N
of B) may be read: it is NaN here, so the test shows it cannot reach a stored value.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import kernel_arena as KA
import test_gpu_kernels as TK
from kernel_arena import Arena
from oracle import transformer_oracle as O

pytestmark = pytest.mark.gpu

FP32, BF16 = 0, 1
F32, BF, I32 = torch.float32, torch.bfloat16, torch.int32
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from composer_amd import _lib
    l = _lib.load()
    _lib.require_gpu()
    return l


def ck(lib, rc):
    assert rc == 0, lib.cmp_last_error().decode()


def tdt(dtype):
    return BF if dtype == BF16 else F32


def P(slot):
    return C.c_void_p(slot.ptr()) if slot is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rounded(t, dtype):
    """float64 values of t as rounded to the compute dtype."""
    return t.to(tdt(dtype)).double()


# ------------------------------------------------------------------------------------------ GEMM
# Kernel families: (dtype, flags).  The launcher's plan (csrc/gemm_plan.h) takes a forced kernel (flags 4 / 8 / 16 / 48) only when the
# shape is `fast`: K % 64 == 0, or (ta && !tb), or CMP_GEMM_KPAD_ZERO with both K-contiguous strides >= K rounded up to 64; ldc,
# ldaux, ldr multiples of 8; N % 8 == 0 unless out_fp32 -- otherwise it runs the generic kernel (tests/test_gemm_plan_host.py
# asserts on the CPU that every row reaches the family it is meant for).  Every M, N and every
# stride below is a multiple of 8, so `fast` is decided by K and the layout alone: FORCED_ROWS holds only rows that qualify (each
# names why), FREE_ROWS says per row which kernel flags 0 picks, FP32_ROWS always run gemm_f32_kernel (these shapes are never `big`: M * N < 512 * 512).
FAMILIES = [(FP32, 0), (BF16, 0), (BF16, 2), (BF16, 4), (BF16, 8), (BF16, 16), (BF16, 48)]
FAMILY_IDS = ["fp32", "bf16-auto", "bf16-generic", "bf16-tile128", "bf16-tile256", "bf16-p4-256", "bf16-p4-128"]
# flags 4: gemm_bf16_fast_kernel (128x128 direct-to-LDS); 8: gemm_bf16_256_kernel (persistent 256x256, 2-stage BK=64); 16:
# gemm_bf16_p4_kernel<.., 2, 4> (deep pipeline 256x256, BK=32); 48: gemm_bf16_p4_kernel<.., 1, 3> (128x256).
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
EPILOGUES = ["none", "bias", "gelu", "gelugrad", "resid", "drop", "f32"]

# Pairwise-covering subsets of layout x M x N x K x epilogue, one table per group of families: every pair of values that the
# group can run together occurs in some row of ITS table (tests/test_kernel_checks_host.py checks each table against the
# group's own valid set).  Columns: ta, tb, M, N, K, kz (CMP_GEMM_KPAD_ZERO: K-contiguous rows zero-padded to 256), epilogue.
#   FREE_ROWS    bf16, flags 0 and 2: K in 64, 160, 200, 200 + kz; 72 for (ta, tb) = (1, 0).
#   FP32_ROWS    fp32 (the flag means nothing there): K in 64, 160, 200; 72 for (1, 0); no kz rows.
#   FORCED_ROWS  bf16, flags 4, 8, 16, 48: only rows that qualify as `fast`.
FREE_ROWS = [
    (0, 0,   8, 136, 160, 0, "f32"),     # flags 0: generic; flags 2: generic
    (0, 0, 264, 264, 160, 0, "drop"),    # flags 0: generic; flags 2: generic
    (0, 0,   8, 136, 200, 0, "resid"),   # flags 0: generic; flags 2: generic
    (0, 0, 264, 264, 200, 0, "drop"),    # flags 0: generic; flags 2: generic
    (0, 0, 264, 264, 200, 0, "bias"),    # flags 0: generic; flags 2: generic
    (0, 0, 136, 136, 200, 1, "gelugrad"), # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (0, 0, 264, 264, 200, 1, "bias"),    # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (0, 0, 264, 264, 200, 1, "gelu"),    # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (0, 0, 136,   8,  64, 0, "gelu"),    # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (0, 0, 264, 264,  64, 0, "none"),    # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (0, 1, 136, 264, 160, 0, "bias"),    # flags 0: generic; flags 2: generic
    (0, 1, 264, 264, 160, 0, "none"),    # flags 0: generic; flags 2: generic
    (0, 1, 264, 136, 200, 0, "gelu"),    # flags 0: generic; flags 2: generic
    (0, 1, 264, 264, 200, 0, "f32"),     # flags 0: generic; flags 2: generic
    (0, 1,   8,   8, 200, 1, "drop"),    # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (0, 1, 136, 264,  64, 0, "resid"),   # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (0, 1, 264, 264,  64, 0, "gelugrad"), # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (1, 0, 264,   8, 160, 0, "resid"),   # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (1, 0,   8, 264, 200, 0, "gelugrad"), # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (1, 0,   8, 136, 200, 1, "none"),    # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (1, 0, 136,   8,  64, 0, "f32"),     # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (1, 0,   8, 264,  72, 0, "gelu"),    # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (1, 0, 136, 136,  72, 0, "drop"),    # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (1, 0, 264,   8,  72, 0, "bias"),    # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (1, 0, 264, 264,  72, 0, "none"),    # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (1, 0, 264, 264,  72, 0, "gelugrad"), # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (1, 0, 264, 264,  72, 0, "resid"),   # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (1, 0, 264, 264,  72, 0, "f32"),     # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (1, 1, 264,   8, 160, 0, "gelugrad"), # flags 0: generic; flags 2: generic
    (1, 1, 264, 264, 160, 0, "gelu"),    # flags 0: generic; flags 2: generic
    (1, 1, 136,   8, 200, 0, "none"),    # flags 0: generic; flags 2: generic
    (1, 1, 264, 264, 200, 1, "f32"),     # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (1, 1, 264, 264, 200, 1, "resid"),   # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (1, 1,   8, 136,  64, 0, "bias"),    # flags 0: 128x128 direct-to-LDS; flags 2: generic
    (1, 1, 264, 264,  64, 0, "drop"),    # flags 0: 128x128 direct-to-LDS; flags 2: generic
]
# FREE_ROWS row by row: the kernel family flags 0 picks (the comments above, as data; flags 2 always picks "generic").  Asserted on the
# CPU against the launcher's plan by tests/test_gemm_plan_host.py.
FREE_AUTO = [
    "generic", "generic", "generic", "generic", "generic", "tile128", "tile128",
    "tile128", "tile128", "tile128", "generic", "generic", "generic", "generic",
    "tile128", "tile128", "tile128", "tile128", "tile128", "tile128", "tile128",
    "tile128", "tile128", "tile128", "tile128", "tile128", "tile128", "tile128",
    "generic", "generic", "generic", "tile128", "tile128", "tile128", "tile128",
]
FP32_ROWS = [
    (0, 0,   8, 264,  64, 0, "gelu"),    # gemm_f32_kernel (64x64x16 tiles: whole k-steps)
    (0, 0, 264,   8,  64, 0, "gelugrad"), # gemm_f32_kernel (64x64x16 tiles: whole k-steps)
    (0, 0, 264, 264,  64, 0, "none"),    # gemm_f32_kernel (64x64x16 tiles: whole k-steps)
    (0, 0,   8, 136, 160, 0, "f32"),     # gemm_f32_kernel (64x64x16 tiles: whole k-steps)
    (0, 0,   8,   8, 200, 0, "resid"),   # gemm_f32_kernel (64x64x16 tiles: ragged last k-step)
    (0, 0, 136, 264, 200, 0, "drop"),    # gemm_f32_kernel (64x64x16 tiles: ragged last k-step)
    (0, 0, 264, 136, 200, 0, "bias"),    # gemm_f32_kernel (64x64x16 tiles: ragged last k-step)
    (0, 1,   8,   8,  64, 0, "bias"),    # gemm_f32_kernel (64x64x16 tiles: whole k-steps)
    (0, 1, 136,   8,  64, 0, "f32"),     # gemm_f32_kernel (64x64x16 tiles: whole k-steps)
    (0, 1, 264, 264,  64, 0, "resid"),   # gemm_f32_kernel (64x64x16 tiles: whole k-steps)
    (0, 1, 264, 264,  64, 0, "drop"),    # gemm_f32_kernel (64x64x16 tiles: whole k-steps)
    (0, 1, 136, 136, 160, 0, "gelugrad"), # gemm_f32_kernel (64x64x16 tiles: whole k-steps)
    (0, 1, 136, 264, 160, 0, "bias"),    # gemm_f32_kernel (64x64x16 tiles: whole k-steps)
    (0, 1, 264, 264, 160, 0, "none"),    # gemm_f32_kernel (64x64x16 tiles: whole k-steps)
    (0, 1, 264, 136, 200, 0, "gelu"),    # gemm_f32_kernel (64x64x16 tiles: ragged last k-step)
    (1, 0, 136, 136,  64, 0, "resid"),   # gemm_f32_kernel (64x64x16 tiles: whole k-steps)
    (1, 0,   8, 136,  72, 0, "none"),    # gemm_f32_kernel (64x64x16 tiles: ragged last k-step)
    (1, 0, 136,   8,  72, 0, "gelu"),    # gemm_f32_kernel (64x64x16 tiles: ragged last k-step)
    (1, 0, 264, 264,  72, 0, "f32"),     # gemm_f32_kernel (64x64x16 tiles: ragged last k-step)
    (1, 0, 264, 264,  72, 0, "bias"),    # gemm_f32_kernel (64x64x16 tiles: ragged last k-step)
    (1, 0, 264, 264,  72, 0, "gelugrad"), # gemm_f32_kernel (64x64x16 tiles: ragged last k-step)
    (1, 0, 264, 264,  72, 0, "resid"),   # gemm_f32_kernel (64x64x16 tiles: ragged last k-step)
    (1, 0, 264, 264,  72, 0, "drop"),    # gemm_f32_kernel (64x64x16 tiles: ragged last k-step)
    (1, 0, 264,   8, 160, 0, "drop"),    # gemm_f32_kernel (64x64x16 tiles: whole k-steps)
    (1, 0,   8, 264, 200, 0, "gelugrad"), # gemm_f32_kernel (64x64x16 tiles: ragged last k-step)
    (1, 1,   8, 136,  64, 0, "drop"),    # gemm_f32_kernel (64x64x16 tiles: whole k-steps)
    (1, 1, 264, 264,  64, 0, "bias"),    # gemm_f32_kernel (64x64x16 tiles: whole k-steps)
    (1, 1, 264, 264,  64, 0, "gelugrad"), # gemm_f32_kernel (64x64x16 tiles: whole k-steps)
    (1, 1, 264, 264, 160, 0, "resid"),   # gemm_f32_kernel (64x64x16 tiles: whole k-steps)
    (1, 1, 264, 264, 160, 0, "gelu"),    # gemm_f32_kernel (64x64x16 tiles: whole k-steps)
    (1, 1, 136,   8, 200, 0, "none"),    # gemm_f32_kernel (64x64x16 tiles: ragged last k-step)
    (1, 1, 264, 264, 200, 0, "f32"),     # gemm_f32_kernel (64x64x16 tiles: ragged last k-step)
]
FORCED_ROWS = [
    (0, 0,   8, 136, 200, 1, "resid"),   # fast (KPAD_ZERO, rows padded to 256)
    (0, 0, 136, 264, 200, 1, "drop"),    # fast (KPAD_ZERO, rows padded to 256)
    (0, 0, 264,   8, 200, 1, "gelu"),    # fast (KPAD_ZERO, rows padded to 256)
    (0, 0,   8,   8,  64, 0, "bias"),    # fast (K % 64 == 0)
    (0, 0, 264, 264,  64, 0, "none"),    # fast (K % 64 == 0)
    (0, 0, 264, 264,  64, 0, "gelugrad"), # fast (K % 64 == 0)
    (0, 0, 264, 264,  64, 0, "f32"),     # fast (K % 64 == 0)
    (0, 1,   8, 136, 200, 1, "none"),    # fast (KPAD_ZERO, rows padded to 256)
    (0, 1, 136, 264, 200, 1, "bias"),    # fast (KPAD_ZERO, rows padded to 256)
    (0, 1,   8,   8,  64, 0, "drop"),    # fast (K % 64 == 0)
    (0, 1, 136,   8,  64, 0, "resid"),   # fast (K % 64 == 0)
    (0, 1, 264, 136,  64, 0, "f32"),     # fast (K % 64 == 0)
    (0, 1, 264, 264,  64, 0, "gelu"),    # fast (K % 64 == 0)
    (0, 1, 264, 264,  64, 0, "gelugrad"), # fast (K % 64 == 0)
    (1, 0,   8, 264, 160, 0, "gelu"),    # fast (ta && !tb: descriptor range check)
    (1, 0, 136,   8, 160, 0, "f32"),     # fast (ta && !tb: descriptor range check)
    (1, 0, 264, 136, 160, 0, "drop"),    # fast (ta && !tb: descriptor range check)
    (1, 0, 264, 264, 160, 0, "none"),    # fast (ta && !tb: descriptor range check)
    (1, 0, 264, 264, 160, 0, "bias"),    # fast (ta && !tb: descriptor range check)
    (1, 0, 264, 264, 160, 0, "gelugrad"), # fast (ta && !tb: descriptor range check)
    (1, 0, 264, 264, 160, 0, "resid"),   # fast (ta && !tb: descriptor range check)
    (1, 0,   8, 136, 200, 0, "gelugrad"), # fast (ta && !tb: descriptor range check)
    (1, 0, 136,   8, 200, 0, "none"),    # fast (ta && !tb: descriptor range check)
    (1, 0, 264, 264, 200, 0, "resid"),   # fast (ta && !tb: descriptor range check)
    (1, 0, 264, 264, 200, 0, "bias"),    # fast (ta && !tb: descriptor range check)
    (1, 0, 264, 264, 200, 0, "gelu"),    # fast (ta && !tb: descriptor range check)
    (1, 0, 264, 264, 200, 0, "drop"),    # fast (ta && !tb: descriptor range check)
    (1, 0, 264, 264, 200, 0, "f32"),     # fast (ta && !tb: descriptor range check)
    (1, 0, 264, 264,  64, 0, "none"),    # fast (K % 64 == 0)
    (1, 0,   8,   8,  72, 0, "none"),    # fast (ta && !tb: descriptor range check)
    (1, 0, 136, 264,  72, 0, "gelugrad"), # fast (ta && !tb: descriptor range check)
    (1, 0, 264, 136,  72, 0, "bias"),    # fast (ta && !tb: descriptor range check)
    (1, 0, 264, 264,  72, 0, "gelu"),    # fast (ta && !tb: descriptor range check)
    (1, 0, 264, 264,  72, 0, "resid"),   # fast (ta && !tb: descriptor range check)
    (1, 0, 264, 264,  72, 0, "drop"),    # fast (ta && !tb: descriptor range check)
    (1, 0, 264, 264,  72, 0, "f32"),     # fast (ta && !tb: descriptor range check)
    (1, 1,   8, 264, 200, 1, "f32"),     # fast (KPAD_ZERO, rows padded to 256)
    (1, 1, 264,   8, 200, 1, "gelugrad"), # fast (KPAD_ZERO, rows padded to 256)
    (1, 1, 136, 136,  64, 0, "gelu"),    # fast (K % 64 == 0)
    (1, 1, 264, 264,  64, 0, "none"),    # fast (K % 64 == 0)
    (1, 1, 264, 264,  64, 0, "bias"),    # fast (K % 64 == 0)
    (1, 1, 264, 264,  64, 0, "resid"),   # fast (K % 64 == 0)
    (1, 1, 264, 264,  64, 0, "drop"),    # fast (K % 64 == 0)
]


def rows_of(dtype, flags):
    if dtype == FP32:
        return FP32_ROWS
    return FREE_ROWS if flags in (0, 2) else FORCED_ROWS


_OPS = {}


def logical_ops(dtype, M, N, K):
    """Logical a [M, K], b [K, N] as rounded to the compute dtype (float64), the float64 product, S = |a|.|b| and q_seq -- computed
    once per shape and shared by every layout, stride regime and epilogue."""
    key = (dtype, M, N, K)
    if key not in _OPS:
        g = torch.Generator().manual_seed(M * 7 + N * 3 + K + dtype)
        a = rounded(torch.randn(M, K, generator=g), dtype)
        b = rounded(torch.randn(K, N, generator=g) * 0.2, dtype)
        q, ref, S = KA.q_seq_of(a, b)
        bias = torch.randn(N, generator=g).double()
        resid = rounded(torch.randn(M, N, generator=g), dtype)
        pre = rounded(torch.randn(M, N, generator=g), dtype)
        c0 = torch.randn(M, N, generator=g).double()
        _OPS[key] = dict(a=a, b=b, q=q, ref=ref, S=S, bias=bias, resid=resid, pre=pre, c0=c0, f=KA.acc_factor(q, K))
    return _OPS[key]


def stage_ab(ar, dtype, ta, tb, M, N, K, kz, pa, pb, o):
    """A and B as the layout stores them.  K-contiguous operands (A when !ta, B when tb) of a kz case hold zeros in columns
    K..256 (the CMP_GEMM_KPAD_ZERO contract) and NaN behind them; every other padding is NaN."""
    dt = tdt(dtype)
    Kp = 256 if kz else K

    def kcontig(x, rows, pad, name):
        h = torch.zeros(rows, Kp, dtype=torch.float64); h[:, :K] = x
        return ar.operand(h, dt, rows, Kp, Kp + pad, name=name)
    A = ar.operand(o["a"].t(), dt, K, M, M + pa, name="A") if ta else kcontig(o["a"], M, pa, "A")
    B = kcontig(o["b"].t(), N, pb, "B") if tb else ar.operand(o["b"], dt, K, N, N + pb, name="B")
    return A, B


def gemm_args(dtype, ta, tb, M, N, K, A, B, Cs, bias=None, act=0, aux=None, resid=None, out_fp32=0, splitk=1, p=0.0,
              seed=0, rng=0, flags=0):
    """The arguments of cmp_k_gemm behind the stream (cmp_gemm_plan takes the same list)."""
    return (dtype, ta, tb, M, N, K, P(A), A.ld, P(B), B.ld, P(Cs), Cs.ld, P(bias), act, P(aux),
            aux.ld if aux is not None else 0, P(resid), resid.ld if resid is not None else 0, out_fp32, splitk, p, seed, rng, flags)


def launch_gemm(lib, *a, **kw):
    ck(lib, lib.cmp_k_gemm(stream(), *gemm_args(*a, **kw)))


GELU_ALLOWANCE = {}       # (what, dtype) -> the largest fp32-evaluation allowance a case used (printed with -s)
WORST = {}                # (dtype, flags) -> the largest error / limit any GEMM element reached (printed with -s)


def stage_gemm_case(dtype, flags, ta, tb, M, N, K, kz, epi, padded, device="cuda"):
    """The arena and the cmp_k_gemm arguments of one table row: (arena, logical operands, C, aux, arguments).  On device "cpu" the
    same strides, flags and epilogue operands with host pointers (tests/test_gemm_plan_host.py plans them, nothing runs)."""
    o = logical_ops(dtype, M, N, K)
    dt = tdt(dtype)
    pa, pb, pc, pu, pr = (8, 16, 16, 8, 8) if padded else (0, 0, 0, 0, 0)        # lda, ldb, ldc, ldaux, ldr: not all equal
    ar = Arena(device, 3 << 20)
    A, B = stage_ab(ar, dtype, ta, tb, M, N, K, kz, pa, pb, o)
    out_f32 = epi == "f32"
    bf16_out = dtype == BF16 and not out_f32
    Cs = ar.output(F32 if (out_f32 or dtype == FP32) else dt, M, N, N + pc, name="C")
    bias = ar.vector(o["bias"], F32, name="bias") if epi in ("bias", "gelu", "resid", "drop") else None
    aux = resid = None
    if epi == "gelu":
        aux = ar.output(dt, M, N, N + pu, name="aux")
    if epi == "gelugrad":
        aux = ar.operand(o["pre"], dt, M, N, N + pu, name="aux")
    if epi in ("resid", "drop"):
        resid = ar.operand(o["resid"], dt, M, N, N + pr, name="resid")
    kw = dict(bias=bias, aux=aux, resid=resid, out_fp32=int(out_f32), flags=flags | (1 if kz else 0))
    if epi == "gelu":
        kw["act"] = 1
    if epi == "gelugrad":
        kw["act"] = 2
    if epi == "drop":
        kw.update(p=0.25, seed=77, rng=9)
    return ar, o, Cs, aux, gemm_args(dtype, ta, tb, M, N, K, A, B, Cs, **kw)


def gemm_case(lib, dtype, flags, ta, tb, M, N, K, kz, epi, padded):
    ar, o, Cs, aux, args = stage_gemm_case(dtype, flags, ta, tb, M, N, K, kz, epi, padded)
    out_f32 = epi == "f32"
    bf16_out = dtype == BF16 and not out_f32
    ar.arm()
    ck(lib, lib.cmp_k_gemm(stream(), *args))
    ar.check()
    what = "gemm dtype=%d flags=%d ta=%d tb=%d M=%d N=%d K=%d kz=%d %s %s" % (dtype, flags, ta, tb, M, N, K, kz, epi, "padded" if padded else "exact")
    out, ref, S, f = Cs.host(), o["ref"], o["S"], o["f"]
    bb = o["bias"][None, :]

    def within(*a, **k):
        WORST[(dtype, flags)] = max(WORST.get((dtype, flags), 0.0), KA.assert_within(*a, **k))
    if epi in ("none", "f32"):
        within(out, ref, f * S, bf16_out, what)
    elif epi == "bias":
        within(out, ref + bb, f * (S + bb.abs()), bf16_out, what)
    elif epi == "gelu":
        pre = ref + bb
        acc = f * (S + bb.abs())
        within(aux.host(), pre, acc, bf16_out, what + " aux")
        allow = KA.f32_eval_allowance(O.gelu, pre.numpy())
        GELU_ALLOWANCE[("gelu", dtype)] = max(allow, GELU_ALLOWANCE.get(("gelu", dtype), 0.0))
        within(out, torch.from_numpy(O.gelu(pre.numpy())), 1.13 * acc, bf16_out, what, extra=allow)       # max |gelu'| < 1.13
    elif epi == "gelugrad":
        gg = torch.from_numpy(O.gelu_grad(o["pre"].numpy()))
        allow = KA.f32_eval_allowance(O.gelu_grad, o["pre"].numpy())
        GELU_ALLOWANCE[("gelu_grad", dtype)] = max(allow, GELU_ALLOWANCE.get(("gelu_grad", dtype), 0.0))
        # an error dg of the factor moves the product by |a.b| dg
        within(out, ref * gg, f * S * gg.abs(), bf16_out, what, extra=ref.abs() * allow)
    elif epi == "resid":
        within(out, ref + bb + o["resid"], f * (S + bb.abs() + o["resid"].abs()), bf16_out, what)
    elif epi == "drop":
        # the mask is a hash of (seed, stream, row, column): the oracle's, whatever ldc is
        keep = torch.from_numpy(O.dropout_keep_rows(77, 9, M, N, 0.25))
        scale = keep.double() / 0.75
        within(out, (ref + bb) * scale + o["resid"], f * ((S + bb.abs()) * scale + o["resid"].abs()), bf16_out, what)
        assert torch.equal(out.double()[~keep], o["resid"][~keep]), what + ": a dropped element is not exactly resid"


@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_gemm_guarded(lib, family, ta, tb):
    """cmp_k_gemm, every family x layout: the family's table rows of this layout, each once with every stride 8 or 16 elements wider
    than the logical row and once with exact strides; the dropout rows so run with ldc > N and with ldc == N (the model's case).

    fp32 allowance for evaluating gelu / gelu' (4 x numpy's float32 evaluation against float64, max over a case; measured here,
    largest over all cases): gelu 2.7e-06, gelu' 2.5e-06.  act=1 adds the allowance to the limit as it is (the function value IS
    the output).  act=2 does NOT add it plainly: the output is (a.b)_ij * gelu'(aux_ij), so an error dg of the factor moves the
    output by |(a.b)_ij| dg, and the term added to element (i, j) is |ref_ij| * allowance with ref = the float64 product.  Where
    |ref_ij| > 1 (it reaches about 10 at K = 200) this is looser than a plain additive allowance, where |ref_ij| < 1 tighter; it
    stays 3e-5 at most, far below the bf16 output rounding 2^-8 |out| and of the order of the accumulation term in fp32."""
    dtype, flags = family
    for (ta_, tb_, M, N, K, kz, epi) in rows_of(dtype, flags):
        if (ta_, tb_) == (ta, tb):
            for padded in (True, False):
                gemm_case(lib, dtype, flags, ta, tb, M, N, K, kz, epi, padded)
    print(" %s (%d, %d): worst error / limit %.3f; fp32 evaluation allowances %s" % (family, ta, tb, WORST.get(family, 0.0),
          {k: "%.2g" % v for k, v in GELU_ALLOWANCE.items() if k[1] == dtype}))


SPLIT_K_MODES = ("slab", "none", "atomic")


def stage_split_k(lib, dtype, flags, ta, tb, M, N, K, o, padded, splitk, mode, device="cuda"):
    """One launch of the split-K test: registers the slab workspace (or none) and returns (arena, C, cmp_k_gemm arguments)."""
    ar = Arena(device, 8 << 20)
    A, B = stage_ab(ar, dtype, ta, tb, M, N, K, 0, 8 if padded else 0, 16 if padded else 0, o)
    Cs = ar.accumulator(o["c0"], F32, M, N, N + (16 if padded else 0), name="C")
    ws = ar.scratch(splitk * M * N * 4, name="slab workspace")
    ck(lib, lib.cmp_gemm_set_workspace(P(ws) if mode != "none" else None, ws.nbytes if mode != "none" else 0))
    return ar, Cs, gemm_args(dtype, ta, tb, M, N, K, A, B, Cs, out_fp32=1, splitk=splitk, flags=flags | (128 if mode == "atomic" else 0))


@pytest.mark.parametrize("ta,tb", [(1, 0), (0, 0)])
@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_gemm_split_k_guarded(lib, family, ta, tb):
    """out_fp32 + splitk 2 and 8 onto a non-zero C at K = 4096, M = N = 136: with a registered slab workspace (exactly
    splitk * M * N floats, flush against a guard; the deep-pipeline kernels then fold per-split slabs in a fixed order when
    ldc == N), without one (f32 atomics), and with flag 128 (atomics forced).  K % 64 == 0: every forced family is reached."""
    dtype, flags = family
    M = N = 136
    K = 4096
    o = logical_ops(dtype, M, N, K)
    ref, S = o["ref"] + o["c0"], o["S"] + o["c0"].abs()
    try:
        for padded in (True, False):
            for splitk in (2, 8):
                for mode in SPLIT_K_MODES:
                    ar, Cs, args = stage_split_k(lib, dtype, flags, ta, tb, M, N, K, o, padded, splitk, mode)
                    ar.arm()
                    ck(lib, lib.cmp_k_gemm(stream(), *args))
                    ar.check()
                    KA.assert_within(Cs.host(), ref, o["f"] * S, False, "split-K dtype=%d flags=%d ta=%d tb=%d splitk=%d %s %s"
                                     % (dtype, flags, ta, tb, splitk, mode, "padded" if padded else "exact"))
    finally:
        ck(lib, lib.cmp_gemm_set_workspace(None, 0))


@pytest.mark.parametrize("tb", [0, 1])
@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_gemm_column_sums_guarded(lib, family, tb):
    """cmp_gemm_colsum_next on the plain and act=2 epilogues at one ragged (136 x 136) and one full-tile (256 x 256) shape, K = 64
    (fast for every family): the vector is flush against its guards, starts non-zero, and ends within the column-sum bound (S = |start| +
    sum of |stored values|, K = rows + 1) of the float64 sums of the values the launch STORED."""
    dtype, flags = family
    for (M, N) in ((136, 136), (256, 256)):
        K = 64
        o = logical_ops(dtype, M, N, K)
        for padded in (True, False):
            for epi in ("none", "gelugrad"):
                ar = Arena("cuda", 2 << 20)
                A, B = stage_ab(ar, dtype, 0, tb, M, N, K, 0, 8 if padded else 0, 16 if padded else 0, o)
                Cs = ar.output(tdt(dtype), M, N, N + (16 if padded else 0), name="C")
                aux = ar.operand(o["pre"], tdt(dtype), M, N, N + (8 if padded else 0), name="aux") if epi == "gelugrad" else None
                start = o["bias"]
                vec = ar.vector(start, F32, name="colsum", kind="acc")
                ar.arm()
                ck(lib, lib.cmp_gemm_colsum_next(P(vec)))
                launch_gemm(lib, dtype, 0, tb, M, N, K, A, B, Cs, aux=aux, act=2 if aux is not None else 0, flags=flags)
                ar.check()
                what = "colsum dtype=%d flags=%d tb=%d M=%d N=%d %s %s" % (dtype, flags, tb, M, N, epi, "padded" if padded else "exact")
                gg = torch.from_numpy(O.gelu_grad(o["pre"].numpy())) if aux is not None else None
                allow = KA.f32_eval_allowance(O.gelu_grad, o["pre"].numpy()) if aux is not None else 0.0
                KA.assert_within(Cs.host(), o["ref"] * gg if aux is not None else o["ref"], o["f"] * o["S"] * (gg.abs() if aux is not None else 1.0),
                                 dtype == BF16, what, extra=o["ref"].abs() * allow)
                cref, cS, cf = KA.colsum_bound(Cs.host().double(), start)
                KA.assert_within(vec.host().reshape(-1), cref, cf * cS, False, what + " sums")


# ------------------------------------------------------------------------------------------ grouped weight gradients
@pytest.mark.parametrize("padded", [True, False])
@pytest.mark.parametrize("K", [32, 96])
def test_wgrad_group_guarded(lib, K, padded):
    """cmp_k_wgrad_group on the ragged problem list: C_i (fp32, non-zero start) += A_i^T . B_i, padded lda / ldb / ldc, per element
    within the fp32 accumulation bound (S = |C_i| + |A_i|^T . |B_i|).  A_i's and B_i's padding columns (m >= M, n >= N) are NaN."""
    shapes = [(264, 520), (8, 8), (1000, 136)]
    g = torch.Generator().manual_seed(K)
    ar = Arena("cuda", 6 << 20)
    As, Bs, Cs, refs = [], [], [], []
    for i, (m, n) in enumerate(shapes):
        a, b = rounded(torch.randn(K, m, generator=g), BF16), rounded(torch.randn(K, n, generator=g), BF16)
        c0 = torch.randn(m, n, generator=g).double()
        As.append(ar.operand(a, BF, K, m, m + (8 if padded else 0), name="A%d" % i))
        Bs.append(ar.operand(b, BF, K, n, n + (16 if padded else 0), name="B%d" % i))
        Cs.append(ar.accumulator(c0, F32, m, n, n + (8 if padded else 0), name="C%d" % i))
        ref, S, f = KA.gemm_bound(a.t().contiguous(), b, c0.abs())
        refs.append((ref + c0, S, f))
    nn = len(shapes)
    vp, ip = C.c_void_p * nn, C.c_int * nn
    ar.arm()
    ck(lib, lib.cmp_k_wgrad_group(stream(), nn, vp(*[s.ptr() for s in As]), ip(*[s.ld for s in As]), vp(*[s.ptr() for s in Bs]),
                                  ip(*[s.ld for s in Bs]), vp(*[s.ptr() for s in Cs]), ip(*[s.ld for s in Cs]),
                                  ip(*[m for m, n in shapes]), ip(*[n for m, n in shapes]), K))
    ar.check()
    for i, (c, (ref, S, f)) in enumerate(zip(Cs, refs)):
        KA.assert_within(c.host(), ref, f * S, False, "wgrad_group K=%d problem %d %s" % (K, i, shapes[i]))


# ------------------------------------------------------------------------------------------ attention
# (module-level: tests/test_attn_plan_host.py holds the rows to the launcher's plan on the CPU)
ATTN_GUARDED_P = [0.0, 0.2]
ATTN_GUARDED_CASES = ([(dt, *s) for s in ((2, 33, 4, 16), (1, 130, 1, 128), (1, 333, 2, 64)) for dt in (FP32, BF16)]
                      + [(BF16, 1, 96, 2, 16)])          # the last one runs the key-split kernels


@pytest.mark.parametrize("p", ATTN_GUARDED_P)
@pytest.mark.parametrize("dtype,B,T,H,D", ATTN_GUARDED_CASES)
def test_attention_guarded(lib, dtype, B, T, H, D, p):
    """cmp_k_attn_fwd / cmp_k_attn_bwd (bias gradient armed) with qkv and dO as arena inputs and o, lse, delta, dqkv as arena
    outputs at ragged T; the values against float64 with the tolerances of test_gpu_kernels.test_attention_fwd_bwd."""
    E = H * D
    dt = tdt(dtype)
    g = torch.Generator().manual_seed(B * 1000 + T + D)
    ar = Arena("cuda", 4 << 20)
    qkv = ar.operand(torch.randn(B * T, 3 * E, generator=g), dt, B * T, 3 * E, 3 * E, name="qkv")
    do = ar.operand(torch.randn(B * T, E, generator=g), dt, B * T, E, E, name="dO")
    o = ar.output(dt, B * T, E, E, name="o")
    lse = ar.output(F32, 1, B * H * T, B * H * T, name="lse")
    ar.arm()
    ck(lib, lib.cmp_k_attn_fwd(stream(), P(qkv), P(o), P(lse), B, T, H, D, 1, dtype, p, 1234, 21))
    ar.check()
    keep = O.dropout_keep_attn(1234, 21, B * H, T, p) if p > 0 else None
    x, oref, lseref = TK.attn_ref(qkv.host(), B, T, H, D, keep, p)
    tol = TK.TOL[dtype] * (3 if dtype == BF16 else 1)
    assert TK.rel_err(o.host(), oref.detach().reshape(B * T, E)) < tol
    assert TK.rel_err(lse.host().reshape(-1), lseref.detach().reshape(-1)) < (1e-5 if dtype == FP32 else 2e-2)
    oref.backward(do.host().double().reshape(B, T, E))
    # backward: o and lse become inputs of the second launch (the same arena, a second window each would hide nothing new)
    ar.freeze(o, lse)
    dqkv = ar.output(dt, B * T, 3 * E, 3 * E, name="dqkv")
    delta = ar.output(F32, 1, B * H * T, B * H * T, name="delta")
    bias_grad = ar.vector(torch.full((3 * E,), 2.0), F32, name="bias_grad", kind="acc")
    ar.arm()
    ck(lib, lib.cmp_attn_bwd_bias_next(P(bias_grad)))
    ck(lib, lib.cmp_k_attn_bwd(stream(), P(qkv), P(o), P(do), P(lse), P(delta), P(dqkv), B, T, H, D, 1, dtype, p, 1234, 21))
    ar.check()
    ref = x.grad.reshape(B * T, 3 * E)
    assert TK.rel_err(bias_grad.host().reshape(-1), ref.sum(0) + 2.0) < tol
    want_delta = (do.host().double() * o.host().double()).reshape(B, T, H, D).sum(-1).permute(0, 2, 1).reshape(-1)
    assert TK.rel_err(delta.host().reshape(-1), want_delta) < tol
    whole = ref.abs().max().item()
    got = dqkv.host().double()
    for name, sl in (("dq", slice(0, E)), ("dk", slice(E, 2 * E)), ("dv", slice(2 * E, 3 * E))):
        err = (got[:, sl] - ref[:, sl]).abs().max().item()
        assert err / max(ref[:, sl].abs().max().item(), 0.1 * whole, 1e-30) < tol * 2, name


# ------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("rows,E", [(37, 64), (66, 256), (37, 768)])
def test_layernorm_guarded(lib, dtype, rows, E):
    """cmp_k_layernorm_fwd / _bwd / _bwd_fused in the arena (the workspace exactly cmp_k_layernorm_bwd_ws bytes, flush against a
    guard), the tolerances of test_gpu_kernels.test_layernorm_fwd_bwd, and the same tolerances row by row: each row's error over
    that row's own largest reference value."""
    dt = tdt(dtype)
    g = torch.Generator().manual_seed(rows + E)
    ar = Arena("cuda", 8 << 20)
    mat = lambda t, name: ar.operand(t, dt, rows, E, E, name=name)
    x = mat(torch.randn(rows, E, generator=g) * 2 + 0.5, "x")
    gamma, beta = ar.vector(torch.randn(E, generator=g), F32, name="gamma"), ar.vector(torch.randn(E, generator=g), F32, name="beta")
    y = ar.output(dt, rows, E, E, name="y")
    mean, rstd = ar.output(F32, 1, rows, rows, name="mean"), ar.output(F32, 1, rows, rows, name="rstd")
    ar.arm()
    ck(lib, lib.cmp_k_layernorm_fwd(stream(), P(x), P(gamma), P(beta), P(y), P(mean), P(rstd), rows, E, 1e-5, dtype))
    ar.check()
    x64, g64 = x.host().double().numpy(), gamma.host().double().numpy().reshape(-1)
    yr, cache = O.layernorm_fwd(x64, g64, beta.host().double().numpy().reshape(-1), 1e-5)
    tol = TK.TOL[dtype]
    assert TK.rel_err(y.host(), torch.tensor(yr)) < tol and KA.rowwise_rel_err(y.host(), torch.tensor(yr)) < tol
    assert TK.rel_err(rstd.host().reshape(-1), torch.tensor(cache[1][:, 0])) < 1e-5
    assert TK.rel_err(mean.host().reshape(-1), torch.tensor(x64.mean(-1))) < 1e-5
    ar.freeze(y, mean, rstd)
    dy = mat(torch.randn(rows, E, generator=g), "dy")
    resid = mat(torch.randn(rows, E, generator=g), "resid")
    dx = ar.output(dt, rows, E, E, name="dx")
    dg = ar.vector(torch.full((E,), 1.0), F32, name="dgamma", kind="acc")
    db = ar.vector(torch.full((E,), -1.0), F32, name="dbeta", kind="acc")
    ws = ar.scratch(int(lib.cmp_k_layernorm_bwd_ws(rows, E)), name="ws")
    ar.arm()
    ck(lib, lib.cmp_k_layernorm_bwd(stream(), P(dy), P(x), P(gamma), P(mean), P(rstd), P(resid), P(dx), P(dg), P(db), P(ws), rows, E, dtype))
    ar.check()
    dxr, dgr, dbr = O.layernorm_bwd(dy.host().double().numpy(), cache, g64)
    want_dx = torch.tensor(dxr) + resid.host().double()
    assert TK.rel_err(dx.host(), want_dx) < tol and KA.rowwise_rel_err(dx.host(), want_dx) < tol
    vtol = 3e-5 * math.sqrt(rows) + (0 if dtype == FP32 else 1e-3)
    assert TK.rel_err(dg.host().reshape(-1), torch.tensor(dgr) + 1.0) < vtol
    assert TK.rel_err(db.host().reshape(-1), torch.tensor(dbr) - 1.0) < vtol
    # fused consumer prologue
    ar.freeze(dx)
    dx2, dmask = ar.output(dt, rows, E, E, name="dx2"), ar.output(dt, rows, E, E, name="dmask")
    dg2 = ar.vector(torch.zeros(E), F32, name="dgamma2", kind="acc")
    db2 = ar.vector(torch.zeros(E), F32, name="dbeta2", kind="acc")
    cs = ar.vector(torch.full((E,), 2.0), F32, name="colsum", kind="acc")
    ar.arm()
    ck(lib, lib.cmp_k_layernorm_bwd_fused(stream(), P(dy), P(x), P(gamma), P(mean), P(rstd), P(resid), P(dx2), P(dg2), P(db2), P(ws),
                                          rows, E, dtype, P(dmask), P(cs), 0.25, 41, 6))
    ar.check()
    assert torch.equal(dx2.host(), dx.host())
    want = dx.host().double() * torch.tensor(O.dropout_keep_rows(41, 6, rows, E, 0.25) / 0.75)
    assert TK.rel_err(dmask.host(), want) < tol and KA.rowwise_rel_err(dmask.host(), want) < tol
    assert TK.rel_err(cs.host().reshape(-1), dmask.host().double().sum(0) + 2.0) < 3e-5 * math.sqrt(rows) + (0 if dtype == FP32 else 2e-3)


# ------------------------------------------------------------------------------------------ softmax cross-entropy
@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("V,ldz", [(390, 448), (512, 512), (513, 576)])
def test_softmax_xent_guarded(lib, dtype, V, ldz):
    """cmp_k_softmax_xent at 37 rows: NaN logit padding, labels 0 and V - 1, dlogits padding must come back ZERO (the header's
    "zeroed padding"), row_loss / row_correct fully written; both kernels (ldz <= 512 register-resident, wider three-pass)."""
    rows = 37
    g = torch.Generator().manual_seed(3)
    z = torch.randn(rows, V, generator=g) * 3
    z[5, 10] = z[5, 20] = 50.0
    yy = torch.randint(0, V, (rows,), generator=g, dtype=I32)
    yy[0], yy[1], yy[5], yy[rows - 1] = 0, V - 1, 10, V - 1
    ar = Arena("cuda", 1 << 20)
    zs = ar.operand(z, F32, rows, V, ldz, name="logits")
    ys = ar.operand(yy, I32, 1, rows, rows, name="labels")
    dz = ar.output(tdt(dtype), rows, V, ldz, name="dlogits", pad_zero=True)
    rl, rc = ar.output(F32, 1, rows, rows, name="row_loss"), ar.output(I32, 1, rows, rows, name="row_correct")
    ar.arm()
    ck(lib, lib.cmp_k_softmax_xent(stream(), P(zs), ldz, P(ys), P(dz), P(rl), P(rc), rows, V, 1.0 / rows, dtype))
    ar.check()
    zz = z.double()
    nll = torch.logsumexp(zz, -1) - zz[torch.arange(rows), yy.long()]
    assert TK.rel_err(rl.host().reshape(-1), nll) < 1e-5
    pred = zz.argmax(-1); pred[5] = 10
    assert torch.equal(rc.host().reshape(-1).long(), (pred == yy.long()).long())
    sm = torch.softmax(zz, -1); sm[torch.arange(rows), yy.long()] -= 1; sm /= rows
    tol = 1e-5 if dtype == FP32 else 1e-2
    assert TK.rel_err(dz.host(), sm) < tol and KA.rowwise_rel_err(dz.host(), sm) < tol


# ------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("B,T,E,V", [(3, 17, 64, 390), (33, 128, 64, 3)])
def test_embedding_guarded(lib, dtype, B, T, E, V):
    """cmp_k_embed_fwd / _bwd / _bwd_v with ids that hit 0 and V - 1 and pos0 > 0 with W = pos0 + T exactly: the last position row
    is flush against the guard, rows below pos0 of the position gradient stay untouched."""
    dt, pos0, p = tdt(dtype), 3, 0.3
    W = pos0 + T
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, V, (B, T), generator=g, dtype=I32)
    ids[0, 0], ids[B - 1, T - 1] = 0, V - 1
    wte, wpe = torch.randn(V, E, generator=g), torch.randn(W, E, generator=g)
    ar = Arena("cuda", 8 << 20)
    ids_s = ar.operand(ids, I32, 1, B * T, B * T, name="ids")
    wte_s, wpe_s = ar.operand(wte, F32, V, E, E, name="wte"), ar.operand(wpe, F32, W, E, E, name="wpe")
    out = ar.output(dt, B * T, E, E, name="out")
    ar.arm()
    ck(lib, lib.cmp_k_embed_fwd(stream(), P(ids_s), P(wte_s), P(wpe_s), P(out), B, T, E, pos0, dtype, p, 5, 2))
    ar.check()
    keep = torch.tensor(O.dropout_keep_rows(5, 2, B * T, E, p) / (1 - p))
    ref = (wte[ids.long()] + wpe[pos0:pos0 + T][None]).reshape(B * T, E).double() * keep
    assert TK.rel_err(out.host(), ref) < (1e-6 if dtype == FP32 else 1e-2)
    ar.freeze(out)
    dh = ar.operand(torch.randn(B * T, E, generator=g), dt, B * T, E, E, name="dh")
    d = dh.host().double() * keep
    dwte0, dwpe0 = torch.randn(V, E, generator=g), torch.randn(W, E, generator=g)
    rw = dwte0.double().clone(); rw.index_add_(0, ids.reshape(-1).long(), d)
    rp = dwpe0.double().clone(); rp[pos0:pos0 + T] += d.reshape(B, T, E).sum(0)
    # the form each launch takes (cmp_embed_bwd_form: 0 atomic, 1 sorted): cmp_k_embed_bwd_v brings a sort workspace, but below 4096
    # tokens -- the (3, 17, ...) case -- its launch is the atomic form a second time
    for entry, want in (("bwd", "atomic"), ("bwd_v", "sorted" if B * T >= 4096 else "atomic")):
        words = lib.cmp_embed_bwd_sort_ws_words(B * T, V) if entry == "bwd_v" else 0
        form = ("atomic", "sorted", "atomic-free")[lib.cmp_embed_bwd_form(B, T, E, dtype, V, words, 0)]
        assert form == want, (entry, form)
        dwte = ar.accumulator(dwte0, F32, V, E, E, name="dwte_%s_%s" % (entry, form))
        dwpe = ar.accumulator(dwpe0, F32, W, E, E, name="dwpe_%s_%s" % (entry, form))
        ar.arm()
        if entry == "bwd_v":
            ck(lib, lib.cmp_k_embed_bwd_v(stream(), P(ids_s), P(dh), P(dwte), P(dwpe), B, T, E, pos0, dtype, p, 5, 2, V))
        else:
            ck(lib, lib.cmp_k_embed_bwd(stream(), P(ids_s), P(dh), P(dwte), P(dwpe), B, T, E, pos0, dtype, p, 5, 2))
        ar.check()
        assert TK.rel_err(dwte.host(), rw) < 2e-5 and TK.rel_err(dwpe.host(), rp) < 2e-5, (entry, form)
        assert torch.equal(dwpe.host()[:pos0], dwpe0[:pos0])
        ar.freeze(dwte, dwpe)


# ------------------------------------------------------------------------------------------ Adam, clipping, column sums
def adam_ref(p0, gr, m0, v0, step, scale):
    g64 = gr.double() * scale
    m1 = 0.9 * m0.double() + 0.1 * g64
    v1 = 0.999 * v0.double() + 0.001 * g64 * g64
    alpha = 1e-3 * math.sqrt(1 - 0.999 ** step) / (1 - 0.9 ** step)
    return p0.double() - alpha * m1 / (v1.sqrt() + 1e-7), m1, v1


@pytest.mark.parametrize("dev_factor", [False, True])
@pytest.mark.parametrize("n", [4, 1028, 4100])
def test_adam_guarded(lib, n, dev_factor):
    """cmp_k_adam / cmp_k_adam_dev: all five arrays flush against guards, n a multiple of 4 but not of the block size."""
    g = torch.Generator().manual_seed(9 + n)
    p0, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    m0, v0 = torch.randn(n, generator=g) * 0.01, torch.rand(n, generator=g) * 0.01
    ar = Arena("cuda", 1 << 20)
    p, m, v = (ar.vector(t, F32, name=nm, kind="acc") for t, nm in ((p0, "p"), (m0, "m"), (v0, "v")))
    gd = ar.vector(gr, F32, name="g")
    sh = ar.output(BF, 1, n, n, name="shadow")
    fac = ar.vector(torch.tensor([0.5]), F32, name="factor")
    ar.arm()
    if dev_factor:
        ck(lib, lib.cmp_k_adam_dev(stream(), P(p), P(gd), P(m), P(v), P(sh), n, 1e-3, 0.9, 0.999, 1e-7, 7, P(fac)))
    else:
        ck(lib, lib.cmp_k_adam(stream(), P(p), P(gd), P(m), P(v), P(sh), n, 1e-3, 0.9, 0.999, 1e-7, 7, 0.5))
    ar.check()
    p1, m1, v1 = adam_ref(p0, gr, m0, v0, 7, 0.5)
    assert TK.rel_err(m.host(), m1[None]) < 1e-6 and TK.rel_err(v.host(), v1[None]) < 1e-6 and TK.rel_err(p.host(), p1[None]) < 1e-6
    assert torch.equal(sh.host(), p.host().to(BF))


def test_adam_and_clip_refuse_n_not_a_multiple_of_4(lib):
    """n % 4 != 0 is an error of all three entry points, and nothing is written -- not one byte of the arena changes."""
    n = 1030
    ar = Arena("cuda", 1 << 20)
    t = torch.randn(n)
    p, gd, m, v = (ar.vector(t, F32, name=nm, kind="acc") for nm in "pgmv")
    sh = ar.accumulator(t, BF, 1, n, n, name="shadow")
    fac = ar.vector(torch.tensor([0.5]), F32, name="factor")
    ws, out = ar.scratch(int(lib.cmp_k_grad_clip_ws(n)), name="ws"), ar.scratch(16, name="clip out")
    ar.arm()
    before = ar.snap.copy()
    assert lib.cmp_k_adam(stream(), P(p), P(gd), P(m), P(v), P(sh), n, 1e-3, 0.9, 0.999, 1e-7, 7, 0.5) < 0
    assert b"multiple of 4" in lib.cmp_last_error()
    assert lib.cmp_k_adam_dev(stream(), P(p), P(gd), P(m), P(v), P(sh), n, 1e-3, 0.9, 0.999, 1e-7, 7, P(fac)) < 0
    assert b"multiple of 4" in lib.cmp_last_error()
    assert lib.cmp_k_grad_clip(stream(), P(gd), n, 1.0, 1.0, P(ws), P(out)) < 0
    assert b"multiple of 4" in lib.cmp_last_error()
    ar.check()
    assert np.array_equal(ar.buf.cpu().numpy(), before)


@pytest.mark.parametrize("n", [4, 1028, 4100])
def test_grad_clip_guarded(lib, n):
    """cmp_k_grad_clip: the gradient, the workspace (exactly cmp_k_grad_clip_ws bytes) and the 16-byte result flush against guards;
    norm against float64, scale and factor as the header defines them."""
    g = torch.Generator().manual_seed(n)
    gr = torch.randn(n, generator=g)
    ar = Arena("cuda", 1 << 20)
    gd = ar.vector(gr, F32, name="g")
    ws, out = ar.scratch(int(lib.cmp_k_grad_clip_ws(n)), name="ws"), ar.scratch(16, name="out")
    gscale, clip = 0.25, 0.5
    ar.arm()
    ck(lib, lib.cmp_k_grad_clip(stream(), P(gd), n, gscale, clip, P(ws), P(out)))
    ar.check()
    raw = out.t.cpu().numpy().tobytes()
    norm, scale, factor = np.frombuffer(raw[:8], np.float64)[0], np.frombuffer(raw[8:12], np.float32)[0], np.frombuffer(raw[12:16], np.float32)[0]
    want = gscale * math.sqrt(float((gr.double() ** 2).sum()))
    assert abs(norm - want) <= 1e-13 * want
    want_scale = 1.0 if want <= clip else clip / want
    assert abs(scale - want_scale) <= 2e-7 * want_scale and abs(factor - gscale * want_scale) <= 3e-7 * gscale * want_scale


@pytest.mark.parametrize("dtype", [FP32, BF16])
def test_colsum_guarded(lib, dtype):
    """cmp_k_colsum at (rows, cols, ldx) = (37, 392, 408): NaN row padding, a non-zero start, the column-sum bound per element."""
    rows, cols, ldx = 37, 392, 408
    g = torch.Generator().manual_seed(7)
    xv = rounded(torch.randn(rows, cols, generator=g), dtype)
    start = torch.randn(cols, generator=g).double()
    ar = Arena("cuda", 1 << 20)
    x = ar.operand(xv, tdt(dtype), rows, cols, ldx, name="x")
    out = ar.vector(start, F32, name="out", kind="acc")
    ar.arm()
    ck(lib, lib.cmp_k_colsum(stream(), P(x), ldx, P(out), rows, cols, dtype))
    ar.check()
    ref, S, f = KA.colsum_bound(xv, start)
    KA.assert_within(out.host().reshape(-1), ref, f * S, False, "colsum dtype=%d" % dtype)
