"""-m gpu: cmp_k_wgrad_group_bias -- the grouped weight-gradient launch with the bias gradients riding on it -- in the pattern of
test_gpu_kernel_guards.test_wgrad_group_guarded: guard-banded arena, padded strides, NaN padding columns, per-element fp32
accumulation bounds.  bias_i (non-zero start) += column sums of B_i as stored; one problem has no bias among two that have one.

The shapes have two (264 rows) and four (1000 rows) tile rows: a sum added once per tile row instead of once is 2x / 4x off; the
ragged N (520, 8, 136) meets the column guard.  The depths: one k-step, three, and one at which the launcher's plan
(cmp_wgrad_group_plan) cuts tiles into several K ranges -- asserted, not assumed."""
import ctypes as C

import numpy as np
import pytest
import torch

import kernel_arena as KA
from kernel_arena import Arena
from test_gpu_kernel_guards import BF, BF16, F32, ck, lib, rounded, stream  # noqa: F401  (lib: the module's fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(264, 520), (8, 8), (1000, 136)]
NO_BIAS = 1                    # the problem without a bias vector
K_SPLIT = 256                  # the plan cuts these tiles into several K ranges here (asserted below)


def plan_ranges(lib, K):
    """Most K ranges of a tile in the plan of SHAPES at depth K (forced, as the entry point does)."""
    from composer_amd import _lib
    n = len(SHAPES)
    ip = C.c_int * n
    info = _lib.WgradPlanInfo()
    rows = np.zeros((1024, 8), np.int32)
    ck(lib, lib.cmp_wgrad_group_plan(n, None, ip(*[m for m, _ in SHAPES]), None, ip(*[nn for _, nn in SHAPES]), ip(*[m for m, _ in SHAPES]),
                                     ip(*[nn for _, nn in SHAPES]), K, 0, 2, C.byref(info), rows.ctypes.data_as(C.c_void_p), 1024))
    assert info.fits and info.taken and info.nitems <= 1024
    return int(rows[:info.nitems, 6].max())


@pytest.mark.parametrize("padded", [True, False])
@pytest.mark.parametrize("K", [32, 96, K_SPLIT])
def test_wgrad_group_bias_guarded(lib, K, padded):
    if K == K_SPLIT:
        assert plan_ranges(lib, K) >= 2
    if K == 32:
        assert plan_ranges(lib, K) == 1
    g = torch.Generator().manual_seed(K + 7)
    ar = Arena("cuda", 6 << 20)
    As, Bs, Cs, bs, refs, brefs, ref0 = [], [], [], [], [], [], []
    for i, (m, n) in enumerate(SHAPES):
        a, b = rounded(torch.randn(K, m, generator=g), BF16), rounded(torch.randn(K, n, generator=g), BF16)
        c0 = torch.randn(m, n, generator=g).double()
        b0 = torch.randn(n, generator=g).double() * 3.0 + 1.0
        As.append(ar.operand(a, BF, K, m, m + (8 if padded else 0), name="A%d" % i))
        Bs.append(ar.operand(b, BF, K, n, n + (16 if padded else 0), name="B%d" % i))
        Cs.append(ar.accumulator(c0, F32, m, n, n + (8 if padded else 0), name="C%d" % i))
        bs.append(ar.vector(b0.float(), F32, name="bias%d" % i, kind="acc"))
        ref, S, f = KA.gemm_bound(a.t().contiguous(), b, c0.abs())
        refs.append((ref + c0, S, f))
        ref0.append(b0.float().double())
        brefs.append(KA.colsum_bound(b, b0.float().double()))        # B_i as stored (bf16), onto the start value
    nn = len(SHAPES)
    vp, ip = C.c_void_p * nn, C.c_int * nn
    args = (vp(*[s.ptr() for s in As]), ip(*[s.ld for s in As]), vp(*[s.ptr() for s in Bs]), ip(*[s.ld for s in Bs]),
            vp(*[s.ptr() for s in Cs]), ip(*[s.ld for s in Cs]), ip(*[m for m, n in SHAPES]), ip(*[n for m, n in SHAPES]), K)
    ar.arm()
    ck(lib, lib.cmp_k_wgrad_group_bias(stream(), nn, *args, vp(*[None if i == NO_BIAS else s.ptr() for i, s in enumerate(bs)])))
    ar.check()
    for i, (c, (ref, S, f)) in enumerate(zip(Cs, refs)):
        KA.assert_within(c.host(), ref, f * S, False, "wgrad_group_bias K=%d C of problem %d %s" % (K, i, SHAPES[i]))
    for i, (v, (ref, S, f)) in enumerate(zip(bs, brefs)):
        if i == NO_BIAS:
            assert torch.equal(v.host().reshape(-1).double(), ref0[i]), "the vector of the problem without a bias was written"
            continue
        KA.assert_within(v.host().reshape(-1), ref, f * S, False, "wgrad_group_bias K=%d bias of problem %d %s" % (K, i, SHAPES[i]))
    # a second launch with every bias null: the vectors (the skipped one included) are inputs now -- bitwise unchanged
    ar.freeze(*bs)
    ar.arm()
    ck(lib, lib.cmp_k_wgrad_group_bias(stream(), nn, *args, vp(*[None] * nn)))
    ar.check()
    ar.arm()
    ck(lib, lib.cmp_k_wgrad_group_bias(stream(), nn, *args, None))
    ar.check()
