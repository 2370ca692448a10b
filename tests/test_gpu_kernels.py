"""-m gpu: kernel-level parity of the HIP kernels, called through the C ABI (cmp_k_*) with device memory
borrowed from torch tensors.  References are float64 torch/numpy restatements of the same op (the oracle's
formulas); the dropout tests use the oracle's counter hash so masks are bit-identical.

Tolerances: fp32 mode ~1e-5 relative (f32 MFMA = exact fma chains, only summation order differs);
bf16 mode: inputs are rounded to bf16 first, then the comparison allows the bf16 output rounding (2^-8 relative).
"""
import ctypes as C
import math
import os
import numpy as np
import pytest
import torch

from oracle import transformer_oracle as O

pytestmark = pytest.mark.gpu

FP32, BF16 = 0, 1


@pytest.fixture(scope="module")
def lib():
    from composer_amd import _lib
    l = _lib.load()
    _lib.require_gpu()
    return l


def ck(lib, rc):
    assert rc == 0, lib.cmp_last_error().decode()


def tdt(dtype):
    return torch.bfloat16 if dtype == BF16 else torch.float32


def dev(a, dtype=None):
    t = torch.as_tensor(a).cuda()
    if dtype is not None:
        t = t.to(tdt(dtype))
    return t.contiguous()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rel_err(a, b):
    a = a.double().cpu(); b = b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


TOL = {FP32: 2e-5, BF16: 1.2e-2}


# ------------------------------------------------------------------------------------------ GEMM
def gemm(lib, dtype, ta, tb, A, B, M, N, K, bias=None, act=0, aux=None, resid=None, out_fp32=False, splitk=1,
         p_drop=0.0, seed=0, rng=0, C0=None, ldc=None, flags=0):
    ldc = ldc or N
    if C0 is not None:
        Cm = C0
    else:
        Cm = torch.zeros(M, ldc, device="cuda", dtype=torch.float32 if out_fp32 else tdt(dtype))
    lda, ldb = A.shape[1], B.shape[1]
    ck(lib, lib.cmp_k_gemm(stream(), dtype, ta, tb, M, N, K, P(A), lda, P(B), ldb, P(Cm), ldc, P(bias), act, P(aux),
                           aux.shape[1] if aux is not None else 0, P(resid), resid.shape[1] if resid is not None else 0,
                           int(out_fp32), splitk, p_drop, seed, rng, flags))
    torch.cuda.synchronize()
    return Cm


@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("flags", [0, 2, 4, 8, 16, 48])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (72, 392, 72), (200, 136, 392), (384, 640, 256), (1000, 264, 512), (2104, 520, 192)])
def test_gemm_layouts(lib, dtype, ta, tb, M, N, K, flags):
    """flags=0: automatic choice; 2: generic register-staged kernel; 4: 128x128 direct-to-LDS; 8: persistent 256x256."""
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + ta * 2 + tb)
    a = torch.randn(M, K, generator=g)
    b = torch.randn(K, N, generator=g)
    A = dev(a.t().contiguous() if ta else a, dtype)
    B = dev(b.t().contiguous() if tb else b, dtype)
    ref = (A.double().t() if ta else A.double()) @ (B.double().t() if tb else B.double())
    out = gemm(lib, dtype, ta, tb, A, B, M, N, K, flags=flags)
    assert rel_err(out, ref) < TOL[dtype]


def wgrad_group(lib, As, Bs, Cs, K):
    n = len(As)
    vp, ip = C.c_void_p * n, C.c_int * n
    ck(lib, lib.cmp_k_wgrad_group(stream(), n, vp(*[a.data_ptr() for a in As]), ip(*[a.shape[1] for a in As]),
                                  vp(*[b.data_ptr() for b in Bs]), ip(*[b.shape[1] for b in Bs]), vp(*[c.data_ptr() for c in Cs]),
                                  ip(*[c.shape[1] for c in Cs]), ip(*[a.shape[1] for a in As]), ip(*[b.shape[1] for b in Bs]), K))
    torch.cuda.synchronize()


@pytest.mark.parametrize("K", [32, 96, 2048, 8192 + 32])
@pytest.mark.parametrize("shapes", [[(512, 2048), (2048, 512), (512, 512), (512, 1536)],           # a C2 decoder block
                                    [(768, 3072), (3072, 768), (768, 768), (768, 2304)],           # a C4 decoder block
                                    [(64, 64)], [(264, 520), (8, 8), (1000, 136)],                 # ragged tiles, one problem, tiny problems
                                    [(256, 256)] * 8])
def test_grouped_weight_gradients(lib, K, shapes):
    """cmp_k_wgrad_group: C_i += A_i^T . B_i for all problems in ONE launch (all output tiles cut into the same K ranges, f32 atomics)
    against float64 products; C_i starts non-zero (accumulate semantics) and the bytes next to every C_i stay untouched."""
    g = torch.Generator().manual_seed(K + len(shapes))
    As = [torch.randn(K, m, generator=g).to(torch.bfloat16).cuda() for m, n in shapes]
    Bs = [torch.randn(K, n, generator=g).to(torch.bfloat16).cuda() for m, n in shapes]
    C0 = [torch.randn(m + 1, n, generator=g) for m, n in shapes]                  # one guard row behind each C_i
    Cs = [c.clone().cuda() for c in C0]
    wgrad_group(lib, As, Bs, [c[:-1] for c in Cs], K)
    for a, b, c0, c in zip(As, Bs, C0, Cs):
        ref = c0[:-1].double() + a.double().cpu().T @ b.double().cpu()
        assert rel_err(c[:-1], ref) < 2e-5, (a.shape, b.shape)
        assert torch.equal(c[-1].cpu(), c0[-1])
    # the same call again adds the products once more (and reuses the cached item table)
    wgrad_group(lib, As, Bs, [c[:-1] for c in Cs], K)
    for a, b, c0, c in zip(As, Bs, C0, Cs):
        assert rel_err(c[:-1], c0[:-1].double() + 2 * (a.double().cpu().T @ b.double().cpu())) < 4e-5


def test_grouped_weight_gradients_with_item_counters(lib, monkeypatch):
    """The grouped launch with its items claimed from the per-XCD counters (what a data-parallel job uses: COMPOSER_GEMM_ITEMS=dynamic
    forces it here) gives the products of the statically strided launch; repeated launches alternate the two counter sets."""
    K, shapes = 4096, [(512, 2048), (2048, 512), (512, 512), (512, 1536)]
    g = torch.Generator().manual_seed(3)
    As = [torch.randn(K, m, generator=g).to(torch.bfloat16).cuda() for m, n in shapes]
    Bs = [torch.randn(K, n, generator=g).to(torch.bfloat16).cuda() for m, n in shapes]
    refs = [a.double().cpu().T @ b.double().cpu() for a, b in zip(As, Bs)]
    monkeypatch.setenv("COMPOSER_GEMM_ITEMS", "dynamic")
    for rep in range(5):
        Cs = [torch.zeros(m, n, device="cuda") for m, n in shapes]
        wgrad_group(lib, As, Bs, Cs, K)
        for c, ref in zip(Cs, refs):
            assert rel_err(c, ref) < 2e-5, rep


def test_grouped_weight_gradients_at_the_timed_depth(lib):
    """The C2 block at K = 131 072 tokens (bench.py's geometry): every problem against its float64 product."""
    K = 131072
    shapes = [(2048, 512), (512, 2048), (512, 512), (512, 1536)]
    g = torch.Generator().manual_seed(9)
    As = [torch.randn(K, m, generator=g).to(torch.bfloat16) for m, n in shapes]
    Bs = [torch.randn(K, n, generator=g).to(torch.bfloat16) for m, n in shapes]
    Cs = [torch.zeros(m, n, device="cuda") for m, n in shapes]
    wgrad_group(lib, [a.cuda() for a in As], [b.cuda() for b in Bs], Cs, K)
    for a, b, c in zip(As, Bs, Cs):
        ref = torch.from_numpy(a.double().numpy().T @ b.double().numpy())
        assert rel_err(c, ref) < 5e-5, (a.shape, b.shape)


@pytest.mark.parametrize("K,shapes", [(65536, [(768, 3072), (3072, 768), (768, 768), (768, 2304)]),      # a C4 block at its timed depth
                                      (4096, [(512, 2048), (2048, 512), (512, 512), (512, 1536)]), (96, [(264, 520), (8, 8)])])
def test_grouped_weight_gradients_last_arriver_form_is_bitwise_reproducible(lib, K, shapes, monkeypatch):
    """Round 6: the grouped launch without float atomics (COMPOSER_WGRAD_TAIL=la here; what COMPOSER_DETERMINISTIC=1 trains with) -- partial
    tiles through workspace slots, summed by the LAST-ARRIVING workgroup of a tile in the order of the K ranges (gemm.hip: WgLa).  Two
    launches from the same start give the same bits, also with the items claimed dynamically (a data-parallel job), the per-tile
    tickets are back at zero for the next launch, and the values are the float64 products."""
    monkeypatch.setenv("COMPOSER_WGRAD_TAIL", "la")
    g = torch.Generator().manual_seed(K)
    As = [torch.randn(K, m, generator=g).to(torch.bfloat16).cuda() for m, n in shapes]
    Bs = [torch.randn(K, n, generator=g).to(torch.bfloat16).cuda() for m, n in shapes]
    C0 = [torch.randn(m, n, generator=g) for m, n in shapes]
    outs = []
    for items in ("static", "dynamic", "static"):
        monkeypatch.setenv("COMPOSER_GEMM_ITEMS", items)
        Cs = [c.clone().cuda() for c in C0]
        wgrad_group(lib, As, Bs, Cs, K)
        outs.append([c.cpu() for c in Cs])
    for a, b, c in zip(*outs):
        assert torch.equal(a, b) and torch.equal(a, c)
    for a, b, c0, c in zip(As, Bs, C0, outs[0]):
        ref = c0.double() + torch.from_numpy(a.float().cpu().double().numpy().T @ b.float().cpu().double().numpy())
        assert rel_err(c, ref) < 5e-5, (a.shape, b.shape)


def test_gemm_bf16_ragged_k_zero_padded(lib):
    """dH = dZ.wte: K = V = 390 with dZ rows zero-padded to 448 (CMP_GEMM_KPAD_ZERO) takes the fast path.  The operands live in a
    guard-banded arena (tests/kernel_arena.py): the memory right after B IS a band of NaN bytes, so a load past B's last row
    that reached the product would show in every output element; range-checked loads keep it out."""
    from kernel_arena import Arena
    M, N, K, ld = 300, 128, 390, 448
    g = torch.Generator().manual_seed(1)
    a = torch.zeros(M, ld); a[:, :K] = torch.randn(M, K, generator=g)
    b = torch.randn(K, N, generator=g)
    for flags in (1, 2):
        ar = Arena("cuda", 2 << 20)
        A = ar.operand(a, torch.bfloat16, M, ld, ld, name="A")            # columns 390..448 are the contract's zeros
        B = ar.operand(b, torch.bfloat16, K, N, N, name="B")              # flush against its guard
        Cm = ar.output(torch.bfloat16, M, N, N, name="C")
        ar.arm()
        ck(lib, lib.cmp_k_gemm(stream(), BF16, 0, 0, M, N, K, P(A.t), ld, P(B.t), N, P(Cm.t), N, None, 0, None, 0, None, 0, 0, 1, 0.0, 0, 0, flags))
        ar.check()
        ref = A.host().double()[:, :K] @ B.host().double()
        assert rel_err(Cm.host(), ref) < TOL[BF16]


@pytest.mark.parametrize("dtype", [FP32, BF16])
def test_gemm_identity_asymmetric(lib, dtype):
    """A = I with an ASYMMETRIC B catches swapped row/col maps in the MFMA C-layout."""
    n = 128
    b = torch.arange(n * n, dtype=torch.float32).reshape(n, n) % 251 - 100
    A = dev(torch.eye(n), dtype)
    B = dev(b, dtype)
    for ta, tb in [(0, 0), (1, 0)]:
        out = gemm(lib, dtype, ta, tb, A, B, n, n, n)
        assert torch.equal(out.float().cpu(), B.float().cpu())
    out = gemm(lib, dtype, 0, 1, A, B, n, n, n)
    assert torch.equal(out.float().cpu(), B.float().cpu().t())


@pytest.mark.parametrize("dtype,flags", [(FP32, 0), (BF16, 0), (BF16, 4), (BF16, 8), (BF16, 16), (BF16, 48)])
def test_gemm_epilogues(lib, dtype, flags):
    M, N, K = 136, 264, 128
    _gemm = globals()["gemm"]
    def gemm(*a, **k):          # every call of this test uses the selected kernel
        k.setdefault("flags", flags)
        return _gemm(*a, **k)
    g = torch.Generator().manual_seed(5)
    A, B = dev(torch.randn(M, K, generator=g), dtype), dev(torch.randn(K, N, generator=g) * 0.2, dtype)
    bias = dev(torch.randn(N, generator=g))
    resid = dev(torch.randn(M, N, generator=g), dtype)
    acc = A.double() @ B.double() + bias.double()
    # bias + gelu, pre-activation to aux
    aux = torch.zeros(M, N, device="cuda", dtype=tdt(dtype))
    out = gemm(lib, dtype, 0, 0, A, B, M, N, K, bias=bias, act=1, aux=aux)
    assert rel_err(aux, acc) < TOL[dtype]
    assert rel_err(out, torch.tensor(O.gelu(acc.cpu().numpy()))) < TOL[dtype]
    # bias + residual
    out = gemm(lib, dtype, 0, 0, A, B, M, N, K, bias=bias, resid=resid)
    assert rel_err(out, acc + resid.double()) < TOL[dtype]
    # multiply by gelu'(aux)
    pre = dev(torch.randn(M, N, generator=g), dtype)
    out = gemm(lib, dtype, 0, 0, A, B, M, N, K, act=2, aux=pre)
    ref = (A.double() @ B.double()).cpu() * torch.tensor(O.gelu_grad(pre.double().cpu().numpy()))
    assert rel_err(out, ref) < TOL[dtype]
    # fp32 output + split-K accumulation on top of existing contents
    C0 = torch.ones(M, N, device="cuda", dtype=torch.float32)
    out = gemm(lib, dtype, 0, 0, A, B, M, N, K, out_fp32=True, splitk=2, C0=C0)
    assert rel_err(out, A.double() @ B.double() + 1.0) < TOL[dtype]
    # dropout in the epilogue uses the oracle's mask
    out = gemm(lib, dtype, 0, 0, A, B, M, N, K, bias=bias, resid=resid, p_drop=0.25, seed=77, rng=9)
    keep = O.dropout_keep_rows(77, 9, M, N, 0.25)
    ref = acc.cpu() * torch.tensor(keep / 0.75) + resid.double().cpu()
    assert rel_err(out, ref) < TOL[dtype]


@pytest.mark.parametrize("tb", [0, 1])
@pytest.mark.parametrize("M,N,K", [(512, 512, 256), (768, 1024, 96), (1024, 512, 512), (1024, 256, 1024), (1024, 256, 768),
                                   (256, 256, 128), (256, 384, 192), (384, 256, 320), (128, 128, 576)])
def test_gemm_epilogue_kinds_full_tiles(lib, tb, M, N, K):
    """Full 256x256 tiles with bf16 output take the compile-time epilogue kinds (gemm.hip EPI_*: operand loads two
    chunks ahead, counted waits) on the forward (tb=0, deep pipeline) and dgrad (tb=1, 2-stage 256) kernels.  Each kind
    must agree with the fp64 reference and, element by element, with the run-time epilogue of the 128x128 kernel (flags=4).
    Shapes of at most 256 128x128 tiles with whole 64-deep k-steps and both operands K-contiguous (tb=1: the default configuration's
    GEMMs at 1 024 tokens) run the four-stage ring of the 128x128 kernel: 2, 3, 4, 5, 8, 9, 12 and 16 k-steps here (prologue shorter
    than the ring, slot wrap-around, a last stage in slot 0 under the epilogue's staging areas)."""
    g = torch.Generator().manual_seed(M + N + K + tb)
    a, b = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) * 0.2
    A, B = dev(a, BF16), dev(b.t().contiguous() if tb else b, BF16)
    bias = dev(torch.randn(N, generator=g))
    resid = dev(torch.randn(M, N, generator=g), BF16)
    pre = dev(torch.randn(M, N, generator=g), BF16)
    acc = A.double() @ (B.double().t() if tb else B.double())
    accb = acc + bias.double()

    def both(**kw):
        outs = []
        for flags in (0, 4):
            k2 = dict(kw)
            if "aux_out" in k2:
                k2.pop("aux_out")
                k2["aux"] = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)
            out = gemm(lib, BF16, 0, tb, A, B, M, N, K, flags=flags, **k2)
            outs.append((out, k2.get("aux") if "aux_out" in kw else None))
        # element by element within one bf16 ulp of the other kernel (fma contraction may differ between kernels)
        for other in outs[1:]:
            assert torch.allclose(outs[0][0].float(), other[0].float(), rtol=2.0 ** -7, atol=2e-3)
            if outs[0][1] is not None:
                assert torch.allclose(outs[0][1].float(), other[1].float(), rtol=2.0 ** -7, atol=2e-3)
        return outs[0]

    out, _ = both(bias=bias)                                             # EPI_PLAIN with bias
    assert rel_err(out, accb) < TOL[BF16]
    out, _ = both()                                                      # EPI_PLAIN without
    assert rel_err(out, acc) < TOL[BF16]
    out, aux = both(bias=bias, act=1, aux_out=True)                      # EPI_GELU_AUX
    assert rel_err(aux, accb) < TOL[BF16]
    assert rel_err(out, torch.tensor(O.gelu(accb.cpu().numpy()))) < TOL[BF16]
    out, _ = both(bias=bias, resid=resid)                                # EPI_RESID
    assert rel_err(out, accb + resid.double()) < TOL[BF16]
    out, _ = both(resid=resid)                                           # EPI_RESID, no bias (dgrad c_attn)
    assert rel_err(out, acc + resid.double()) < TOL[BF16]
    out, _ = both(bias=bias, resid=resid, p_drop=0.25, seed=77, rng=9)   # EPI_RESID + dropout (oracle's mask)
    keep = O.dropout_keep_rows(77, 9, M, N, 0.25)
    assert rel_err(out, accb.cpu() * torch.tensor(keep / 0.75) + resid.double().cpu()) < TOL[BF16]
    out, _ = both(act=2, aux=pre)                                        # EPI_GELUGRAD
    assert rel_err(out, acc.cpu() * torch.tensor(O.gelu_grad(pre.double().cpu().numpy()))) < TOL[BF16]


@pytest.mark.parametrize("M,N,K,tb", [(512, 512, 256, 1), (1024, 768, 128, 0), (136, 264, 128, 1), (1024, 256, 1024, 1)])
def test_gemm_fused_column_sums(lib, M, N, K, tb):
    """cmp_gemm_colsum_next: the next GEMM also accumulates the column sums of its STORED bf16 output into an fp32
    vector (bias gradient) -- fused into the compile-time epilogues (full 256-tiles) or via a colsum pass (ragged)."""
    g = torch.Generator().manual_seed(M + N)
    a, b = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) * 0.2
    A, B = dev(a, BF16), dev(b.t().contiguous() if tb else b, BF16)
    pre = dev(torch.randn(M, N, generator=g), BF16)
    for kw in (dict(), dict(act=2, aux=pre)):
        out_vec = torch.full((N,), 3.0, device="cuda")
        ck(lib, lib.cmp_gemm_colsum_next(P(out_vec)))
        out = gemm(lib, BF16, 0, tb, A, B, M, N, K, **kw)
        ref = out.double().sum(0) + 3.0
        assert rel_err(out_vec, ref) < 1e-5
        again = gemm(lib, BF16, 0, tb, A, B, M, N, K, **kw)            # one-shot: the next launch does not touch it
        assert torch.equal(out, again) and rel_err(out_vec, ref) < 1e-5


@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("flags", [4, 8, 16, 48, 16 | 128])
def test_gemm_wgrad_shape_large_k(lib, dtype, flags):
    """wgrad: contraction over tokens (K=4096), split-K via partial slabs + ordered reduce (flags 16, 48: a workspace is
    registered) or f32 atomics (other kernels, or flag 128); ragged output (V=390 rows)."""
    M, N, K = 390, 128, 4096
    ws = torch.empty(8 * M * N + 64, device="cuda")
    ck(lib, lib.cmp_gemm_set_workspace(P(ws), ws.numel() * 4))
    g = torch.Generator().manual_seed(11)
    At = dev(torch.randn(K, 448, generator=g) * 0.1, dtype)       # stored [K][ld=448], logical A[m,k]=At[k,m]
    At[:, 390:] = 0
    B = dev(torch.randn(K, N, generator=g) * 0.1, dtype)
    C0 = torch.zeros(M, N, device="cuda", dtype=torch.float32)
    out = gemm(lib, dtype, 1, 0, At, B, M, N, K, out_fp32=True, splitk=8, C0=C0, flags=flags)
    ref = At.double()[:, :390].t() @ B.double()
    assert rel_err(out, ref) < TOL[dtype]
    if dtype == BF16 and flags in (16, 48):          # the slab path is bitwise reproducible
        C1 = torch.zeros(M, N, device="cuda", dtype=torch.float32)
        out2 = gemm(lib, dtype, 1, 0, At, B, M, N, K, out_fp32=True, splitk=8, C0=C1, flags=flags)
        assert torch.equal(out, out2)
    ck(lib, lib.cmp_gemm_set_workspace(None, 0))


# ------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("rows,E", [(66, 64), (130, 256), (1000, 512), (37, 768)])
def test_layernorm_fwd_bwd(lib, dtype, rows, E):
    g = torch.Generator().manual_seed(rows + E)
    x = dev(torch.randn(rows, E, generator=g) * 2 + 0.5, dtype)
    gamma, beta = dev(torch.randn(E, generator=g)), dev(torch.randn(E, generator=g))
    y = torch.empty_like(x)
    mean = torch.empty(rows, device="cuda"); rstd = torch.empty(rows, device="cuda")
    ck(lib, lib.cmp_k_layernorm_fwd(stream(), P(x), P(gamma), P(beta), P(y), P(mean), P(rstd), rows, E, 1e-5, dtype))
    torch.cuda.synchronize()
    yr, cache = O.layernorm_fwd(x.double().cpu().numpy(), gamma.double().cpu().numpy(), beta.double().cpu().numpy(), 1e-5)
    assert rel_err(y, torch.tensor(yr)) < TOL[dtype]
    assert rel_err(rstd, torch.tensor(cache[1][:, 0])) < 1e-5
    dy = dev(torch.randn(rows, E, generator=g), dtype)
    resid = dev(torch.randn(rows, E, generator=g), dtype)
    dx = torch.empty_like(x)
    dg = torch.full((E,), 1.0, device="cuda"); db = torch.full((E,), -1.0, device="cuda")
    ws = torch.empty(lib.cmp_k_layernorm_bwd_ws(rows, E) // 4 + 16, device="cuda")
    ck(lib, lib.cmp_k_layernorm_bwd(stream(), P(dy), P(x), P(gamma), P(mean), P(rstd), P(resid), P(dx), P(dg), P(db), P(ws),
                                    rows, E, dtype))
    torch.cuda.synchronize()
    dxr, dgr, dbr = O.layernorm_bwd(dy.double().cpu().numpy(), cache, gamma.double().cpu().numpy())
    assert rel_err(dx, torch.tensor(dxr) + resid.double().cpu()) < TOL[dtype]
    assert rel_err(dg, torch.tensor(dgr) + 1.0) < 3e-5 * math.sqrt(rows) + (0 if dtype == FP32 else 1e-3)
    assert rel_err(db, torch.tensor(dbr) - 1.0) < 3e-5 * math.sqrt(rows) + (0 if dtype == FP32 else 1e-3)
    # fused consumer prologue: dropout-gradient mask of dx and its column sums
    dx2 = torch.empty_like(x); dmask = torch.zeros_like(x)
    dg2 = torch.zeros(E, device="cuda"); db2 = torch.zeros(E, device="cuda"); cs = torch.full((E,), 2.0, device="cuda")
    ck(lib, lib.cmp_k_layernorm_bwd_fused(stream(), P(dy), P(x), P(gamma), P(mean), P(rstd), P(resid), P(dx2), P(dg2), P(db2), P(ws),
                                          rows, E, dtype, P(dmask), P(cs), 0.25, 41, 6))
    torch.cuda.synchronize()
    assert torch.equal(dx2, dx)
    keep = torch.tensor(O.dropout_keep_rows(41, 6, rows, E, 0.25) / 0.75)
    want = dx.double().cpu() * keep
    assert rel_err(dmask, want) < TOL[dtype]
    assert rel_err(cs, dmask.double().cpu().sum(0) + 2.0) < 3e-5 * math.sqrt(rows) + (0 if dtype == FP32 else 2e-3)


# ------------------------------------------------------------------------------------------ attention
def attn_ref(qkv, B, T, H, D, keep=None, p=0.0):
    """float64 restatement of transformer.py:331-371 incl. the exact -1e4 masking; returns o, lse and a closure for grads."""
    E = H * D
    x = qkv.double().cpu().reshape(B, T, 3 * E).clone().requires_grad_(True)
    q, k, v = x.split(E, dim=2)
    sh = lambda t: t.reshape(B, T, H, D).permute(0, 2, 1, 3)
    q, k, v = sh(q), sh(k), sh(v)
    w = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(D))
    b = torch.tril(torch.ones(T, T, dtype=torch.float64))
    w = w * b - 1e4 * (1 - b)
    lse = torch.logsumexp(w, -1)
    pr = torch.softmax(w, -1)
    if keep is not None:
        pr = pr * torch.tensor(keep.reshape(B, H, T, T) / (1 - p))
    o = (pr @ v).permute(0, 2, 1, 3).reshape(B, T, E)
    return x, o, lse


# The attention case tables are module-level so that tests/test_attn_plan_host.py can hold every row to the launcher's plan on the CPU:
# the kernel form a row's comment names IS the form it reaches.
ATTN_FWD_BWD_SHAPES = [(2, 33, 4, 16), (1, 64, 2, 32), (2, 200, 2, 64), (1, 130, 1, 128), (1, 256, 3, 64), (1, 333, 2, 64), (1, 520, 1, 32)]
ATTN_FWD_BWD_P = [0.0, 0.2]


@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("B,T,H,D", ATTN_FWD_BWD_SHAPES)
@pytest.mark.parametrize("p", ATTN_FWD_BWD_P)
def test_attention_fwd_bwd(lib, dtype, B, T, H, D, p):
    E = H * D
    g = torch.Generator().manual_seed(B * 1000 + T + D)
    qkv = dev(torch.randn(B * T, 3 * E, generator=g), dtype)
    o = torch.zeros(B * T, E, device="cuda", dtype=tdt(dtype))
    lse = torch.zeros(B * H * T, device="cuda")
    ck(lib, lib.cmp_k_attn_fwd(stream(), P(qkv), P(o), P(lse), B, T, H, D, 1, dtype, p, 1234, 21))
    torch.cuda.synchronize()
    keep = O.dropout_keep_attn(1234, 21, B * H, T, p) if p > 0 else None
    x, oref, lseref = attn_ref(qkv, B, T, H, D, keep, p)
    tol = TOL[dtype] * (3 if dtype == BF16 else 1)
    assert rel_err(o, oref.detach().reshape(B * T, E)) < tol
    assert rel_err(lse, lseref.detach().reshape(-1)) < (1e-5 if dtype == FP32 else 2e-2)
    do = dev(torch.randn(B * T, E, generator=g), dtype)
    oref.backward(do.double().cpu().reshape(B, T, E))
    dqkv = torch.zeros(B * T, 3 * E, device="cuda", dtype=tdt(dtype))
    delta = torch.zeros(B * H * T, device="cuda")
    # backward consumes the kernel's own o / lse (as the train step does); armed: it also accumulates the c_attn bias
    # gradient (column sums of [dQ|dK|dV]) from its f32 accumulators, on top of the vector's contents
    bias_grad = torch.full((3 * E,), 2.0, device="cuda")
    ck(lib, lib.cmp_attn_bwd_bias_next(P(bias_grad)))
    ck(lib, lib.cmp_k_attn_bwd(stream(), P(qkv), P(o), P(do), P(lse), P(delta), P(dqkv), B, T, H, D, 1, dtype, p, 1234, 21))
    torch.cuda.synchronize()
    ref = x.grad.reshape(B * T, 3 * E)
    assert rel_err(bias_grad, ref.sum(0) + 2.0) < tol
    assert rel_err(delta, (do.double() * o.double()).reshape(B, T, H, D).sum(-1).permute(0, 2, 1).reshape(-1)) < tol
    # per slice, relative to that slice's largest reference value -- but not to less than 10 % of the whole gradient's: at T = 1
    # dq is exactly zero in exact arithmetic (p = 1, dp = delta) and the kernel's dp - delta is the rounding residue of the
    # stored o (bf16 with dropout: ~2^-9 of |dO.v|, i.e. ~1e-3 of the gradient's scale)
    whole = ref.abs().max().item()
    for name, sl in (("dq", slice(0, E)), ("dk", slice(E, 2 * E)), ("dv", slice(2 * E, 3 * E))):
        err = (dqkv[:, sl].double().cpu() - ref[:, sl]).abs().max().item()
        assert err / max(ref[:, sl].abs().max().item(), 0.1 * whole, 1e-30) < tol * 2, name


def check_attention_groups(lib, B, H, D, T, dtype, p, groups, inputs="randn"):
    """The whole grid runs on the GPU; the float64 reference is computed for the listed (batch, head) groups, each of them
    checked in full: o, lse, dq, dk, dv -- first with the global-maximum tolerances this file has always used, then per element under
    the limits of tests/attention_bounds.py (attn_check).  inputs: "randn", or "planted" (attention_bounds.attn_inputs: every query
    weights a partner key, so that a key or a tile that some row does not see moves that row by many limits)."""
    import attention_bounds as AB
    E = H * D
    g = torch.Generator().manual_seed(T + int(p * 100) + dtype + B)
    if inputs == "planted":
        qkv, do = (dev(t, dtype) for t in AB.attn_inputs(B, T, H, D, 1.0 / math.sqrt(D), seed=T + int(p * 100) + dtype + B, device="cuda"))
    else:
        qkv = dev(torch.randn(B * T, 3 * E, generator=g), dtype)
        do = dev(torch.randn(B * T, E, generator=g), dtype)
    o = torch.zeros(B * T, E, device="cuda", dtype=tdt(dtype))
    lse = torch.zeros(B * H * T, device="cuda")
    ck(lib, lib.cmp_k_attn_fwd(stream(), P(qkv), P(o), P(lse), B, T, H, D, 1, dtype, p, 77, 9))
    dqkv = torch.zeros(B * T, 3 * E, device="cuda", dtype=tdt(dtype))
    delta = torch.zeros(B * H * T, device="cuda")
    ck(lib, lib.cmp_k_attn_bwd(stream(), P(qkv), P(o), P(do), P(lse), P(delta), P(dqkv), B, T, H, D, 1, dtype, p, 77, 9))
    torch.cuda.synchronize()
    qh = qkv.double().cpu().reshape(B, T, 3, H, D)
    oh = o.double().cpu().reshape(B, T, H, D)
    dh = do.double().cpu().reshape(B, T, H, D)
    gh = dqkv.double().cpu().reshape(B, T, 3, H, D)
    lh = lse.cpu().reshape(B, H, T)
    # no 128-position block of any (batch, head) group left at its zero initialisation: every block was visited by both launches
    # (single positions can be exactly zero: dq of position 0, dv of a position whose probabilities were all dropped)
    for t0 in range(0, T, 128):
        if p > 0 and T - t0 < 8:
            continue        # (a last block of a few positions: dk / dv of the final keys are all-zero whenever their few probabilities were dropped)
        assert bool((oh[:, t0:t0 + 128] != 0).any(-1).any(1).all()) and bool((lh[:, :, t0:t0 + 128] != 0).any(-1).all()), t0
        assert bool((gh[:, t0:t0 + 128] != 0).any(-1).any(1).all()), t0
    tol = TOL[dtype] * (3 if dtype == BF16 else 1)
    tri = torch.tril(torch.ones(T, T, dtype=torch.float64))
    for b, h in groups:
        x = qh[b, :, :, h, :].clone().requires_grad_(True)          # [T, 3, D]
        w = (x[:, 0] @ x[:, 1].T) * (1.0 / math.sqrt(D))
        w = w * tri - 1e4 * (1 - tri)
        pr = torch.softmax(w, -1)
        if p > 0:
            keep = O.dropout_keep_rows(77, 9, T, T, p, row0=(b * H + h) * T)
            pr = pr * torch.tensor(keep / (1 - p))
        oref = pr @ x[:, 2]
        oref.backward(dh[b, :, h, :])
        assert rel_err(oh[b, :, h, :], oref.detach()) < tol, (b, h)
        assert rel_err(lh[b, h], torch.logsumexp(w, -1).detach()) < (1e-5 if dtype == FP32 else 2e-2), (b, h)
        for j, name in enumerate(("dq", "dk", "dv")):
            assert rel_err(gh[b, :, j, h, :], x.grad[:, j]) < tol * 2, (b, h, name)
    what = "attention %s B%d T%d H%d D%d p%.1f %s" % ("bf16" if dtype == BF16 else "fp32", B, T, H, D, p, inputs)
    # planted: the groups that cover every partner offset the grid holds (the callers' lists are chosen for the schedule, not for that)
    bound_groups = AB.covering_groups(B, H) if inputs == "planted" else groups
    worst = AB.attn_check(qkv, do, o, lse, delta, dqkv, B, T, H, D, dtype, p, 1.0 / math.sqrt(D), 77, 9, bound_groups, what=what, raise_on_fail=False)
    print(AB.figures(what, worst, dtype))
    AB.raise_first(worst)


ATTN_FULL_LENGTH_CASES = [(BF16, 1024, 0.0), (BF16, 1024, 0.1), (BF16, 2048, 0.0), (BF16, 2048, 0.1), (FP32, 1024, 0.1)]
ATTN_FULL_LENGTH_BHD = (8, 8, 64)


@pytest.mark.parametrize("dtype,T,p", ATTN_FULL_LENGTH_CASES)
def test_attention_full_length_many_groups(lib, dtype, T, p):
    """BASELINE shapes (seq 1024 / 2048, D = 64) with B*H = 64 (batch, head) groups: the balanced q-block pairing, the XCD
    re-deal of workgroups and the 64-key fused softmax step run with >= 8 query blocks per group; five groups (first, last and
    three in between) against float64."""
    for inputs in ("randn", "planted"):
        check_attention_groups(lib, *ATTN_FULL_LENGTH_BHD, T, dtype, p, ((0, 0), (1, 5), (3, 2), (6, 7), (7, 7)), inputs=inputs)


ATTN_BLOCK_PLAN_CASES = [
    (BF16, 32, 8, 64, 1024, 0.1),      # 32 rows per XCD, 128 pairs over 96 slots: 24 rows paired, 8 as single blocks
    (BF16, 16, 8, 64, 1000, 0.1),      # less than one round of pairs: 12 of 16 rows as single blocks; ragged last block
    (BF16, 40, 8, 64, 640, 0.0),       # five blocks per row (the middle one runs alone in a paired row), 8 rows unpaired
    (BF16, 8, 16, 32, 2048, 0.1),      # 16 blocks per row, head size 32: dQ runs 4 of 16 rows single; the forward (4 per CU) pairs all 16
    (FP32, 40, 8, 64, 512, 0.1),       # parity mode: two workgroups per CU, 64 slots per XCD
]


@pytest.mark.parametrize("dtype,B,H,D,T,p", ATTN_BLOCK_PLAN_CASES)
def test_attention_block_plans(lib, dtype, B, H, D, T, p):
    """Forward and dQ launches whose paired workgroups do not fill whole rounds of the resident slots run the rows of the last
    round as single blocks, heaviest first (attention.hip attn_job / attn_plan_u): every block of every row must still be
    computed exactly once.  Groups from the paired part and from the unpaired part (row index within an XCD below the plan's
    count) against float64, and the whole output must be free of untouched (zero-initialised) rows."""
    rows = B * H
    groups = sorted({(0, 0), (0, H - 1), ((rows // 2) // H, (rows // 2) % H), ((rows - 9) // H, (rows - 9) % H), (B - 1, H - 1)})
    for inputs in ("randn", "planted"):
        check_attention_groups(lib, B, H, D, T, dtype, p, groups, inputs=inputs)


ATTN_KEY_SPLIT_CASES = [
    (1, 16, 16, 1024, 0.1),      # the reference's default configuration (default_config.yml:32-48) at batch 1
    (1, 16, 16, 1000, 0.0),      # ragged: the last 256-row staging tile and the last 32-row block are partial
    (2, 4, 32, 600, 0.1),        # head size 32; three staging tiles, the last one ragged
    (1, 2, 16, 96, 0.1),         # a single staging tile: three of the four waves own no key at all for the first block
]


@pytest.mark.parametrize("B,H,D,T,p", ATTN_KEY_SPLIT_CASES)
def test_attention_key_split_kernels(lib, B, H, D, T, p):
    """Small grids (B*H*ceil(T/128) <= 128 workgroups of the 128-row kind, bf16, head size <= 32) run the key-split forms of the
    three attention kernels (attention.hip KS): 32-row blocks, the four waves of a workgroup split every staged 256-row tile and
    merge their partial softmax states / gradient tiles through LDS.  Every (batch, head) group against float64, with the
    dropout masks the other kernels draw."""
    for inputs in ("randn", "planted"):
        check_attention_groups(lib, B, H, D, T, BF16, p, [(b, h) for b in range(B) for h in range(H)][:6] + [(B - 1, H - 1)], inputs=inputs)


ATTN_BIAS_PATH_CASES = [
    (8, 8, 64, 1024, 0.1, True),       # [tokens, 3E] gradient of 25 MB: the sums stay fused in dQ / dK-dV (float atomics)
    (5, 12, 64, 2048, 0.0, True),      # C4's head layout, 47 MB
    (1, 16, 16, 1024, 0.1, False),     # 1.6 MB: key-split kernels, the sums come from a column-sum pass over the stored gradient
    (8, 16, 16, 1024, 0.1, False),     # 12.6 MB: the 128-row kernels, column-sum pass
]


def test_attention_caps_are_what_the_host_tables_assume(lib):
    """cmp_attn_caps: what the launcher asks this device about the kernels of every (dtype, head size) -- resident workgroups per CU of the
    forward, dQ and rstd-scaled dQ kernels, the key-split opt-in -- is what tests/test_attn_plan_host.py plans the case tables with."""
    import test_attn_plan_host as HP
    for (dtype, D), per_kernel in HP.DEVICE_CAPS.items():
        for kernel, want in enumerate(per_kernel):
            wgs, ks_ok = C.c_int(-1), C.c_int(-1)
            rc = lib.cmp_attn_caps(dtype, D, kernel, C.byref(wgs), C.byref(ks_ok))
            if want is None:
                assert rc != 0 and "no kernel" in lib.cmp_last_error().decode(), (dtype, D, kernel)       # rstd rows exist in bf16 only
                continue
            ck(lib, rc)
            assert (wgs.value, ks_ok.value) == (want, HP.device_ks_ok(dtype, D)), (dtype, D, kernel)


def device_attn_plan(lib, dtype, B, T, H, D, p, backward, want_bias=0, has_ln_rows=0):
    """What the launcher decides for such a cmp_k_attn_fwd / cmp_k_attn_bwd call on this device (cmp_attn_caps, cmp_attn_plan)."""
    from composer_amd import _lib
    wgs, ks_ok, info = C.c_int(0), C.c_int(0), _lib.AttnPlanInfo()
    ck(lib, lib.cmp_attn_caps(dtype, D, (2 if has_ln_rows else 1) if backward else 0, C.byref(wgs), C.byref(ks_ok)))
    ck(lib, lib.cmp_attn_plan(dtype, B, T, H, D, p, 0, want_bias, has_ln_rows, backward, wgs.value, ks_ok.value, C.byref(info)))
    return info


@pytest.mark.parametrize("B,H,D,T,p,fused", ATTN_BIAS_PATH_CASES)
def test_attention_bias_gradient_paths(lib, B, H, D, T, p, fused):
    """The c_attn bias gradient = column sums of [dQ | dK | dV] (Conv1D bias under tf.GradientTape, transformer.py:205-209): fused
    into the backward kernels from their f32 accumulators where the launch is long enough to hide the atomics, a pass over the stored
    bf16 gradient otherwise (attn_plan.h: behind the key-split kernels, or at most 16 MiB; which one is read from the launcher's
    plan).  Either way it must equal the column sums of the gradient the same call stored -- exactly those of the stored values for the pass, within bf16 rounding of the summands for the fused form -- and
    accumulate on top of the vector's contents."""
    E = H * D
    g = torch.Generator().manual_seed(B + T + D)
    qkv = dev(torch.randn(B * T, 3 * E, generator=g), BF16)
    do = dev(torch.randn(B * T, E, generator=g), BF16)
    o = torch.zeros(B * T, E, device="cuda", dtype=torch.bfloat16)
    lse = torch.zeros(B * H * T, device="cuda")
    ck(lib, lib.cmp_k_attn_fwd(stream(), P(qkv), P(o), P(lse), B, T, H, D, 1, BF16, p, 5, 3))
    dqkv = torch.zeros(B * T, 3 * E, device="cuda", dtype=torch.bfloat16)
    delta = torch.zeros(B * H * T, device="cuda")
    bias = torch.full((3 * E,), 7.0, device="cuda")
    ck(lib, lib.cmp_attn_bwd_bias_next(P(bias)))
    ck(lib, lib.cmp_k_attn_bwd(stream(), P(qkv), P(o), P(do), P(lse), P(delta), P(dqkv), B, T, H, D, 1, BF16, p, 5, 3))
    torch.cuda.synchronize()
    planned = bool(device_attn_plan(lib, BF16, B, T, H, D, p, backward=1, want_bias=1).bias_fused)
    if int(os.environ.get("COMPOSER_ATTN_BIAS_PASS", "16")) == 16:      # (the measurement override moves the bound; the forms stay right)
        assert planned == fused
    fused = planned
    want = dqkv.double().sum(0).cpu() + 7.0
    scale = dqkv.double().abs().sum(0).cpu().clamp_min(1e-30)           # rounding of the summands is relative to their magnitudes
    err = ((bias.double().cpu() - want).abs() / scale).max().item()
    assert err < (3e-3 if fused else 2e-6), err
    # not armed: the next call leaves the vector alone
    ck(lib, lib.cmp_k_attn_bwd(stream(), P(qkv), P(o), P(do), P(lse), P(delta), P(dqkv), B, T, H, D, 1, BF16, p, 5, 3))
    torch.cuda.synchronize()
    assert ((bias.double().cpu() - want).abs() / scale).max().item() == err


def test_attention_forced_rescale(lib):
    """Online-softmax rescale branch: a key far down the sequence dominates a query row (rule: force the branch)."""
    B, T, H, D = 1, 192, 1, 64
    qkv = torch.randn(T, 3 * D) * 0.1
    qkv[150, :D] = 3.0            # query 150
    qkv[140, D:2 * D] = 5.0       # key 140 -> score 3*5*64/8 = 120 arrives in the 3rd key tile
    for dtype in (FP32, BF16):
        q = dev(qkv, dtype)
        o = torch.zeros(T, D, device="cuda", dtype=tdt(dtype)); lse = torch.zeros(T, device="cuda")
        ck(lib, lib.cmp_k_attn_fwd(stream(), P(q), P(o), P(lse), B, T, H, D, 1, dtype, 0.0, 0, 0))
        torch.cuda.synchronize()
        _, oref, _ = attn_ref(q, B, T, H, D)
        assert rel_err(o, oref.detach().reshape(T, D)) < TOL[dtype] * 3


# ------------------------------------------------------------------------------------------ loss / adam / embedding
@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("V,ldz", [(390, 448), (512, 512), (513, 576), (1384, 1408), (5000, 5056)])
def test_softmax_xent(lib, dtype, V, ldz):
    """V <= 512: the register-resident kernel; wider vocabularies (a config with more time-shift / velocity events than the
    default's 390, dataset.py vocab_size): the three-pass kernel."""
    rows = 300
    g = torch.Generator().manual_seed(3)
    z = torch.zeros(rows, ldz); z[:, :V] = torch.randn(rows, V, generator=g) * 3
    z[5, 10] = z[5, 20] = 50.0     # exact tie -> argmax must be the LOWER index
    y = torch.randint(0, V, (rows,), generator=g, dtype=torch.int32); y[5] = 10
    zd, yd = dev(z), dev(y)
    dz = torch.full((rows, ldz), 7.0, device="cuda", dtype=tdt(dtype))
    rl = torch.zeros(rows, device="cuda"); rc = torch.zeros(rows, device="cuda", dtype=torch.int32)
    ck(lib, lib.cmp_k_softmax_xent(stream(), P(zd), ldz, P(yd), P(dz), P(rl), P(rc), rows, V, 1.0 / rows, dtype))
    torch.cuda.synchronize()
    zz = z[:, :V].double()
    lse = torch.logsumexp(zz, -1)
    nll = lse - zz[torch.arange(rows), y.long()]
    assert rel_err(rl, nll) < 1e-5
    pred = zz.argmax(-1)
    pred[5] = 10
    assert torch.equal(rc.cpu().long(), (pred == y.long()).long())
    sm = torch.softmax(zz, -1); sm[torch.arange(rows), y.long()] -= 1; sm /= rows
    assert rel_err(dz[:, :V], sm) < (1e-5 if dtype == FP32 else 1e-2)
    assert (dz[:, V:] == 0).all()


def test_adam_keras_formulation(lib):
    n = 4096 + 8
    g = torch.Generator().manual_seed(9)
    p0, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    m0, v0 = torch.randn(n, generator=g) * 0.01, torch.rand(n, generator=g) * 0.01
    p, gd, m, v = dev(p0), dev(gr), dev(m0), dev(v0)
    sh = torch.zeros(n, device="cuda", dtype=torch.bfloat16)
    ck(lib, lib.cmp_k_adam(stream(), P(p), P(gd), P(m), P(v), P(sh), n, 1e-3, 0.9, 0.999, 1e-7, 7, 0.5))
    torch.cuda.synchronize()
    g64 = gr.double() * 0.5
    m1 = 0.9 * m0.double() + 0.1 * g64
    v1 = 0.999 * v0.double() + 0.001 * g64 * g64
    alpha = 1e-3 * math.sqrt(1 - 0.999 ** 7) / (1 - 0.9 ** 7)
    p1 = p0.double() - alpha * m1 / (v1.sqrt() + 1e-7)
    assert rel_err(m, m1) < 1e-6 and rel_err(v, v1) < 1e-6 and rel_err(p, p1) < 1e-6
    assert torch.equal(sh.cpu(), p.cpu().to(torch.bfloat16))


@pytest.mark.parametrize("dtype", [FP32, BF16])
def test_embedding_fwd_bwd(lib, dtype):
    B, T, E, V, W = 3, 17, 64, 390, 32
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, V, (B, T), generator=g, dtype=torch.int32)
    wte, wpe = torch.randn(V, E, generator=g), torch.randn(W, E, generator=g)
    out = torch.zeros(B * T, E, device="cuda", dtype=tdt(dtype))
    ids_d, wte_d, wpe_d = dev(ids), dev(wte), dev(wpe)      # keep alive across the launches
    ck(lib, lib.cmp_k_embed_fwd(stream(), P(ids_d), P(wte_d), P(wpe_d), P(out), B, T, E, 0, dtype, 0.3, 5, 2))
    torch.cuda.synchronize()
    keep = torch.tensor(O.dropout_keep_rows(5, 2, B * T, E, 0.3) / 0.7)
    ref = (wte[ids.long()] + wpe[:T][None]).reshape(B * T, E).double() * keep
    assert rel_err(out, ref) < (1e-6 if dtype == FP32 else 1e-2)
    dh = dev(torch.randn(B * T, E, generator=g), dtype)
    dwte = torch.zeros(V, E, device="cuda"); dwpe = torch.zeros(W, E, device="cuda")
    ck(lib, lib.cmp_k_embed_bwd(stream(), P(ids_d), P(dh), P(dwte), P(dwpe), B, T, E, 0, dtype, 0.3, 5, 2))
    torch.cuda.synchronize()
    d = dh.double().cpu() * keep
    rw = torch.zeros(V, E, dtype=torch.float64); rw.index_add_(0, ids.reshape(-1).long(), d)
    rp = torch.zeros(W, E, dtype=torch.float64); rp[:T] = d.reshape(B, T, E).sum(0)
    assert rel_err(dwte, rw) < 1e-5 and rel_err(dwpe, rp) < 1e-5


@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("B,T,E,V,p", [(8, 512, 512, 390, 0.3), (5, 1000, 768, 1384, 0.0), (33, 128, 64, 3, 0.1), (2, 2048, 1024, 8000, 0.2),
                                       (16, 256, 2048, 390, 0.0)])
def test_embedding_bwd_sorted_form(lib, dtype, B, T, E, V, p):
    """cmp_k_embed_bwd_v: the form the model's backward pass uses from 4096 tokens on -- tokens counting-sorted by id, up to 128 rows
    of one id summed by a workgroup before E atomics, position gradient as a per-position batch sum -- against float64 index_add /
    batch sums with the oracle's dropout masks; ids skewed (half the tokens share three ids), ids that never occur, and the
    gradients ACCUMULATE into what the buffers hold (the tied logits gradient is already in dwte when the model gets here)."""
    g = torch.Generator().manual_seed(B * T + V)
    ids = torch.randint(0, V, (B, T), generator=g, dtype=torch.int32)
    hot = torch.rand(B, T, generator=g) < 0.5
    ids[hot] = torch.randint(0, min(V, 3), (int(hot.sum()),), generator=g, dtype=torch.int32)
    W = T + 5
    dh = dev(torch.randn(B * T, E, generator=g), dtype)
    dwte0, dwpe0 = torch.randn(V, E, generator=g), torch.randn(W, E, generator=g)
    dwte, dwpe = dwte0.clone().cuda(), dwpe0.clone().cuda()
    ids_d = dev(ids)
    ck(lib, lib.cmp_k_embed_bwd_v(stream(), P(ids_d), P(dh), P(dwte), P(dwpe), B, T, E, 2, dtype, p, 5, 2, V))
    torch.cuda.synchronize()
    d = dh.double().cpu()
    if p > 0:
        d = d * torch.tensor(O.dropout_keep_rows(5, 2, B * T, E, p) / (1 - p))
    rw = dwte0.double().clone(); rw.index_add_(0, ids.reshape(-1).long(), d)
    rp = dwpe0.double().clone(); rp[2:2 + T] += d.reshape(B, T, E).sum(0)
    assert rel_err(dwte, rw) < 2e-5 and rel_err(dwpe, rp) < 2e-5
    assert torch.equal(dwpe[:2].cpu(), dwpe0[:2]) and torch.equal(dwpe[2 + T:].cpu(), dwpe0[2 + T:])


@pytest.mark.parametrize("dtype", [FP32, BF16])
def test_colsum(lib, dtype):
    rows, cols = 1000, 392
    x = dev(torch.randn(rows, cols), dtype)
    out = torch.ones(cols, device="cuda")
    ck(lib, lib.cmp_k_colsum(stream(), P(x), cols, P(out), rows, cols, dtype))
    torch.cuda.synchronize()
    assert rel_err(out, x.double().sum(0) + 1.0) < 1e-4
