"""CPU checks of the GEMM launcher's decision (composer_amd/csrc/gemm_plan.h) through cmp_gemm_plan: which kernel family, grid,
epilogue kind, LayerNorm mode, slabs or atomics a cmp_k_gemm argument list gets -- for the case tables of
tests/test_gpu_kernel_guards.py (the kernel each row is meant to test IS the kernel it reaches), for the model's own launches,
for every refusal, and as a sweep of internal invariants.  Nothing here touches a GPU: pointers are host or made-up addresses."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

import test_gpu_kernel_guards as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32, BF16 = 0, 1
F32K, GENERIC, TILE128, RING, TILE256, P4_256, P4_128 = range(7)                    # CMP_GEMM_FAM_*
EPI_GENERIC, EPI_PLAIN, EPI_GELU_AUX, EPI_RESID, EPI_GELUGRAD, EPI_PLAIN32 = range(6)
KPAD_ZERO, F_GENERIC, F_TILE128, F_TILE256, F_P4, F_P4_128, F_ATOMICS = 1, 2, 4, 8, 16, 32, 128
PTR = C.c_void_p(0x7f0000001000)          # any non-null 16-byte-aligned value: never dereferenced
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from composer_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def plan_args(lib, args):
    """cmp_gemm_plan on a cmp_k_gemm argument list: the plan as a dict, or (status, message) of a refusal."""
    from composer_amd import _lib
    info = _lib.GemmPlanInfo()
    rc = lib.cmp_gemm_plan(*args, C.byref(info))
    if rc != 0:
        return rc, lib.cmp_last_error().decode()
    return {n: getattr(info, n) for n, _ in info._fields_}


def plan(lib, ta, tb, M, N, K, lda=None, ldb=None, ldc=None, bias=False, act=0, aux=False, resid=False, out_fp32=0, splitk=1,
         p=0.0, flags=0, dtype=BF16, A=PTR, B=PTR):
    """A launch with the model's leading dimensions unless given: rows as long as they are."""
    lda = lda if lda is not None else (M if ta else K)
    ldb = ldb if ldb is not None else (K if tb else N)
    ldc = ldc if ldc is not None else N
    return plan_args(lib, (dtype, ta, tb, M, N, K, A, lda, B, ldb, PTR, ldc, PTR if bias else None, act, PTR if aux else None,
                           N if aux else 0, PTR if resid else None, N if resid else 0, out_fp32, splitk, p, 77, 9, flags))


# ------------------------------------------------------------------------------------------ (a) the case tables, asserted
FORCED_FAMILY = {F_TILE128: (TILE128, RING), F_TILE256: (TILE256,), F_P4: (P4_256,), F_P4 | F_P4_128: (P4_128,)}


def expected_families(dtype, flags, row_index):
    if dtype == FP32:
        return (F32K,)
    if flags == 0:
        return {"generic": (GENERIC,), "tile128": (TILE128, RING)}[G.FREE_AUTO[row_index]]
    return (GENERIC,) if flags == F_GENERIC else FORCED_FAMILY[flags]


@pytest.mark.parametrize("family", G.FAMILIES, ids=G.FAMILY_IDS)
def test_case_tables_reach_the_kernel_they_name(lib, family):
    """Every row of FREE_ROWS / FORCED_ROWS / FP32_ROWS, every layout, padded and exact strides, staged by the code the GPU test
    launches with (stage_gemm_case on a host arena): the planned family is the one the table says -- never the generic fallback
    for a forced family."""
    dtype, flags = family
    rows = G.rows_of(dtype, flags)
    assert len(G.FREE_AUTO) == len(G.FREE_ROWS)
    for i, (ta, tb, M, N, K, kz, epi) in enumerate(rows):
        for padded in (True, False):
            args = G.stage_gemm_case(dtype, flags, ta, tb, M, N, K, kz, epi, padded, device="cpu")[4]
            p = plan_args(lib, args)
            what = (family, rows[i], padded, p)
            assert isinstance(p, dict), what
            assert p["family"] in expected_families(dtype, flags, i), what
            assert (p["a_km"], p["b_km"]) == (1 - ta, tb), what
            assert args[7] == (M if ta else (256 if kz else K)) + (8 if padded else 0) and args[11] == N + (16 if padded else 0), what


@pytest.mark.parametrize("family", G.FAMILIES, ids=G.FAMILY_IDS)
def test_split_k_modes_take_slabs_or_atomics(lib, family):
    """The split-K test's three modes at its shape (136 x 136 x 4096, splitk 2 and 8): only the deep pipeline folds slabs, and only
    with a workspace that holds splitk * M * N floats, ldc == N and without CMP_GEMM_ATOMICS; every forced family is reached."""
    dtype, flags = family
    M = N = 136
    K = 4096
    o = G.logical_ops(dtype, M, N, K)
    try:
        for (ta, tb), padded, splitk, mode in itertools.product([(1, 0), (0, 0)], (True, False), (2, 8), G.SPLIT_K_MODES):
            args = G.stage_split_k(lib, dtype, flags, ta, tb, M, N, K, o, padded, splitk, mode, device="cpu")[2]
            p = plan_args(lib, args)
            what = (family, ta, tb, padded, splitk, mode, p)
            # flags 0: a split-K launch is `big` only from 512 x 512 outputs on, so 136 x 136 stays on the 128x128 kernel
            want = (F32K,) if dtype == FP32 else (TILE128,) if flags == 0 else (GENERIC,) if flags == F_GENERIC else FORCED_FAMILY[flags]
            assert p["family"] in want, what
            assert p["nsplit"] == splitk and p["per"] * splitk == p["nk"], what
            slabs = p["family"] in (P4_256, P4_128) and mode == "slab" and not padded
            assert p["slabs"] == int(slabs) and p["swap"] == int(slabs) and (p["reduce_grid"] > 0) == slabs, what
    finally:
        assert lib.cmp_gemm_set_workspace(None, 0) == 0


@pytest.mark.parametrize("family", G.FAMILIES, ids=G.FAMILY_IDS)
def test_the_grid_hook_changes_one_plan_and_nothing_when_unarmed(lib, family):
    """cmp_gemm_grid_next is one-shot: over the case tables, the plan after an armed plan was consumed -- and the plan armed with
    (0, 0) -- is field for field the plan of a thread that never armed it; the armed plan itself differs in grid_x alone, and only
    on the persistent kernels (the cap, twice the cap for the 128x256 deep pipeline, or all items when they are fewer)."""
    dtype, flags = family
    for (ta, tb, M, N, K, kz, epi) in G.rows_of(dtype, flags):
        args = G.stage_gemm_case(dtype, flags, ta, tb, M, N, K, kz, epi, True, device="cpu")[4]
        p0 = plan_args(lib, args)
        assert lib.cmp_gemm_grid_next(3, 1) == 0
        p1 = plan_args(lib, args)
        p2 = plan_args(lib, args)
        assert lib.cmp_gemm_grid_next(0, 0) == 0
        p3 = plan_args(lib, args)
        assert p2 == p0 and p3 == p0, (family, ta, tb, M, N, K, epi)
        want = dict(p0)
        if p0["family"] >= TILE256:
            want["grid_x"] = min(p0["ntiles"] * p0["nsplit"], 6 if p0["family"] == P4_128 else 3)
        assert p1 == want, (family, ta, tb, M, N, K, epi, p1)
    assert lib.cmp_gemm_grid_next(257, 0) == INVALID and lib.cmp_gemm_grid_next(-1, 0) == INVALID
    p = plan(lib, 0, 1, T, 1536, 512, bias=True)            # a refused arming call arms nothing
    assert p["grid_x"] == 256, p


# ------------------------------------------------------------------------------------------ (b) the model's own launches
T = 131072          # C2: E = 512, 131 072 tokens, V = 390 (logits rows padded to 448)


def test_model_launches_c2(lib):
    # forward c_attn on the transposed shadow: 3072 tiles of 256x256 >= 192 -> big; both operands K-contiguous -> two-stage 256x256
    p = plan(lib, 0, 1, T, 1536, 512, bias=True)
    assert (p["family"], p["kind"], p["grid_x"], p["block"], p["sched"], p["cls"]) == (TILE256, EPI_PLAIN, 256, 512, 1, 1), p
    # c_proj: residual + dropout -> the residual kind carries the dropout
    p = plan(lib, 0, 1, T, 512, 512, bias=True, resid=True, p=0.1)
    assert (p["family"], p["kind"]) == (TILE256, EPI_RESID), p
    # c_fc: gelu with the stored pre-activation
    p = plan(lib, 0, 1, T, 2048, 512, bias=True, act=1, aux=True)
    assert (p["family"], p["kind"]) == (TILE256, EPI_GELU_AUX), p
    # GELU' dgrad with the armed bias-gradient column sums: fused into the compile-time epilogue, no pass afterwards
    assert lib.cmp_gemm_colsum_next(PTR) == 0
    p = plan(lib, 0, 1, T, 2048, 512, act=2, aux=True)
    assert (p["family"], p["kind"], p["colsum_fused"], p["colsum_pass"]) == (TILE256, EPI_GELUGRAD, 1, 0), p
    p = plan(lib, 0, 1, T, 2048, 512, act=2, aux=True)          # one-shot: consumed by the plan above as by a launch
    assert (p["colsum_fused"], p["colsum_pass"]) == (0, 0), p
    # tied logits: fp32 output has no compile-time kind
    p = plan(lib, 0, 1, T, 390, 512, ldc=448, out_fp32=1)
    assert (p["family"], p["kind"], p["grid_x"]) == (TILE256, EPI_GENERIC, 256), p
    # dlogits dgrad: K = 390 rides on the zero padding to 448; K % 32 != 0 keeps it off the deep pipeline; <A_KM, !B_KM>
    p = plan(lib, 0, 0, T, 512, 390, lda=448, flags=KPAD_ZERO)
    assert (p["family"], p["a_km"], p["b_km"], p["kind"]) == (TILE256, 1, 0, EPI_GENERIC), p
    assert plan(lib, 0, 0, T, 512, 390, lda=448)["family"] == GENERIC          # ... and without the flag it is not `fast`
    # tied weight gradient: 4 tiles, CMP_GEMM_P4, 64 splits of 64 k-steps of 32; atomics without a workspace ...
    p = plan(lib, 1, 0, 390, 512, T, lda=448, out_fp32=1, splitk=64, flags=F_P4)
    assert (p["family"], p["nsplit"], p["per"], p["ntiles"], p["grid_x"], p["slabs"], p["swap"], p["cls"]) == (P4_256, 64, 64, 4, 256, 0, 0, 2), p
    # ... slabs with one that holds 64 x 390 x 512 floats, atomics again when it is one byte short
    need = 64 * 390 * 512 * 4
    try:
        assert lib.cmp_gemm_set_workspace(PTR, need) == 0
        p = plan(lib, 1, 0, 390, 512, T, lda=448, out_fp32=1, splitk=64, flags=F_P4)
        assert (p["slabs"], p["swap"], p["reduce_grid"]) == (1, 1, 195), p          # 390 * 512 / 4 floats4 in blocks of 256
        assert lib.cmp_gemm_set_workspace(PTR, need - 1) == 0
        assert plan(lib, 1, 0, 390, 512, T, lda=448, out_fp32=1, splitk=64, flags=F_P4)["slabs"] == 0
    finally:
        assert lib.cmp_gemm_set_workspace(None, 0) == 0
    # block weight gradient g^T . dmo: wgrad_splits(131072, 2048, 512) = 256 / 16 tiles = 16; split-K of >= 512^2 outputs is big, K % 32 == 0
    p = plan(lib, 1, 0, 2048, 512, T, out_fp32=1, splitk=16)
    assert (p["family"], p["nsplit"], p["ntiles"], p["grid_x"], p["kind"]) == (P4_256, 16, 16, 256, EPI_GENERIC), p


def test_model_launches_small(lib):
    # the reference's default configuration (E = 256, 1024 tokens): c_attn has 12 tiles of 256x256 -> 128x128, whole tiles and 4 k-steps -> ring
    p = plan(lib, 0, 1, 1024, 768, 256, bias=True)
    assert (p["family"], p["kind"], p["ntiles"], p["grid_x"], p["smem"], p["sched"]) == (RING, EPI_PLAIN, 48, 48, 131072, 0), p
    # ragged K without the padding promise: no direct-to-LDS staging
    assert plan(lib, 0, 0, 1024, 768, 160)["family"] == GENERIC


def ln_next(lib, in_part=False, np_=2, cs=False, gamma_beta=False, out_part=False):
    f = lambda on: PTR if on else None
    assert lib.cmp_gemm_ln_next(f(in_part), np_, 1e-5, f(cs), f(gamma_beta), f(gamma_beta), f(out_part)) == 0


@pytest.mark.parametrize("E,tokens", [(512, 24576), (768, 16384)])
def test_fused_block_path_kinds_at_the_smallest_size(lib, E, tokens):
    """DESIGN.md section 4, the four fused-path kinds where (tokens / 256) * (E / 256) = 192, the `big` threshold of the [M, E] launches."""
    assert (tokens // 256) * (E // 256) == 192
    n = E // 256
    ln_next(lib, in_part=True, np_=n, cs=True)                                   # c_attn: fold
    p = plan(lib, 0, 1, tokens, 3 * E, E, bias=True)
    assert (p["family"], p["kind"], p["lnm"], p["np"]) == (TILE256, EPI_PLAIN, 1, n), p
    ln_next(lib, in_part=True, np_=n, gamma_beta=True, out_part=True)            # attention c_proj: rebuilt residual in, statistics out
    p = plan(lib, 0, 1, tokens, E, E, bias=True, resid=True, p=0.1)
    assert (p["family"], p["kind"], p["lnm"], p["np"], p["ntiles"]) == (TILE256, EPI_RESID, 3, n, 192), p
    ln_next(lib, in_part=True, np_=n, cs=True)                                   # c_fc: fold + gelu
    p = plan(lib, 0, 1, tokens, 4 * E, E, bias=True, act=1, aux=True)
    assert (p["family"], p["kind"], p["lnm"], p["np"]) == (TILE256, EPI_GELU_AUX, 1, n), p
    ln_next(lib, out_part=True, np_=n)                                           # MLP c_proj: statistics out only
    p = plan(lib, 0, 1, tokens, E, 4 * E, bias=True, resid=True)
    assert (p["family"], p["kind"], p["lnm"], p["np"]) == (TILE256, EPI_RESID, 2, 1), p
    # the backward pass's scale forms: rstd o (acc * gelu'(aux)) with fused column sums; acc + rstd o resid
    assert lib.cmp_gemm_ln_scale_next(PTR, n, 1e-5) == 0 and lib.cmp_gemm_colsum_next(PTR) == 0
    p = plan(lib, 0, 1, tokens, 4 * E, E, act=2, aux=True)
    assert (p["kind"], p["lnm"], p["np"], p["colsum_fused"]) == (EPI_GELUGRAD, 5, n, 1), p
    assert lib.cmp_gemm_ln_scale_next(PTR, n, 1e-5) == 0
    p = plan(lib, 0, 1, tokens, E, 3 * E, resid=True)
    assert (p["kind"], p["lnm"], p["np"]) == (EPI_RESID, 5, n), p
    # ln_f folded into the tied logits: [M, 390] has fewer tiles than the threshold, CMP_GEMM_TILE256 takes it to the kernel with the fold
    ln_next(lib, in_part=True, np_=n, cs=True)
    p = plan(lib, 0, 1, tokens, 390, E, ldc=448, bias=True, out_fp32=1, flags=F_TILE256)
    assert (p["family"], p["kind"], p["lnm"], p["np"]) == (TILE256, EPI_PLAIN32, 1, n), p
    ln_next(lib, in_part=True, np_=n, cs=True)
    p = plan(lib, 0, 1, tokens, 390, E, ldc=448, bias=True, out_fp32=1)
    if E == 512:                     # 96 x 2 tiles reach the threshold on their own
        assert (p["family"], p["kind"]) == (TILE256, EPI_PLAIN32), p
    else:                            # 64 x 2 = 128 tiles do not (model.hip passes the flag)
        assert p[0] == INVALID and "went to a kernel without one" in p[1], p


# ------------------------------------------------------------------------------------------ (c) refusals
def test_every_refusal_is_reached_with_its_message(lib):
    def refused(text, *a, **kw):
        r = plan(lib, *a, **kw)
        assert isinstance(r, tuple) and r[0] == INVALID and text in r[1], (text, r)
    refused("gemm: K must be positive", 0, 1, 256, 256, 0)
    for kw in (dict(bias=True), dict(act=1, aux=True), dict(resid=True), dict(p=0.5), dict(out_fp32=0)):
        refused("gemm: split-K needs a plain fp32 accumulate epilogue", 0, 1, 256, 256, 512, **dict(dict(out_fp32=1, splitk=2), **kw))
    refused("gemm: act=2 needs aux", 0, 1, 256, 256, 512, act=2)
    refused("gemm(bf16): leading dimensions must be multiples of 8 (lda=516 ldb=512)", 0, 1, 256, 256, 512, lda=516)
    refused("gemm(bf16): leading dimensions must be multiples of 8 (lda=512 ldb=260)", 0, 0, 256, 256, 512, ldb=260)
    refused("gemm(bf16): operands must be 16-byte aligned", 0, 1, 256, 256, 512, A=C.c_void_p(PTR.value + 8))
    refused("gemm(bf16): operands must be 16-byte aligned", 0, 1, 256, 256, 512, B=C.c_void_p(PTR.value + 2))
    assert isinstance(plan(lib, 0, 1, 256, 256, 512, dtype=FP32, lda=516, A=C.c_void_p(PTR.value + 4)), dict)      # bf16 rules only
    for kw in (dict(out_fp32=1), dict(out_fp32=1, splitk=2)):
        assert lib.cmp_gemm_colsum_next(PTR) == 0
        refused("gemm: column sums need a plain (non split-K) output in the compute dtype", 0, 1, 256, 256, 512, **kw)
    # a LayerNorm epilogue below the `big` threshold (190 tiles), on the fp32 kernel, on the deep pipeline: no kernel with one
    no_kernel = "gemm: a LayerNorm epilogue was asked of a launch that went to a kernel without one (M=%d N=512 K=512 dtype=%d flags=0)"
    ln_next(lib, in_part=True, cs=True)
    refused(no_kernel % (24320, BF16), 0, 1, 24320, 512, 512, bias=True)
    ln_next(lib, in_part=True, cs=True)
    refused(no_kernel % (24576, FP32), 0, 1, 24576, 512, 512, bias=True, dtype=FP32)
    ln_next(lib, in_part=True, cs=True)
    refused(no_kernel % (24576, BF16), 0, 0, 24576, 512, 512, bias=True)            # wrong layout: forward-layout launches take the deep pipeline
    # ... and on the 256x256 kernel: four segments, the wrong layout, a ragged row count, split-K, missing fold operands
    cannot = "gemm: this launch cannot carry the LayerNorm epilogue that was asked for (M=%d N=%d K=%d ta=%d tb=%d act=0)"
    ln_next(lib, in_part=True, np_=4, cs=True)
    refused(cannot % (24576, 512, 1024, 0, 1), 0, 1, 24576, 512, 1024, bias=True)
    ln_next(lib, in_part=True, cs=True)
    refused(cannot % (24576, 512, 512, 0, 0), 0, 0, 24576, 512, 512, bias=True, flags=F_TILE256)
    ln_next(lib, in_part=True, cs=True)
    refused(cannot % (24584, 512, 512, 0, 1), 0, 1, 24584, 512, 512, bias=True, flags=F_TILE256)
    ln_next(lib, in_part=True, cs=True)
    refused(cannot % (24576, 512, 512, 0, 1), 0, 1, 24576, 512, 512)                # the fold needs the folded bias
    ln_next(lib, in_part=True, cs=True)
    assert isinstance(plan(lib, 0, 1, 24576, 512, 512, bias=True), dict)            # the same launch with it
    assert plan(lib, 0, 1, 24576, 512, 512, bias=True)["lnm"] == 0                  # armed state is one-shot


# ------------------------------------------------------------------------------------------ (d) consistency sweep
EPIS = {"none": {}, "bias": dict(bias=True), "gelu": dict(bias=True, act=1, aux=True), "gelugrad": dict(act=2, aux=True),
        "resid": dict(bias=True, resid=True), "drop": dict(bias=True, resid=True, p=0.25), "f32": dict(out_fp32=1), "colsum": {}}


@pytest.mark.parametrize("ta,tb", G.LAYOUTS)
def test_plan_invariants_sweep(lib, ta, tb):
    """Layouts x M, N x K x epilogues x flags x splitk: whatever is planned is launchable and consistent with itself.  (The grid cap
    max_wgs is the model's, not the C ABI's: tests/gemm_plan_sweep.cpp sweeps it natively.)"""
    sizes, ks, flagset = (8, 136, 264, 512, 24576), (64, 72, 160, 200, 512), (0, 1, 2, 4, 8, 16, 48, 128)
    planned = 0
    for ctx in (0, 1):
        ws_bytes = 3 * 512 * 512 * 4 if ctx else 0
        assert lib.cmp_gemm_set_workspace(PTR if ctx else None, ws_bytes) == 0
        for M, N, K, (epi, kw), flags, sk in itertools.product(sizes, sizes, ks, EPIS.items(), flagset, (1, 2, 5)):
            if sk > 1 and epi not in ("none", "f32"):
                continue                                  # refused by rule: test_every_refusal_is_reached_with_its_message
            kp = (K + 63) // 64 * 64 if flags & 1 else K
            if epi == "colsum":
                assert lib.cmp_gemm_colsum_next(PTR) == 0
            kw = dict(kw, out_fp32=1) if sk > 1 else kw
            p = plan(lib, ta, tb, M, N, K, lda=M if ta else kp, ldb=kp if tb else N, ldc=N + 16 * ctx, splitk=sk, flags=flags, **kw)
            what = (ta, tb, M, N, K, epi, flags, sk, ctx, p)
            if epi == "colsum" and sk > 1:
                assert isinstance(p, tuple), what
                continue
            assert isinstance(p, dict), what
            planned += 1
            assert min(p["grid_x"], p["grid_y"], p["grid_z"], p["block"]) > 0, what
            assert p["per"] * p["nsplit"] >= p["nk"] > p["per"] * (p["nsplit"] - 1), what
            if p["family"] >= TILE256:
                assert p["grid_x"] <= (512 if p["family"] == P4_128 else 256) and p["sched"] == 1, what
            tile = 128 if p["family"] in (TILE128, RING) else 256
            if p["kind"] != EPI_GENERIC:
                assert M % tile == 0 and N % tile == 0 and p["family"] >= TILE128 and p["swap"] == 1, what
            assert not p["colsum_fused"] or p["kind"] != EPI_GENERIC, what
            assert p["colsum_fused"] + p["colsum_pass"] == int(epi == "colsum"), what
            if p["slabs"]:
                assert p["nsplit"] * M * N * 4 <= ws_bytes and p["reduce_grid"] > 0 and not flags & F_ATOMICS, what
            if flags & F_GENERIC:
                assert p["family"] == GENERIC, what
    assert lib.cmp_gemm_set_workspace(None, 0) == 0
    assert planned == 2 * 5 * 5 * 5 * 8 * (8 + 2 + 2)


def test_gemm_plan_header_stands_alone_under_host_sanitizers(tmp_path):
    """gemm_plan.h compiles with the host compiler, no HIP include path, and the sweep runs clean under ASan + UBSan: the header is
    HIP-free and M . N, the operand spans and nsplit . M . N . 4 do not overflow at M = 131072, N = 2048, K = 131072."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = "clang++"
    exe = str(tmp_path / "gemm_plan_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "gemm_plan_sweep.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "gemm_plan sweep ok" in r.stdout and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
    hdr = open(os.path.join(ROOT, "composer_amd", "csrc", "gemm_plan.h")).read()
    code = "\n".join(l.split("//")[0] for l in hdr.split("\n"))
    for banned in ("hip/", "hipcc", "getenv", "std::string", "std::vector", "std::map", "malloc", "new "):
        assert banned not in code, banned
