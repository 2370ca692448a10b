"""-m gpu: the embedding kernels of composer_amd/csrc/elementwise.hip and the atomic-free column sums held to tests/embed_bounds.py: the
forward bit for bit, the partial statistics and every form of the backward pass per element, the atomic-free forms bit for bit at p = 0.
Every launch runs in a kernel_arena.Arena (guard bands; dwte / dwpe accumulate onto non-zero start values; workspaces exactly their
`_ws` size; W = pos0 + T exactly).  Every backward case first asserts the form it takes (cmp_embed_bwd_form).
tests/test_embed_checks_host.py proves on the CPU that these checks reject wrong kernels and that every case below reaches the path its
row names (`reach_*`: the launcher's arithmetic written out).

q (embed_bounds: the largest |emulation - reference| / S of an output over the case; for the partial statistics the relative fp32 floor) is
measured from the CPU emulation on EVERY element, never from a kernel.  Below, per case, fp32 / bf16 operands, the larger figure over
the case's p values: q in units of u = 2^-24, and the worst error / limit the kernels returned on one run on an MI355X.  No limit was
tuned to a kernel's result.  The forward cases (the rows of the statistics cases included) have no figure: they are bit for bit the
emulation, as are dwpe in every form and the atomic-free dwte at p = 0 (their figures below are those of p > 0, where the bound holds
them) and the column sums.  An error / limit of 0.50 is what a kernel gives that returns exactly what the emulation did: q is that emulation's
own error and MARGIN is 2.

    stats tokens 120 E 256                   q/u: mean - / 0.6, M2 - / 14.5
                                             err/limit: mean - / 0.02, M2 - / 0.03
    stats tokens 120 E 512                   q/u: mean - / 0.7, M2 - / 14.6
                                             err/limit: mean - / 0.02, M2 - / 0.03
    stats tokens 120 E 768                   q/u: mean - / 0.7, M2 - / 17.9
                                             err/limit: mean - / 0.03, M2 - / 0.03
    stats tokens 120 E 1280                  q/u: mean - / 0.9, M2 - / 15.1
                                             err/limit: mean - / 0.03, M2 - / 0.04
    stats tokens 120 E 1536                  q/u: mean - / 0.8, M2 - / 18.1
                                             err/limit: mean - / 0.03, M2 - / 0.03
    stats tokens 120 E 2048                  q/u: mean - / 0.8, M2 - / 27.2
                                             err/limit: mean - / 0.03, M2 - / 0.03
    stats tokens 32776 E 256                 q/u: mean - / 1.1, M2 - / 30.4
                                             err/limit: mean - / 0.05, M2 - / 0.02
    sorted (1, 4096, 8) V 8192               q/u: dwte 9.0 / 1.7, dwpe 0.9 / 0.6
                                             err/limit: dwte 0.47 / 0.26, dwpe 0.44 / 0.29
    sorted (3, 1366, 24) V 1025              q/u: dwte 8.0 / 1.8, dwpe 1.7 / 0.7
                                             err/limit: dwte 0.24 / 0.28, dwpe 0.50 / 0.33
    sorted (17, 241, 64) V 390               q/u: dwte 6.2 / 1.7, dwpe 3.9 / 1.0
                                             err/limit: dwte 0.38 / 0.33, dwpe 0.50 / 0.49
    sorted (5, 820, 768) V 1024              q/u: dwte 19.0 / 2.4, dwpe 2.6 / 1.0
                                             err/limit: dwte 0.41 / 0.45, dwpe 0.50 / 0.39
    sorted (3, 1366, 2048) V 3               q/u: dwte 14.3 / 4.7, dwpe 2.2 / 0.9
                                             err/limit: dwte 0.41 / 0.45, dwpe 0.50 / 0.43
    sorted (1, 4096, 64) V 1                 q/u: dwte 7.6 / 3.6, dwpe 1.0 / 0.6
                                             err/limit: dwte 0.33 / 0.36, dwpe 0.49 / 0.29
    threshold (5, 819, 64) V 390 form 0      q/u: dwte 21.0 / 1.8, dwpe 2.5 / 0.7
                                             err/limit: dwte 0.26 / 0.37, dwpe 0.50 / 0.36
    threshold (4, 1024, 64) V 390 form 1     q/u: dwte 7.2 / 2.5, dwpe 2.1 / 0.7
                                             err/limit: dwte 0.26 / 0.38, dwpe 0.50 / 0.33
    threshold (4, 1024, 64) V 8193 form 0    q/u: dwte 25.1 / 1.8, dwpe 2.2 / 0.8
                                             err/limit: dwte 0.24 / 0.40, dwpe 0.50 / 0.38
    atomic (3, 17, 64) V 390                 q/u: dwte 1.0 / 0.7, dwpe 1.2 / 0.6
                                             err/limit: dwte 0.44 / 0.31, dwpe 0.50 / 0.31
    atomic (1, 40, 64) V 390                 q/u: dwte 0.8 / 0.6, dwpe 0.9 / 0.6
                                             err/limit: dwte 0.42 / 0.29, dwpe 0.44 / 0.29
    atomic-free (1, 63, 64) V 390            q/u: dwte 1.0 / 1.0, dwpe 0.8 / 0.8
                                             err/limit: dwte 0.44 / 0.49, dwpe 0.41 / 0.42
    atomic-free (4, 25, 264) V 390           q/u: dwte 1.2 / 1.3, dwpe 1.6 / 1.8
                                             err/limit: dwte 0.50 / 0.50, dwpe 0.50 / 0.50
    atomic-free (17, 241, 64) V 390          q/u: dwte 5.9 / 4.4, dwpe 4.7 / 4.5
                                             err/limit: dwte 0.50 / 0.50, dwpe 0.50 / 0.50
    atomic-free (17, 241, 2048) V 17         q/u: dwte 9.8 / 9.7, dwpe 6.5 / 4.9
                                             err/limit: dwte 0.50 / 0.50, dwpe 0.50 / 0.50
    colsum_det (37, 392, 408)                err/limit against float64: out 0.06 / 0.10; bit for bit the emulation
    colsum_det (130, 64, 64)                 err/limit against float64: out 0.04 / 0.12; bit for bit the emulation
    colsum_det (8193, 64, 72)                err/limit against float64: out 0.02 / 0.11; bit for bit the emulation
    colsum_det (8200, 4608, 4608)            err/limit against float64: out 0.01 / -; bit for bit the emulation
"""
import ctypes as C

import numpy as np
import pytest
import torch

import embed_bounds as EB
from kernel_arena import Arena

pytestmark = pytest.mark.gpu
FP32, BF16 = 0, 1
F32, BF, I32 = torch.float32, torch.bfloat16, torch.int32
SEED, STREAM, POS0 = 5, 2, 3

# ---------------------------------------------------------------------------------------------------------------- the cases
# forward: (B, T, E, V, trips of the grid-stride loop in {dtype})
FWD = [(3, 17, 64, 390, {FP32: 1, BF16: 1}),
       (5, 820, 2048, 390, {FP32: 3, BF16: 2})]            # 4100 tokens: more than 4096 * 256 sixteen-byte chunks in either dtype
FWD_EX = ("pos", "type", "both")                           # the small case again through cmp_k_embed_fwd_ex
# forward with statistics (bf16): (B, T, E, MAXI, trips of the row loop, ragged last slot)
STATS = [(3, 40, 256, 1, 1, True), (3, 40, 512, 1, 1, False), (3, 40, 768, 2, 1, True), (3, 40, 1280, 4, 1, True),
         (3, 40, 1536, 4, 1, False), (3, 40, 2048, 4, 1, False),
         (8, 4097, 256, 1, 2, True)]                       # 32776 tokens: the grid is capped at 8192 workgroups of 4 rows
# sorted backward: (B, T, E, V, {dtype: (CPR, RP, idle threads, trips of the c0 loop)}, `per` of embed_scan2_kernel)
SORTED = [(1, 4096, 8, 8192, {FP32: (2, 128, 0, 1), BF16: (1, 256, 0, 1)}, 8),        # B = 1; CPR = 1; the widest vocabulary
          (3, 1366, 24, 1025, {FP32: (6, 42, 4, 1), BF16: (3, 85, 1, 1)}, 2),         # CPR does not divide 256; B odd; V = 1025
          (17, 241, 64, 390, {FP32: (16, 16, 0, 1), BF16: (8, 32, 0, 1)}, 1),         # 4097 tokens
          (5, 820, 768, 1024, {FP32: (192, 1, 64, 1), BF16: (96, 2, 64, 1)}, 1),      # B = 2 RP + 1 in bf16; V = 1024
          (3, 1366, 2048, 3, {FP32: (512, 1, 0, 2), BF16: (256, 1, 0, 1)}, 1),        # B = 2 RP + 1; CPR > 256 in fp32: two trips
          (1, 4096, 64, 1, {FP32: (16, 16, 0, 1), BF16: (8, 32, 0, 1)}, 1)]           # one id holds every token; B = 1
P_SORTED = (0.0, 0.2)
# the threshold: (B, T, E, V, form) -- each through cmp_k_embed_bwd_v, which brings a sort workspace
THRESHOLD = [(5, 819, 64, 390, 0), (4, 1024, 64, 390, 1), (4, 1024, 64, 8193, 0)]
ATOMIC = [(3, 17, 64, 390), (1, 40, 64, 390)]
# atomic-free backward: (B, T, E, V, `per`, segments without a token)
DET = [(1, 63, 64, 390, 1, 1), (4, 25, 264, 390, 2, 14), (17, 241, 64, 390, 65, 0), (17, 241, 2048, 17, 65, 0)]
P_DET = (0.0, 0.1)
# atomic-free column sums: (rows, cols, ldx, dtypes, splits, splits without a row, capped by the column grid)
COLSUM = [(37, 392, 408, (FP32, BF16), 1, 0, False), (130, 64, 64, (FP32, BF16), 2, 0, False),
          (8193, 64, 72, (FP32, BF16), 128, 1, False), (8200, 4608, 4608, (FP32,), 56, 0, True)]


# ---------------------------------------------------------------------------------------------------------------- plumbing
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


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def dname(dtype):
    return "bf16" if dtype else "fp32"


def report(what, res):
    print("EMBED_BOUNDS %s | err/limit %s | q/u %s" % (what, " ".join("%s %.2f" % kv for kv in res["worst"].items()),
                                                       " ".join("%s %.1f" % (k, v / EB.U) for k, v in res["q"].items())))
    EB.raise_first(res)


def tables(V, W, E, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 1.0, (V, E)).astype(np.float32), rng.normal(0, 1.0, (W, E)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- forward
def run_fwd(lib, dtype, B, T, E, V, p, ex=None):
    ntok, W = B * T, POS0 + T
    rng = np.random.default_rng(B * T + E)
    ids = rng.integers(0, V, ntok).astype(np.int32)
    ids[0], ids[-1] = 0, V - 1
    wte, wpe = tables(V, W, E, ntok)
    pos_ids = rng.integers(0, W, ntok).astype(np.int32) if ex in ("pos", "both") else None
    type_ids = rng.integers(0, V, ntok).astype(np.int32) if ex in ("type", "both") else None
    if pos_ids is not None:
        pos_ids[0], pos_ids[-1] = W - 1, 0
    ar = Arena("cuda", ntok * E * 4 + (V + W) * E * 4 + (1 << 20))
    ids_s = ar.operand(T_(ids), I32, 1, ntok, ntok, name="ids")
    wte_s, wpe_s = ar.operand(T_(wte), F32, V, E, E, name="wte"), ar.operand(T_(wpe), F32, W, E, E, name="wpe")
    pos_s = ar.operand(T_(pos_ids), I32, 1, ntok, ntok, name="pos_ids") if pos_ids is not None else None
    type_s = ar.operand(T_(type_ids), I32, 1, ntok, ntok, name="type_ids") if type_ids is not None else None
    out = ar.output(tdt(dtype), ntok, E, E, name="out")
    ar.arm()
    if ex is None:
        ck(lib, lib.cmp_k_embed_fwd(stream(), P(ids_s), P(wte_s), P(wpe_s), P(out), B, T, E, POS0, dtype, p, SEED, STREAM))
    else:
        ck(lib, lib.cmp_k_embed_fwd_ex(stream(), P(ids_s), P(wte_s), P(wpe_s), P(out), B, T, E, POS0, dtype, p, SEED, STREAM, P(pos_s), P(type_s)))
    ar.check()
    EB.embed_fwd_check(dtype, out.host(), ids, wte, wpe, T, POS0, p, SEED, STREAM, pos_ids, type_ids,
                       what="embed_fwd%s %s %s p %g" % ("_ex " + ex if ex else "", dname(dtype), (B, T, E), p))


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("B,T,E,V", [c[:4] for c in FWD])
def test_embedding_forward_is_exact(lib, dtype, B, T, E, V, p):
    run_fwd(lib, dtype, B, T, E, V, p)


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("ex", FWD_EX)
def test_embedding_forward_with_position_and_type_ids_is_exact(lib, dtype, ex, p):
    run_fwd(lib, dtype, *FWD[0][:4], p, ex=ex)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,T,E", [c[:3] for c in STATS])
def test_embedding_forward_statistics_within_bounds(lib, B, T, E, p):
    ntok, W, V, npart = B * T, POS0 + T, 390, E // 256
    rng = np.random.default_rng(ntok + E)
    ids = rng.integers(0, V, ntok).astype(np.int32)
    ids[0], ids[-1] = 0, V - 1
    wte, wpe = tables(V, W, E, ntok)
    wte += 0.75                                      # a mean that is not zero: the cancellation in x - mu
    ar = Arena("cuda", ntok * E * 2 + (V + W) * E * 4 + ntok * npart * 8 + (1 << 20))
    ids_s = ar.operand(T_(ids), I32, 1, ntok, ntok, name="ids")
    wte_s, wpe_s = ar.operand(T_(wte), F32, V, E, E, name="wte"), ar.operand(T_(wpe), F32, W, E, E, name="wpe")
    out = ar.output(BF, ntok, E, E, name="out")
    part = ar.output(F32, ntok, 2 * npart, 2 * npart, name="part")
    ar.arm()
    ck(lib, lib.cmp_k_embed_fwd_stats(stream(), P(ids_s), P(wte_s), P(wpe_s), P(out), P(part), B, T, E, POS0, p, SEED, STREAM))
    ar.check()
    report("stats tokens %d E %d p %g" % (ntok, E, p),
           EB.embed_stats_check(out.host(), part.host(), ids, wte, wpe, T, POS0, p, SEED, STREAM, raise_on_fail=False))


# ---------------------------------------------------------------------------------------------------------------- backward
def form_of(lib, B, T, E, dtype, V, sort_ws, det):
    words = int(lib.cmp_embed_bwd_sort_ws_words(B * T, V)) if sort_ws else 0
    return int(lib.cmp_embed_bwd_form(B, T, E, dtype, V, words, int(det)))


def run_bwd(lib, entry, form, dtype, B, T, E, V, p, inp=None, short=False):
    """One launch in a fresh arena through `entry` (bwd, bwd_v, bwd_det) -> (embed_bounds' result, dwte, dwpe as read back)."""
    ntok, W = B * T, POS0 + T
    inp = inp or EB.bwd_inputs(B, T, E, V, dtype, POS0, seed=ntok + E + V)
    ws_bytes = int(lib.cmp_k_embed_bwd_det_ws(V, E)) if entry == "bwd_det" else 0
    ar = Arena("cuda", ntok * E * 4 + (V + W) * E * 4 + ws_bytes + (1 << 20))
    ids_s = ar.operand(T_(inp["ids"]), I32, 1, ntok, ntok, name="ids")
    dh = ar.operand(T_(inp["dh"]), tdt(dtype), ntok, E, E, name="dh")
    dwte = ar.accumulator(T_(inp["dwte0"]), F32, V, E, E, name="dwte")
    dwpe = ar.accumulator(T_(inp["dwpe0"]), F32, W, E, E, name="dwpe")
    args = (stream(), P(ids_s), P(dh), P(dwte), P(dwpe), B, T, E, POS0, dtype, p, SEED, STREAM)
    if entry == "bwd_det":
        ws = ar.scratch(ws_bytes - (1 if short else 0), name="ws")                 # flush against its guard
        ar.arm()
        rc = lib.cmp_k_embed_bwd_det(*args, V, P(ws), ws_bytes - (1 if short else 0))
        if short:
            torch.cuda.synchronize()
            assert rc != 0, "a workspace one byte short must be refused"
            assert bool((ar.buf.cpu() == torch.from_numpy(ar.snap)).all()), "a refused launch wrote to the arena"
            return None
        ck(lib, rc)
    else:
        ar.arm()
        ck(lib, lib.cmp_k_embed_bwd_v(*args, V) if entry == "bwd_v" else lib.cmp_k_embed_bwd(*args))
    ar.check()
    res = EB.embed_bwd_check(form, dtype, inp["ids"], inp["dh"], B, T, POS0, p, SEED, STREAM, inp["dwte0"], inp["dwpe0"], dwte.host(),
                             dwpe.host(), raise_on_fail=False)
    return res, dwte.host(), dwpe.host()


@pytest.mark.parametrize("p", P_SORTED)
@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("B,T,E,V", [c[:4] for c in SORTED])
def test_sorted_backward_within_bounds(lib, dtype, B, T, E, V, p):
    assert form_of(lib, B, T, E, dtype, V, True, False) == 1
    report("sorted %s %s V %d p %g" % (dname(dtype), (B, T, E), V, p), run_bwd(lib, "bwd_v", 1, dtype, B, T, E, V, p)[0])


@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("B,T,E,V,form", THRESHOLD)
def test_backward_form_threshold_each_side_under_the_form_it_takes(lib, dtype, B, T, E, V, form):
    assert form_of(lib, B, T, E, dtype, V, True, False) == form
    report("threshold %s %s V %d form %d" % (dname(dtype), (B, T, E), V, form), run_bwd(lib, "bwd_v", form, dtype, B, T, E, V, 0.2)[0])


@pytest.mark.parametrize("p", P_SORTED)
@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("B,T,E,V", ATOMIC)
def test_atomic_backward_within_bounds(lib, dtype, B, T, E, V, p):
    assert form_of(lib, B, T, E, dtype, V, False, False) == 0
    report("atomic %s %s V %d p %g" % (dname(dtype), (B, T, E), V, p), run_bwd(lib, "bwd", 0, dtype, B, T, E, V, p)[0])


@pytest.mark.parametrize("p", P_DET)
@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("B,T,E,V", [c[:4] for c in DET])
def test_atomic_free_backward_exact_at_p0_within_bounds_and_reproducible(lib, dtype, B, T, E, V, p):
    assert form_of(lib, B, T, E, dtype, V, False, True) == 2
    inp = EB.bwd_inputs(B, T, E, V, dtype, POS0, seed=B * T + E + V)
    res, dwte, dwpe = run_bwd(lib, "bwd_det", 2, dtype, B, T, E, V, p, inp)
    report("atomic-free %s %s V %d p %g" % (dname(dtype), (B, T, E), V, p), res)
    _, dwte2, dwpe2 = run_bwd(lib, "bwd_det", 2, dtype, B, T, E, V, p, inp)
    EB.same_bits("atomic-free, second launch", "dwte", dwte2, dwte)
    EB.same_bits("atomic-free, second launch", "dwpe", dwpe2, dwpe)


@pytest.mark.parametrize("dtype", [FP32, BF16])
def test_atomic_free_backward_refuses_a_short_workspace(lib, dtype):
    run_bwd(lib, "bwd_det", 2, dtype, *DET[1][:4], 0.0, short=True)


# ---------------------------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("rows,cols,ldx,dtype", [(c[0], c[1], c[2], d) for c in COLSUM for d in c[3]])
def test_atomic_free_column_sums_exact_and_reproducible(lib, rows, cols, ldx, dtype):
    rng = np.random.default_rng(rows + cols)
    x = EB.store(rng.normal(0.3, 1.0, (rows, cols)), dtype)
    start = rng.normal(0, 3.0, cols).astype(np.float32)
    ws_bytes = int(lib.cmp_k_colsum_det_ws(rows, cols, dtype))
    assert ws_bytes == EB.colsum_splits(rows, cols, dtype) * cols * 4
    outs = []
    for launch in range(2):
        ar = Arena("cuda", rows * ldx * 4 + ws_bytes + (1 << 20), big=rows * ldx * 4 > (48 << 20))
        xs = ar.operand(T_(x), tdt(dtype), rows, cols, ldx, name="x")
        out = ar.vector(T_(start), F32, name="out", kind="acc")
        ws = ar.scratch(ws_bytes, name="ws")
        if launch == 0:
            ar.arm()
            assert lib.cmp_k_colsum_det(stream(), P(xs), ldx, P(out), rows, cols, dtype, P(ws), ws_bytes - 1) != 0, "one byte short must be refused"
            torch.cuda.synchronize()
            assert bool((ar.buf.cpu() == torch.from_numpy(ar.snap)).all()), "a refused launch wrote to the arena"
        ar.arm()
        ck(lib, lib.cmp_k_colsum_det(stream(), P(xs), ldx, P(out), rows, cols, dtype, P(ws), ws_bytes))
        ar.check()
        outs.append(out.host().reshape(-1))
        del ar
    worst = EB.colsum_det_check(dtype, x, start, outs[0], what="colsum_det %s %s" % (dname(dtype), (rows, cols, ldx)))
    print("EMBED_BOUNDS colsum_det %s %s | err/limit out %.2f (and bit for bit the emulation)" % (dname(dtype), (rows, cols, ldx), worst))
    EB.same_bits("colsum_det, second launch", "out", outs[1], outs[0])
