"""-m gpu: cmp_k_score_rows (composer_amd/csrc/score.hip) against float64, on the guard-banded arena of tests/kernel_arena.py:
logits with NaN in-row padding (a kernel that uses a column >= V fails), outputs flush against guard bands.

Shapes: rows = 300 with (V, ldz) = (390, 448) and (512, 512): the register-resident form with 16-byte loads; (390, 452): its 4-byte
form (a stride that is no multiple of 8), also reached with (390, 448) on a base pointer that is only 4-byte aligned; (513, 576):
the first wide shape; (5000, 5056): the widest vocabulary the project tests.
Bound: logp and entropy to rel_err < 1e-5 of float64, what tests/test_gpu_kernels.py::test_softmax_xent holds row_loss to on the
same kind of input (N(0, 3) logits); logp = -row_loss of cmp_k_softmax_xent to the same bound; the rank equal as integers."""
import ctypes as C

import numpy as np
import pytest
import torch

from kernel_arena import Arena

pytestmark = pytest.mark.gpu

ROWS = 300
RANK_FILL = -7
SHAPES = [(390, 448), (512, 512), (390, 452), (513, 576), (5000, 5056)]
# special rows (everything else: N(0, 3) logits, a random target)
R_TIE_HI, R_TIE_LO, R_Y0, R_YLAST, R_INFRUN, R_PAD_NEG, R_PAD_V, R_PEAK = 5, 6, 7, 8, 9, 10, 11, 12


@pytest.fixture(scope="module")
def lib():
    from composer_amd import _lib
    l = _lib.load()
    _lib.require_gpu()
    return l


def ck(lib, rc):
    assert rc == 0, lib.cmp_last_error().decode()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rel_err(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


_cases = {}


def case(V):
    """(z float32 [ROWS, V], y int32 [ROWS]) and the float64 reference (logp, rank, entropy), computed once per V."""
    if V in _cases:
        return _cases[V]
    g = torch.Generator().manual_seed(11 + V)
    z = torch.randn(ROWS, V, generator=g) * 3
    y = torch.randint(0, V, (ROWS,), generator=g, dtype=torch.int32)
    z[R_TIE_HI, 10] = z[R_TIE_HI, 20] = 50.0; y[R_TIE_HI] = 20          # exact tie at the target, the target on the higher index: rank 1
    z[R_TIE_LO, 10] = z[R_TIE_LO, 20] = 50.0; y[R_TIE_LO] = 10          # ... on the lower index: rank 0
    y[R_Y0] = 0
    y[R_YLAST] = V - 1
    z[R_INFRUN, 30:30 + V // 3] = float("-inf"); y[R_INFRUN] = 5        # a run of -inf columns
    y[R_PAD_NEG] = -1                                                     # not scored
    y[R_PAD_V] = V
    z[R_PEAK] = -40.0; z[R_PEAK, V // 2] = 30.0; y[R_PEAK] = V // 2      # one column holds all the mass: entropy ~ 0
    zz = z.double()
    lse = torch.logsumexp(zz, -1)
    valid = (y >= 0) & (y < V)
    yc = torch.where(valid, y, torch.zeros_like(y)).long()
    zy = zz[torch.arange(ROWS), yc]
    logp = torch.where(valid, zy - lse, torch.zeros_like(lse))
    col = torch.arange(V)
    rank = ((zz > zy[:, None]) | ((zz == zy[:, None]) & (col[None, :] < yc[:, None]))).sum(-1)
    rank = torch.where(valid, rank, torch.full_like(rank, -1))
    p = torch.softmax(zz, -1)
    ent = lse - torch.where(p > 0, p * zz, torch.zeros_like(zz)).sum(-1)
    _cases[V] = (z, y, logp, rank.to(torch.int32), ent)
    return _cases[V]


def launch(lib, V, ldz, z, y, want=(True, True, True), rows=ROWS, logp_ws=False, misalign=False):
    ar = Arena(nbytes=(rows * ldz * 4 + (64 << 10) + 255) // 256 * 256)
    if misalign:     # the matrix one float into a flat window (NaN in front, NaN in-row padding): a base pointer that is 4-byte aligned only
        flat = torch.full((rows * ldz + 1,), float("nan"))
        flat[1:].view(rows, ldz)[:, :V] = z
        zs = ar.vector(flat, torch.float32, name="logits")
    else:
        zs = ar.operand(z, torch.float32, rows, V, ldz, name="logits")
    ys = ar.vector(y, torch.int32, name="y")
    if logp_ws:      # a -inf result: the arena refuses non-finite outputs, so this window is checked here (its guards still by the arena)
        lp = ar.scratch(rows * 4, name="logp")
    else:
        lp = ar.output(torch.float32, 1, rows, rows, name="logp") if want[0] else None
    # (rank = -1, "not scored", is the arena's own fill pattern: the window starts at RANK_FILL instead, a value no row can get,
    #  and the comparison with the reference shows that every element was written)
    rk = ar.vector(torch.full((rows,), RANK_FILL), torch.int32, name="rank", kind="acc") if want[1] else None
    en = ar.output(torch.float32, 1, rows, rows, name="entropy") if want[2] else None
    ptr = lambda s: C.c_void_p(s.ptr()) if s is not None else None
    ar.arm()
    zp = C.c_void_p(zs.ptr() + 4) if misalign else ptr(zs)
    assert (zp.value % 16 == 4) == misalign
    ck(lib, lib.cmp_k_score_rows(stream(), zp, ldz, ptr(ys), ptr(lp), ptr(rk), ptr(en), rows, V))
    ar.check()       # guards, in-row padding and inputs bitwise unchanged; every requested output element written and finite
    return lp, rk, en


@pytest.mark.parametrize("V,ldz", SHAPES)
def test_score_rows_against_float64(lib, V, ldz):
    z, y, logp, rank, ent = case(V)
    lp, rk, en = launch(lib, V, ldz, z, y)
    got_lp, got_rk, got_en = lp.vec.cpu(), rk.vec.cpu(), en.vec.cpu()
    e1, e2 = rel_err(got_lp, logp), rel_err(got_en, ent)
    print("V=%d ldz=%d: logp rel_err %.3g, entropy rel_err %.3g" % (V, ldz, e1, e2))
    assert e1 < 1e-5 and e2 < 1e-5
    assert torch.equal(got_rk, rank)
    assert got_rk[R_TIE_HI] == 1 and got_rk[R_TIE_LO] == 0
    assert got_rk[R_PAD_NEG] == -1 and got_rk[R_PAD_V] == -1 and got_lp[R_PAD_NEG] == 0 and got_lp[R_PAD_V] == 0
    assert abs(got_en[R_PAD_NEG] - ent[R_PAD_NEG]) < 1e-5 * ent.abs().max()          # entropy as computed on a row that is not scored
    assert 0 <= got_en[R_PEAK] < 1e-5
    # the loss kernel on the same rows (targets of the rows not scored replaced: it takes ids in [0, V) only)
    ys = torch.where((y >= 0) & (y < V), y, torch.zeros_like(y))
    zp = torch.zeros(ROWS, ldz); zp[:, :V] = z
    zd, yd = zp.cuda(), ys.cuda()
    rl = torch.zeros(ROWS, device="cuda"); rc = torch.zeros(ROWS, device="cuda", dtype=torch.int32)
    ck(lib, lib.cmp_k_softmax_xent(stream(), C.c_void_p(zd.data_ptr()), ldz, C.c_void_p(yd.data_ptr()), None, C.c_void_p(rl.data_ptr()),
                                   C.c_void_p(rc.data_ptr()), ROWS, V, 1.0 / ROWS, 0))
    torch.cuda.synchronize()
    scored = (y >= 0) & (y < V)
    assert rel_err(got_lp[scored], -rl.cpu()[scored]) < 1e-5
    assert torch.equal((got_rk[scored] == 0), rc.cpu()[scored] == 1)


def test_score_rows_misaligned_base_pointer(lib):
    """ldz a multiple of 8 but the logits 4-byte aligned only: the dispatcher must take the 4-byte-load form (16-byte loads would be
    misaligned); the same results as the aligned launch to the float64 bound, the rank equal."""
    V, ldz = 390, 448
    z, y, logp, rank, ent = case(V)
    lp, rk, en = launch(lib, V, ldz, z, y, misalign=True)
    assert rel_err(lp.vec.cpu(), logp) < 1e-5 and rel_err(en.vec.cpu(), ent) < 1e-5
    assert torch.equal(rk.vec.cpu(), rank)


@pytest.mark.parametrize("V,ldz", SHAPES)
def test_score_rows_each_output_alone_and_null(lib, V, ldz):
    """Every output pointer null in turn, and each output alone: what is written does not depend on what else was asked for."""
    z, y, logp, rank, ent = case(V)
    full = [s.vec.cpu() for s in launch(lib, V, ldz, z, y)]
    for want in ((False, True, True), (True, False, True), (True, True, False), (True, False, False), (False, True, False),
                 (False, False, True)):
        got = launch(lib, V, ldz, z, y, want)
        for s, f, w in zip(got, full, want):
            assert (s is None) == (not w)
            if w:
                assert torch.equal(s.vec.cpu(), f)
    launch(lib, V, ldz, z, y, (False, False, False))             # nothing asked for: nothing written (the arena checks the guards)


@pytest.mark.parametrize("V,ldz", SHAPES)
def test_score_rows_target_at_minus_inf(lib, V, ldz):
    """A row whose target column holds -inf: logp = -inf, the rank as defined (every finite column, and the -inf columns below the
    target), the entropy finite.  Few rows, and a row count that is no multiple of the 4 waves of a block."""
    rows = 7
    z, y, _, _, _ = case(V)
    z, y = z[:rows].clone(), y[:rows].clone()
    y[:] = torch.tensor([3, 40, V - 1, 0, 17, 9, 25], dtype=torch.int32)
    z[2, 30:60] = float("-inf"); z[2, V - 1] = float("-inf")    # target -inf at the last column, a run of -inf below it
    z[4, 17] = float("-inf")                                      # the only -inf column is the target
    lp, rk, en = launch(lib, V, ldz, z, y, rows=rows, logp_ws=True)
    got_lp = lp.t.view(torch.float32)[0, :rows].cpu()
    got_rk, got_en = rk.vec.cpu(), en.vec.cpu()
    zz = z.double()
    lse = torch.logsumexp(zz, -1)
    zy = zz[torch.arange(rows), y.long()]
    assert got_lp[2] == float("-inf") and got_lp[4] == float("-inf")
    fin = torch.isfinite(zy)
    assert rel_err(got_lp[fin], (zy - lse)[fin]) < 1e-5
    assert got_rk[2] == (V - 31) + 30 and got_rk[4] == V - 1
    col = torch.arange(V)
    rank = ((zz > zy[:, None]) | ((zz == zy[:, None]) & (col[None, :] < y.long()[:, None]))).sum(-1).to(torch.int32)
    assert torch.equal(got_rk, rank)
    p = torch.softmax(zz, -1)
    ent = lse - torch.where(p > 0, p * zz, torch.zeros_like(zz)).sum(-1)
    assert torch.isfinite(got_en).all() and rel_err(got_en, ent) < 1e-5


def test_score_rows_refuses_bad_shapes(lib):
    z = torch.zeros(4, 16, device="cuda"); y = torch.zeros(4, device="cuda", dtype=torch.int32); o = torch.zeros(4, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    assert lib.cmp_k_score_rows(stream(), P(z), 16, P(y), P(o), None, None, 4, 17) == -1          # V > ldz
    assert lib.cmp_k_score_rows(stream(), P(z), 16, P(y), P(o), None, None, 4, 0) == -1
    assert lib.cmp_k_score_rows(stream(), None, 16, P(y), P(o), None, None, 4, 16) == -1
    assert lib.cmp_k_score_rows(stream(), P(z), 16, P(y), P(o), None, None, 0, 16) == 0           # no rows: nothing to do
