"""-m gpu: the row kernels of composer_amd/csrc/elementwise.hip held to per-element bounds (tests/row_bounds.py) at the row counts the
train step runs and at every size where their code takes another path.  Every launch runs in a kernel_arena.Arena (guard bands, NaN
padding, the backward workspace exactly cmp_k_layernorm_bwd_ws bytes).  tests/test_row_checks_host.py proves on the CPU that these
checks reject wrong kernels, that the planted inputs meet their conditions on every geometry below, and that every case reaches the
kernel form its row of the tables names (`reach_*`: the launcher's arithmetic written out).

Left out: the wide cross-entropy kernel's plain grid-stride loop past 32768 rows (no prefetch, no second code path: one more trip of the
loop its 1408-row cases run), and a launch with a null `dlogits` (the header's contract does not name it as allowed).

q (row_bounds: the largest |emulation - reference| / S of an output over the case; for mean, rstd and row_loss the relative fp32 floor) is
measured from the CPU emulation on EVERY row of the case, never from a kernel.  Below, per case (plain and fused launches and both
launches of a repeated case taken together), fp32 / bf16 operands: q in units of u = 2^-24, and the worst error / limit the kernels
returned on one run on an MI355X.  No limit was tuned to a kernel's result.  A bf16 output stands at 0.96 .. 1.00 of its limit by
construction: round-to-nearest alone uses up to 2^-8 |ref|, the BF16_OUT term.

    ln_fwd rows 65539 E 64             q/u: y 5.9 / 4.1, mean 8.2 / 0.8, rstd 6.3 / 12.6
                                       err/limit: y 0.23 / 1.00, mean 0.05 / 0.05, rstd 0.08 / 0.05
    ln_fwd rows 13 E 2048              q/u: y 11.0 / 17.7, mean 21.6 / 0.4, rstd 15.2 / 234.8
                                       err/limit: y 0.16 / 0.99, mean 0.02 / 0.01, rstd 0.05 / 0.00
    ln_fwd rows 13 E 1032              q/u: y 10.4 / 5.1, mean 12.5 / 0.9, rstd 7.6 / 117.3
                                       err/limit: y 0.10 / 0.98, mean 0.02 / 0.03, rstd 0.04 / 0.00
    ln_fwd rows 1 E 8                  q/u: y 1.0 / 0.9, mean 0.0 / 0.0, rstd 0.9 / 0.6
                                       err/limit: y 0.27 / 0.86, mean 0.04 / 0.00, rstd 0.05 / 0.03
    ln_fwd rows 3 E 8                  q/u: y 1.0 / 0.6, mean 1.9 / 0.0, rstd 0.8 / 0.9
                                       err/limit: y 0.24 / 0.74, mean 0.02 / 0.00, rstd 0.04 / 0.04
    ln_fwd rows 37 E 768               q/u: y 11.8 / 7.0, mean 12.7 / 0.9, rstd 8.1 / 85.1
                                       err/limit: y 0.06 / 0.99, mean 0.02 / 0.04, rstd 0.03 / 0.01
    ln_bwd rows 2048 E 64              q/u: dx 2.0 / 2.2, dgamma 10.6 / 9.9, dbeta 9.0 / 2.1, colsum 11.1 / 6.9
                                       err/limit: dx 0.29 / 0.99, dgamma 0.43 / 0.39, dbeta 0.42 / 0.23, colsum 0.33 / 0.43
    ln_bwd rows 2049 E 64              q/u: dx 1.8 / 2.0, dgamma 5.3 / 4.4, dbeta 4.9 / 1.6, colsum 4.9 / 3.6
                                       err/limit: dx 0.29 / 0.99, dgamma 0.33 / 0.50, dbeta 0.37 / 0.28, colsum 0.44 / 0.60
    ln_bwd rows 8200 E 64              q/u: dx 2.4 / 2.2, dgamma 7.0 / 5.5, dbeta 6.3 / 2.4, colsum 8.9 / 5.6
                                       err/limit: dx 0.24 / 1.00, dgamma 0.39 / 0.38, dbeta 0.41 / 0.41, colsum 0.18 / 0.30
    ln_bwd rows 2049 E 768             q/u: dx - / 4.1, dgamma - / 5.4, dbeta - / 3.0, colsum - / 4.1
                                       err/limit: dx - / 1.00, dgamma - / 0.53, dbeta - / 0.36, colsum - / 0.56
    ln_bwd rows 9 E 2048               q/u: dx 1.3 / 2.3, dgamma 2.5 / 2.3, dbeta 2.5 / 0.9, colsum 1.4 / 0.9
                                       err/limit: dx 0.33 / 0.98, dgamma 0.50 / 0.50, dbeta 0.50 / 0.46, colsum 0.50 / 0.39
    ln_bwd rows 1 E 64                 q/u: dx 0.6 / 0.6, dgamma 1.2 / 0.7, dbeta 0.5 / 0.5, colsum 0.5 / 0.5
                                       err/limit: dx 0.30 / 0.96, dgamma 0.50 / 0.36, dbeta 0.26 / 0.26, colsum 0.24 / 0.24
    ln_bwd rows 3 E 64                 q/u: dx 0.6 / 0.6, dgamma 1.2 / 0.8, dbeta 0.8 / 0.5, colsum 1.0 / 0.5
                                       err/limit: dx 0.21 / 0.85, dgamma 0.50 / 0.41, dbeta 0.38 / 0.26, colsum 0.50 / 0.26
    ln_stats_merge rows 2049 E 512     q/u: mean 0.4 / -, rstd 1.9 / -
                                       err/limit: mean 0.02 / -, rstd 0.08 / -
    ln_bwd_prescaled rows 2049 E 512   q/u: dx - / 2.5, dgamma - / 6.8, dbeta - / 5.6, colsum - / 4.6
                                       err/limit: dx - / 1.00, dgamma - / 0.34, dbeta - / 0.38, colsum - / 0.56
    ln_stats_merge rows 66 E 256       q/u: mean 0.0 / -, rstd 1.4 / -
                                       err/limit: mean 0.00 / -, rstd 0.06 / -
    ln_bwd_prescaled rows 66 E 256     q/u: dx - / 1.3, dgamma - / 3.1, dbeta - / 3.4, colsum - / 1.2
                                       err/limit: dx - / 0.99, dgamma - / 0.46, dbeta - / 0.38, colsum - / 0.46
    ln_stats_merge rows 66 E 1024      q/u: mean 0.4 / -, rstd 1.8 / -
                                       err/limit: mean 0.02 / -, rstd 0.05 / -
    ln_bwd_prescaled rows 66 E 1024    q/u: dx - / 1.6, dgamma - / 4.0, dbeta - / 4.4, colsum - / 1.4
                                       err/limit: dx - / 0.99, dgamma - / 0.36, dbeta - / 0.35, colsum - / 0.47
    ln_stats_merge rows 66 E 2048      q/u: mean 0.7 / -, rstd 2.0 / -
                                       err/limit: mean 0.03 / -, rstd 0.05 / -
    ln_bwd_prescaled rows 66 E 2048    q/u: dx - / 1.4, dgamma - / 3.7, dbeta - / 3.7, colsum - / 1.8
                                       err/limit: dx - / 1.00, dgamma - / 0.47, dbeta - / 0.42, colsum - / 0.50
    wgrad_ln_fix 512 x 1536            q/u: G 7.6 / -
                                       err/limit: G 0.11 / -
    wgrad_ln_fix 130 x 33              q/u: G 2.4 / -
                                       err/limit: G 0.27 / -
    wgrad_ln_fix 768 x 40              q/u: G 4.7 / -
                                       err/limit: G 0.13 / -
    xent rows 65539 V 50 ldz 56 off 0  q/u: dlogits 2.5 / 2.5, row_loss 2.3 / 2.3
                                       err/limit: dlogits 0.25 / 1.00, row_loss 0.08 / 0.08
    xent rows 520 V 390 ldz 448 off 0  q/u: dlogits 3.2 / 3.2, row_loss 2.5 / 2.5
                                       err/limit: dlogits 0.16 / 0.99, row_loss 0.05 / 0.05
    xent rows 520 V 512 ldz 512 off 0  q/u: dlogits 2.9 / 2.9, row_loss 2.2 / 2.2
                                       err/limit: dlogits 0.18 / 0.99, row_loss 0.06 / 0.06
    xent rows 520 V 8 ldz 8 off 0      q/u: dlogits 1.6 / 1.6, row_loss 1.7 / 1.7
                                       err/limit: dlogits 0.33 / 0.98, row_loss 0.07 / 0.07
    xent rows 520 V 1 ldz 8 off 0      q/u: dlogits 0.0 / 0.0, row_loss 0.0 / 0.0
                                       err/limit: dlogits 0.00 / 0.00, row_loss 0.00 / 0.00
    xent rows 520 V 390 ldz 390 off 0  q/u: dlogits 2.7 / 2.7, row_loss 2.2 / 2.2
                                       err/limit: dlogits 0.33 / 0.99, row_loss 0.06 / 0.06
    xent rows 520 V 50 ldz 51 off 0    q/u: dlogits 2.1 / 2.1, row_loss 1.6 / 1.6
                                       err/limit: dlogits 0.43 / 0.99, row_loss 0.06 / 0.06
    xent rows 520 V 390 ldz 448 off 1  q/u: dlogits 3.2 / 3.2, row_loss 2.5 / 2.5
                                       err/limit: dlogits 0.26 / 0.99, row_loss 0.06 / 0.06
    xent rows 1408 V 513 ldz 576 off 0 q/u: dlogits 2.9 / 2.9, row_loss 2.7 / 2.7
                                       err/limit: dlogits 0.28 / 0.99, row_loss 0.06 / 0.06
    xent rows 1408 V 1384 ldz 1408 off 0 q/u: dlogits 4.7 / 4.7, row_loss 3.2 / 3.2
                                       err/limit: dlogits 0.19 / 0.99, row_loss 0.04 / 0.04
"""
import ctypes as C

import numpy as np
import pytest
import torch

import row_bounds as RB
from kernel_arena import Arena
from oracle import transformer_oracle as O

pytestmark = pytest.mark.gpu
FP32, BF16 = 0, 1
F32, BF, I32 = torch.float32, torch.bfloat16, torch.int32
EPS = RB.EPS
SEED, STREAM, P_FUSED = 41, 6, 0.25

# ---------------------------------------------------------------------------------------------------------------- the cases
# LayerNorm forward: (rows, E, {dtype: MAXI}, most rows a wave takes, waves of the launch without a row)
LN_FWD = [(65539, 64, {FP32: 1, BF16: 1}, 3, 0),          # waves with 3, 2 and 1 rows: the prefetch branch (grid capped at 8192)
          (13, 2048, {FP32: 8, BF16: 4}, 1, 3),           # fp32 MAXI 8, bf16 MAXI 4
          (13, 1032, {FP32: 8, BF16: 4}, 1, 3),           # fp32: slot 4 holds lanes 0-1 only, slots 5-7 empty; bf16: a ragged third slot
          (1, 8, {FP32: 1, BF16: 1}, 1, 3),               # waves with no row; one chunk (bf16), two (fp32)
          (3, 8, {FP32: 1, BF16: 1}, 1, 1),
          (37, 768, {FP32: 4, BF16: 2}, 1, 3)]            # planted rows
# LayerNorm backward: (rows, E, dtypes, grid, direct atomics, most rows a wave takes, partials in the reduce tail, 96 KiB LDS opt-in)
LN_BWD = [(2048, 64, (FP32, BF16), 256, True, 2, 0, False),       # the last direct-atomics grid
          (2049, 64, (FP32, BF16), 257, False, 2, 1, False),      # one unrolled reduce pass of 8 x 32 partials plus a one-element tail
          (8200, 64, (FP32, BF16), 1024, False, 3, 0, False),     # the capped grid
          (2049, 768, (BF16,), 257, False, 2, 1, False),
          (9, 2048, (FP32, BF16), 2, True, 2, 0, True),           # fp32 MAXI 8, the LDS opt-in
          (1, 64, (FP32, BF16), 1, True, 1, 0, False),            # waves with no row
          (3, 64, (FP32, BF16), 1, True, 1, 0, False)]
TWICE = (2049, 8200)                                      # launched twice on the same inputs: atomics may reorder
PARTS = [(2049, 512), (66, 256), (66, 1024), (66, 2048)]  # `_prescaled`, ln_stats_merge: bf16, per-segment offsets planted
FIX = [(512, 1536), (130, 33), (768, 40)]
# cross-entropy: (rows, V, ldz, logits pointer offset in floats, kernel)
XENT = [(65539, 50, 56, 0, "xent8"), (520, 390, 448, 0, "xent8"), (520, 512, 512, 0, "xent8"), (520, 8, 8, 0, "xent8"), (520, 1, 8, 0, "xent8"),
        (520, 390, 390, 0, "generic"), (520, 50, 51, 0, "generic"), (520, 390, 448, 1, "generic"),
        (1408, 513, 576, 0, "wide"), (1408, 1384, 1408, 0, "wide")]


# ---------------------------------------------------------------------------------------------------------------- the launcher's arithmetic
def cdiv(a, b):
    return -(-a // b)


def ln_maxi(E, dtype):
    """elementwise.hip: the MAXI instance the LayerNorm launchers pick (16-byte chunks per lane, rounded up to 1, 2, 4, 8)."""
    m = cdiv(E // (8 if dtype == BF16 else 4), 64)
    return 1 if m == 1 else 2 if m == 2 else 4 if m <= 4 else 8


def reach_ln_fwd(rows, E, dtype):
    grid = min(cdiv(rows, 4), 8192)
    return ln_maxi(E, dtype), cdiv(rows, 4 * grid), max(0, 4 * grid - rows)


def reach_ln_bwd(rows, E, dtype):
    grid = RB.ln_bwd_grid(rows)
    direct = grid <= 256
    slices = min(grid, 32)
    per_slice = cdiv(grid, slices)                     # partials of slice 0
    return grid, direct, cdiv(rows, 4 * grid), 0 if direct else per_slice % 8, 4 * 3 * E * 4 > 65536


def reach_xent(ldz, offset_floats):
    if ldz > 512:
        return "wide"
    return "xent8" if ldz % 8 == 0 and offset_floats % 4 == 0 else "generic"


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


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def report(what, res):
    print(RB.figures(what, res))
    RB.raise_first(res)


def keep_of(rows, E, p):
    return O.dropout_keep_rows(SEED, STREAM, rows, E, p) if p > 0 else None


def stats_of(inp):
    """The statistics arrays a backward launch reads: the float64 statistics of the stored rows, rounded to fp32."""
    ref = RB.ln_fwd_ref(inp["x"], inp["gamma"], inp["beta"], EPS)
    return ref["mean"].astype(np.float32), ref["rstd"].astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- LayerNorm forward
@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("rows,E", [c[:2] for c in LN_FWD])
def test_layernorm_forward_within_bounds(lib, dtype, rows, E):
    inp = RB.ln_inputs(rows, E, dtype, seed=rows + E)
    dt = tdt(dtype)
    ar = Arena("cuda", 2 * rows * E * 4 + (1 << 20))
    x = ar.operand(T(inp["x"]), dt, rows, E, E, name="x")
    gamma, beta = ar.vector(T(inp["gamma"]), F32, name="gamma"), ar.vector(T(inp["beta"]), F32, name="beta")
    y = ar.output(dt, rows, E, E, name="y")
    mean, rstd = ar.output(F32, 1, rows, rows, name="mean"), ar.output(F32, 1, rows, rows, name="rstd")
    ar.arm()
    ck(lib, lib.cmp_k_layernorm_fwd(stream(), P(x), P(gamma), P(beta), P(y), P(mean), P(rstd), rows, E, EPS, dtype))
    ar.check()
    report("ln_fwd %s rows %d E %d" % ("bf16" if dtype else "fp32", rows, E),
           RB.ln_check(dtype, inp["x"], inp["gamma"], inp["beta"], EPS, y=y.host(), mean=mean.host().reshape(-1), rstd=rstd.host().reshape(-1),
                       raise_on_fail=False))


# ---------------------------------------------------------------------------------------------------------------- LayerNorm backward
def run_ln_bwd(lib, inp, dtype, rows, E, fused, form="plain", st=None):
    """One launch in a fresh arena -> the result of ln_check.  form: plain (cmp_k_layernorm_bwd / _fused), prescaled."""
    dt = tdt(dtype)
    ar = Arena("cuda", 8 * rows * E * 4 + (2 << 20))
    mat = lambda a, name: ar.operand(T(a), dt, rows, E, E, name=name)
    dy_h = inp["dy"]
    if form == "prescaled":                                # the stored, rstd-scaled gradient
        dy_h = RB.store(inp["dy"].astype(np.float64) * st[1][:, None].astype(np.float64), dtype)
    dy, x, resid = mat(dy_h, "dy"), mat(inp["x"], "x"), mat(inp["resid"], "resid")
    gamma = ar.vector(T(inp["gamma"]), F32, name="gamma")
    dx = ar.output(dt, rows, E, E, name="dx")
    rng = np.random.default_rng(rows)
    s_g, s_b, s_c = (rng.normal(0, 3.0, E).astype(np.float32) for _ in range(3))          # the accumulators start non-zero
    dg, db = ar.vector(T(s_g), F32, name="dgamma", kind="acc"), ar.vector(T(s_b), F32, name="dbeta", kind="acc")
    ws = ar.scratch(int(lib.cmp_k_layernorm_bwd_ws(rows, E)), name="ws")
    p = P_FUSED if fused else 0.0
    mean, rstd = ar.vector(T(st[0]), F32, name="mean"), ar.vector(T(st[1]), F32, name="rstd")
    kw = dict(stats=st)
    if form == "prescaled":
        dmask = ar.output(dt, rows, E, E, name="dmask")
        cs = ar.vector(T(s_c), F32, name="colsum", kind="acc")
        ar.arm()
        ck(lib, lib.cmp_k_layernorm_bwd_prescaled(stream(), P(dy), P(x), P(gamma), P(mean), P(rstd), P(resid), P(dx), P(dg), P(db), P(ws),
                                                  rows, E, P(dmask), P(cs), p, SEED, STREAM))
        kw.update(prescaled=True, dmask=dmask.host(), colsum=cs.host().reshape(-1), start_cs=s_c)
    elif fused:
        dmask = ar.output(dt, rows, E, E, name="dmask")
        cs = ar.vector(T(s_c), F32, name="colsum", kind="acc")
        ar.arm()
        ck(lib, lib.cmp_k_layernorm_bwd_fused(stream(), P(dy), P(x), P(gamma), P(mean), P(rstd), P(resid), P(dx), P(dg), P(db), P(ws),
                                              rows, E, dtype, P(dmask), P(cs), p, SEED, STREAM))
        kw.update(dmask=dmask.host(), colsum=cs.host().reshape(-1), start_cs=s_c)
    else:
        ar.arm()
        ck(lib, lib.cmp_k_layernorm_bwd(stream(), P(dy), P(x), P(gamma), P(mean), P(rstd), P(resid), P(dx), P(dg), P(db), P(ws), rows, E, dtype))
    ar.check()
    return RB.ln_check(dtype, inp["x"], inp["gamma"], dy=dy_h, resid=inp["resid"], dx=dx.host(), dgamma=dg.host().reshape(-1),
                       dbeta=db.host().reshape(-1), start_g=s_g, start_b=s_b, keep=keep_of(rows, E, p), p=p, raise_on_fail=False, **kw)


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("dtype,rows,E", [(d, c[0], c[1]) for c in LN_BWD for d in c[2]])
def test_layernorm_backward_within_bounds(lib, dtype, rows, E, fused):
    inp = RB.ln_inputs(rows, E, dtype, seed=rows + E + 1)
    st = stats_of(inp)
    for launch in range(2 if rows in TWICE else 1):
        report("ln_bwd%s %s rows %d E %d launch %d" % ("_fused" if fused else "", "bf16" if dtype else "fp32", rows, E, launch),
               run_ln_bwd(lib, inp, dtype, rows, E, fused, st=st))


@pytest.mark.parametrize("form", ["prescaled"])
@pytest.mark.parametrize("rows,E", PARTS)
def test_layernorm_backward_from_partials_and_prescaled_within_bounds(lib, rows, E, form):
    inp = RB.ln_inputs(rows, E, BF16, seed=rows + E + 2, segments=True)
    part = RB.parts_of(inp["x"]).astype(np.float32)
    ar = Arena("cuda", 1 << 20)
    npart = E // 256
    pt = ar.operand(T(part.reshape(rows, -1)), F32, rows, 2 * npart, 2 * npart, name="part")
    mean, rstd = ar.output(F32, 1, rows, rows, name="mean"), ar.output(F32, 1, rows, rows, name="rstd")
    ar.arm()
    ck(lib, lib.cmp_k_ln_stats_merge(stream(), P(pt), npart, EPS, P(mean), P(rstd), rows))
    ar.check()
    st = (mean.host().reshape(-1).numpy(), rstd.host().reshape(-1).numpy())
    report("ln_stats_merge rows %d E %d" % (rows, E), RB.merge_check(part, st[0], st[1], EPS, raise_on_fail=False))
    report("ln_bwd_%s rows %d E %d" % (form, rows, E), run_ln_bwd(lib, inp, BF16, rows, E, True, form=form, st=st))


@pytest.mark.parametrize("rows,cols", FIX)
def test_wgrad_ln_fix_within_bounds(lib, rows, cols):
    inp = RB.fix_inputs(rows, cols, seed=rows + cols)
    ar = Arena("cuda", 2 * rows * cols * 4 + (1 << 20))
    G = ar.accumulator(T(inp["G"]), F32, rows, cols, cols, name="G")
    gamma, beta = ar.vector(T(inp["gamma"]), F32, name="gamma"), ar.vector(T(inp["beta"]), F32, name="beta")
    cs = ar.vector(T(inp["colsum"]), F32, name="colsum")
    ar.arm()
    ck(lib, lib.cmp_k_wgrad_ln_fix(stream(), P(G), rows, cols, P(gamma), P(beta), P(cs)))
    ar.check()
    report("wgrad_ln_fix %d x %d" % (rows, cols), RB.fix_check(inp["G"], inp["gamma"], inp["beta"], inp["colsum"], G.host(), raise_on_fail=False))


# ---------------------------------------------------------------------------------------------------------------- cross-entropy
@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("rows,V,ldz,off", [c[:4] for c in XENT])
def test_softmax_xent_within_bounds(lib, dtype, rows, V, ldz, off):
    z, y, _ = RB.xent_inputs(rows, V, seed=rows + V + ldz)
    inv_n = 1.0 / rows
    ar = Arena("cuda", 2 * rows * ldz * 4 + (1 << 20))
    if off:
        # the logits start `off` floats inside their window: a pointer that is not 16-byte aligned
        flat = torch.full((rows * ldz + off,), float("nan"))
        flat[off:].view(rows, ldz)[:, :V] = T(z)
        zs = ar.operand(flat, F32, 1, flat.numel(), flat.numel(), name="logits")
        zp = C.c_void_p(zs.ptr() + 4 * off)
    else:
        zs = ar.operand(T(z), F32, rows, V, ldz, name="logits")
        zp = P(zs)
    ys = ar.operand(T(y), I32, 1, rows, rows, name="labels")
    dz = ar.output(tdt(dtype), rows, V, ldz, name="dlogits", pad_zero=True)
    rl, rc = ar.output(F32, 1, rows, rows, name="row_loss"), ar.output(I32, 1, rows, rows, name="row_correct")
    ar.arm()
    ck(lib, lib.cmp_k_softmax_xent(stream(), zp, ldz, P(ys), P(dz), P(rl), P(rc), rows, V, inv_n, dtype))
    ar.check()
    report("xent %s rows %d V %d ldz %d off %d" % ("bf16" if dtype else "fp32", rows, V, ldz, off),
           RB.xent_check(dtype, z, y, inv_n, dz.t.detach().cpu(), rl.host().reshape(-1), rc.host().reshape(-1), V, raise_on_fail=False))
