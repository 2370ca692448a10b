"""Persistent GEMM items: case tables, planted inputs, float64 references and per-element limits for the kernels of gemm.hip whose
workgroups run SEVERAL items (gemm_bf16_256_kernel with its eleven compile-time forms, the two deep-pipeline p4 kernels).
Shared by tests/test_gpu_gemm_items.py (the launches) and tests/test_gemm_items_checks_host.py (plans, references, planted faults on
the CPU).  The pattern of tests/row_bounds.py and tests/kernel_arena.py, whose pieces it reuses.  numpy and torch on the CPU only.

A persistent workgroup takes item blockIdx.x, then item + gridDim.x (static) or what it claims from its XCD group's counter
(dynamic); between two items the next item's first k-slab, the fold kinds' statistics / bias / column-sum image, the EpiPre operand
chunks, the LDS words lstat / lrow and the column-sum atomics all change hands.  The grid is min(items, cap): with the one-shot
cmp_gemm_grid_next(cap, rev) a launch of 14 to 64 items runs on 6 to 24 workgroups, three items or more in some of them.

Every limit is  min(SEQ_MARGIN x q, analytic multiple of 2^-24) x S  (+ 2^-8 |reference| for a bf16 store), q the error of a plain
fp32 numpy emulation of the SAME formula against float64 relative to the magnitude sum S, measured on the CPU.  Nothing is
calibrated on what a kernel returns.  References are float64 evaluations of the epilogue's own formula on exactly what the kernel
is handed: the bf16 rows as stored, the fp32 partials, cs and bias' as stored, the weight as rounded.

  lnm 0 kinds (plain, bias, GELU + aux, GELU', residual with / without bias, dropout): the bounds of test_gpu_kernel_guards.gemm_case,
      unchanged (`reference`): f x S with f = acc_factor(q_seq, K), S = |a|.|b| + |bias| + |resid|.
  fold (EPI_PLAIN / EPI_GELU_AUX / EPI_PLAIN32 at lnm 1):  ref_ij = rs_i (x.WT^T)_ij - rs_i mu_i cs_j + b'_j, (mu, rs) merged in float64
      from the handed partials (RB.merge_ref).  Limit, four parts:
        rs_i f S_ij                                       accumulation (f as above, S = |x|.|WT|^T)
        |drs_i| |acc_ij - mu_i cs_j| + rs_i |dmu_i| |cs_j|     the merge error of (mu, rs) through the formula; dmu, drs are RB's merge
                                                          limits (f32_limits of merge_emulation against merge_ref)
        min(SEQ_MARGIN q_eval, 4 x 2^-24) T_ij            fp32 evaluation, T = rs |acc| + rs |mu| |cs| + |b'|; q_eval from `fold_eval32`;
                                                          4: the product mu rs, the inner and the outer fma, one to spare
        2^-8 |ref|                                        bf16 store (not EPI_PLAIN32)
      GELU kind: aux to the same limit, the activation to 1.13 x it + the gelu allowance, as gemm_case does.
  statistics out (lnm 2, 3): reference RB.parts_of(the rows as STORED).  mean: min(SEQ_MARGIN q, 12 x 2^-24) A with A the segment's
      mean |value|; M2: min(SEQ_MARGIN q, 32 x 2^-24) (M2 + 2 sqrt(256 M2) A) -- d = f - mean carries the mean's error A u into every
      d^2, sum |d| <= sqrt(256 M2).  q from `stats_out_emulation`, the kernel's tree: 8 columns, three equal-count Chan steps, the
      four-way fold with 64 sum d^2.  12 and 32 count the roundings along that tree (7 + 3 + 2; 8 + 3 x 4 + 6 + the mean's share).
  rebuilt residual (lnm 3): the residual term is t = bf16(LN(raw row)) with the kernel's single rounding; the residual-kind limit with
      |t| in S, plus one bf16 ulp of t (2^-7 |t|: a 1-ulp difference of the fp32 LayerNorm can flip the rounding).
  scale kinds (lnm 5): GELU': C = rs o (acc gelu'(aux)), limit rs (f S |g'| + |acc| allowance) + |drs| |acc g'| + 2 x 2^-24 |ref|;
      residual: C = acc + rs o resid, limit f (S + rs |resid|) + |drs| |resid| + 2 x 2^-24 |ref|.  The fused column sums of the GELU'
      scale kind are those of the UNSCALED product and are held, per column, to colsum_bound on the float64 product.  Everywhere else
      the fused column sums are sums of the stored output and are held to colsum_bound on the stored output.
  split-K (atomics): the bound of test_gemm_split_k_guarded, f (S + |c0|).

Inputs.  LayerNorm rows are of RB.LN_KINDS (row r of kind r mod 8: off24 and off300 with |mean| >> sigma, where the fold subtracts two
large terms; a constant row; a constant row in place of the zero row, zero in tile 0 only), per-segment offsets of +-1.5 sigma, a per-row
scale in [1/2, 2] (the constant rows keep theirs at 1), and -- the point of these cases -- every 256-row tile its own offset and scale (`TILE_OFF`, `TILE_SCALE`): an
epilogue that used the previous item's statistics, bias image or operand chunk lands far outside the limit
(tests/test_gemm_items_checks_host.py: swapping the statistics of two tiles moves some element of every affected row by ten limits).
bias' and cs differ per 256-column tile in the same way; output rows carry per-64-column and per-256-column offsets (`col_pattern`: +-3, +-4)
so that the between-part terms of both statistics merges are at least RB.SEG_SHARE_MIN of a row's M2 (asserted where used).
"""
import ctypes as C

import numpy as np
import torch

import kernel_arena as KA
import row_bounds as RB
import test_gpu_kernel_guards as G
from kernel_arena import Arena, EPS24, BF16_OUT, SEQ_MARGIN
from oracle import transformer_oracle as O

FP32, BF16 = 0, 1
F32, BF = torch.float32, torch.bfloat16
f32 = np.float32
EPS = RB.EPS
M_ROWS = 1792                              # 7 tile rows
SEED, STREAM = 21, 9                       # dropout
F32K, GENERIC, TILE128, RING, TILE256, P4_256, P4_128 = range(7)                    # CMP_GEMM_FAM_*
EPI_GENERIC, EPI_PLAIN, EPI_GELU_AUX, EPI_RESID, EPI_GELUGRAD, EPI_PLAIN32 = range(6)
TILE_OFF = (0.0, -2.0, 4.0, -6.0, 8.0, -10.0, 12.0, -14.0)
TILE_SCALE = (1.0, 1.5, 0.75)
EVAL_CAP, MEAN_CAP, M2_CAP = 4.0, 12.0, 32.0
A64 = RB.A64


# ================================================================================================================ case tables
def _case(table, name, kind, flags, M, N, K, cap, ta=0, tb=1, lnm=0, np_=1, p=0.0, colsum=False, splitk=1, mode=None, want=None, revs=(0,)):
    return dict(id="%s-%s" % (table, name), table=table, kind=kind, flags=flags, M=M, N=N, K=K, cap=cap, ta=ta, tb=tb, lnm=lnm, np=np_, p=p,
                colsum=colsum, splitk=splitk, mode=mode, want=want, revs=revs)


def cap_for(items):
    """8 unless 8 cannot give a workgroup three items with uneven counts: 14 items take 6 workgroups, 24 take 9, 32 take 12 (the
    128x256 deep pipeline launches two workgroups per capped CU: 42 items on 16, 64 on 24)."""
    return {14: 6, 24: 9, 32: 12, 64: 12}.get(items, 8)


def _tables():
    cs = []
    M = M_ROWS
    R = (0, 1)
    # Table A: gemm_bf16_256_kernel, flags 8, ta = 0, tb = 1 -- every row of the dispatch switch
    for K in (64, 320, 512):           # 1, 5, 8 k-steps
        for kind, ek, colsum in (("bias", EPI_PLAIN, False), ("none", EPI_PLAIN, False), ("gelu", EPI_GELU_AUX, False),
                                 ("gelugrad", EPI_GELUGRAD, False), ("gelugrad", EPI_GELUGRAD, True), ("resid", EPI_RESID, False),
                                 ("resid-nobias", EPI_RESID, False), ("drop", EPI_RESID, False)):
            cs.append(_case("A", "%s%s-K%d" % (kind, "+sums" if colsum else "", K), kind, 8, M, 768, K, 8, colsum=colsum,
                            p=0.25 if kind == "drop" else 0.0, want=(TILE256, ek, 0, 1), revs=R))
    for n in (2, 3):
        cs.append(_case("A", "fold-np%d" % n, "fold", 8, M, 768, 256 * n, 8, lnm=1, np_=n, want=(TILE256, EPI_PLAIN, 1, n), revs=R))
        cs.append(_case("A", "fold-gelu-np%d" % n, "fold-gelu", 8, M, 768, 256 * n, 8, lnm=1, np_=n, want=(TILE256, EPI_GELU_AUX, 1, n), revs=R))
        cs.append(_case("A", "fold32-np%d" % n, "fold32", 8, M, 648, 256 * n, 8, lnm=1, np_=n, want=(TILE256, EPI_PLAIN32, 1, n), revs=R))
        for p in (0.0, 0.1):
            cs.append(_case("A", "stats-N%d-p%g" % (256 * n, p), "stats", 8, M, 256 * n, 320, cap_for(7 * n), lnm=2, np_=1, p=p,
                            want=(TILE256, EPI_RESID, 2, 1), revs=R))
            cs.append(_case("A", "rebuild-np%d-p%g" % (n, p), "rebuild", 8, M, 256 * n, 320, cap_for(7 * n), lnm=3, np_=n, p=p,
                            want=(TILE256, EPI_RESID, 3, n), revs=R))
        for K in (64, 320):
            cs.append(_case("A", "scale-gelugrad-np%d-K%d" % (n, K), "scale-gelugrad", 8, M, 768, K, 8, lnm=5, np_=n, colsum=True,
                            want=(TILE256, EPI_GELUGRAD, 5, n), revs=R))
            cs.append(_case("A", "scale-resid-np%d-K%d" % (n, K), "scale-resid", 8, M, 768, K, 8, lnm=5, np_=n,
                            want=(TILE256, EPI_RESID, 5, n), revs=R))
    # Table B: the same kernel's run-time epilogue and split-K items
    cs.append(_case("B", "ragged-drop", "drop-noresid", 8, 1800, 520, 320, cap_for(24), p=0.25, want=(TILE256, EPI_GENERIC, 0, 1)))
    cs.append(_case("B", "f32", "f32", 8, M, 768, 320, 8, want=(TILE256, EPI_GENERIC, 0, 1)))
    # (the 256x256 kernel has no slab form: all three modes plan as float atomics there -- one code path, asked for in the three ways
    #  test_gemm_split_k_guarded asks, none of them compared bitwise; the slab form is the deep pipeline's, Table C)
    for mode in G.SPLIT_K_MODES:
        cs.append(_case("B", "wgrad-%s" % mode, "wgrad", 8, 512, 512, 2048, cap_for(32), ta=1, tb=0, splitk=8, mode=mode,
                        want=(TILE256, EPI_GENERIC, 0, 1)))
    # Table C: the deep pipeline, forward layout (ta = 0, tb = 0); 1, 3, 16 k-steps of 32 against the three- and four-stage rings
    for flags, fam, nm in ((16, P4_256, "p4-256"), (48, P4_128, "p4-128")):
        for K in (32, 96, 512):
            for kind, ek in (("bias", EPI_PLAIN), ("gelu", EPI_GELU_AUX), ("resid", EPI_RESID)):
                cs.append(_case("C", "%s-%s-K%d" % (nm, kind, K), kind, flags, M, 768, K, 8, ta=0, tb=0, want=(fam, ek, 0, 1)))
        cs.append(_case("C", "%s-wgrad" % nm, "wgrad", flags, 512, 512, 2048, cap_for(32 if flags == 16 else 64), ta=1, tb=0, splitk=8,
                        mode="slab", want=(fam, EPI_GENERIC, 0, 1)))
    return cs


def caps_of(case):
    """The caps a case is launched at: its own; where that is 8 also 6 -- at 8 a workgroup's items w, w + 8, ... belong to one XCD group,
    which item_coords maps to consecutive tiles, so almost every transition stays inside one tile row; 6 mixes the groups and most
    transitions change the tile row (and the statistics) -- then 24 and none."""
    return (case["cap"], 6, 24, 0) if case["cap"] == 8 else (case["cap"], 24, 0)


def row_changes(case, cap, rev=0):
    """(transitions between consecutive items of a workgroup that change the tile row, all transitions) under static striding on the
    capped grid; cases without split-K."""
    bm = 128 if case["flags"] == 48 else 256
    tiles_n = -(-case["N"] // 256)
    ntiles = tiles_n * (-(-case["M"] // bm))
    grid = cap * (2 if case["flags"] == 48 else 1)
    ch = n = 0
    for items in static_walk(ntiles, grid):
        rows = [item_tile(i, ntiles, ntiles, rev)[1] // tiles_n for i in items]
        ch += sum(a != b for a, b in zip(rows, rows[1:]))
        n += len(rows) - 1
    return ch, n


CASES = _tables()
CASE_IDS = [c["id"] for c in CASES]
ITEM_MODES = ("static", "dynamic")


def kz_of(case):
    """K-contiguous operands of the forward-layout deep-pipeline rows with K % 64 != 0 ride on zero padding (CMP_GEMM_KPAD_ZERO)."""
    return int(case["K"] % 64 != 0 and not (case["ta"] and not case["tb"]))


# ================================================================================================================ inputs
def col_pattern(N):
    """+-3 per 64 columns and +-4 per 256 columns: the between-part terms of the producer's four-way fold (64 d^2) and of the
    consumer's segment merge (256 d^2) are each more than SEG_SHARE_MIN of a unit-variance row's M2."""
    j = np.arange(N)
    return 3.0 * (-1.0) ** (j // 64) + 4.0 * (-1.0) ** (j // 256)


def ln_rows(M, E, seed):
    """[M, E] LayerNorm input rows as stored in bf16 (float32 values) and their kinds; see the module docstring."""
    rng = np.random.default_rng(seed)
    r = np.arange(M)
    kinds = np.array([RB.LN_KINDS[i % len(RB.LN_KINDS)] for i in r])
    x = rng.normal(0.0, 1.0, (M, E)) + np.repeat(1.5 * (-1.0) ** np.arange(E // 256), 256)[None, :]
    for kind, off in (("off0.5", 0.5), ("off24", 24.0), ("off300", 300.0)):
        x[kinds == kind] += off
    x[kinds == "const"] = 3.25
    x[kinds == "zero"] = 0.0
    orow = np.flatnonzero(kinds == "outlier")
    x[orow, (7 * orow + 3) % E] = 200.0
    row_scale = 2.0 ** rng.uniform(-1.0, 1.0, M)
    row_scale[np.isin(kinds, ("const", "zero"))] = 1.0       # (scaled, the constants of two tiles can round to the same bf16 value)
    t = r // 256
    x = x * (row_scale * np.take(TILE_SCALE, t % len(TILE_SCALE)))[:, None] + np.take(TILE_OFF, t % len(TILE_OFF))[:, None]
    return RB.store(x, BF16), kinds


def stored_part(x):
    """The partial statistics a producer would have left for the rows x: float32 [M, E / 256, 2]."""
    return RB.parts_of(x).astype(f32)


def _bf(a):
    return RB.store(np.asarray(a, dtype=f32), BF16).astype(np.float64)


_OPS = {}
OPS_KEPT = 8


def _acc(a, b, K):
    """float64 product, S and the accumulation factor of a [M, K] . b [K, N] (numpy float64 values as rounded)."""
    q, ref, S = KA.q_seq_of(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))
    return ref.numpy(), S.numpy(), KA.acc_factor(q, K)


def operands(case):
    """Host operands of a case (float64 values as stored unless named otherwise), the float64 product `ref`, `S`, `f`; cached per
    (input class, M, N, K, np) and shared by every stride regime, walk and kind that can."""
    kind, M, N, K, n = case["kind"], case["M"], case["N"], case["K"], case["np"]
    cls = "fold" if kind.startswith("fold") else kind if kind in ("stats", "rebuild") else "scale" if kind.startswith("scale") else "plain"
    key = (cls, M, N, K, n if cls != "plain" else 0)
    if key in _OPS:
        _OPS[key] = _OPS.pop(key)                                    # (most recently used last)
        return _OPS[key]
    while len(_OPS) >= OPS_KEPT:                                     # a few shapes at a time: a session holds no operand set it is done with
        old = next(iter(_OPS))
        G._OPS.pop((BF16, old[1], old[2], old[3]), None)
        del _OPS[old]
    if cls == "plain":
        o = G.logical_ops(BF16, M, N, K)
        _OPS[key] = dict(cls=cls, a=o["a"].numpy(), b=o["b"].numpy(), ref=o["ref"].numpy(), S=o["S"].numpy(), f=o["f"], bias=o["bias"].numpy(),
                         resid=o["resid"].numpy(), pre=o["pre"].numpy(), c0=o["c0"].numpy(), torch_ops=o)
        return _OPS[key]
    rng = np.random.default_rng(1000 * n + N + K)
    d = dict(cls=cls)
    ct = np.arange(-(-N // 256) * 256) // 256                        # column tile of every (padded) column
    if cls == "fold":
        x, kinds = ln_rows(M, K, seed=K + N)
        gamma = 1 + 0.3 * rng.normal(size=K)
        wt_exact = rng.normal(0, 0.05, (N, K)) * gamma[None, :] + 0.004 * ((ct[:N] % 3) - 1)[:, None]
        wt = _bf(wt_exact)                                           # [N, K] as the kernel reads it
        npad = ct.size
        cs = np.zeros(npad); cs[:N] = wt.sum(1)
        bias = np.zeros(npad); bias[:N] = rng.normal(0, 0.1, N) + 0.7 * ct[:N]
        d.update(a=x.astype(np.float64), b=wt.T.copy(), kinds=kinds, part=stored_part(x), cs=cs.astype(f32).astype(np.float64),
                 bias=bias.astype(f32).astype(np.float64), cs_unrounded=wt_exact.sum(1))
    else:
        a = _bf(rng.normal(0, 1.0, (M, K)))
        w = _bf(rng.normal(0, 0.05, (N, K)))
        d.update(a=a, b=w.T.copy(), bias=rng.normal(0, 0.1, N).astype(f32).astype(np.float64) + 0.0)
        if cls == "stats":
            d.update(resid=_bf(rng.normal(0.5, 1.0, (M, N)) * 2.0 ** rng.uniform(-1, 1, (M, 1)) + col_pattern(N)[None, :]))
        elif cls == "rebuild":
            raw, kinds = ln_rows(M, N, seed=N + 7)
            d.update(resid=raw.astype(np.float64), kinds=kinds, part=stored_part(raw), gamma=(1 + 0.3 * rng.normal(size=N)).astype(f32).astype(np.float64),
                     beta=(rng.normal(0, 0.2, N) + col_pattern(N)).astype(f32).astype(np.float64))
        else:
            rows, kinds = ln_rows(M, 256 * n, seed=n + 3)
            d.update(kinds=kinds, part=stored_part(rows), pre=_bf(rng.normal(0, 1.5, (M, N))), resid=_bf(rng.normal(0, 1.0, (M, N))))
    d["ref"], d["S"], d["f"] = _acc(d["a"], d["b"], K)
    _OPS[key] = d
    return d


def merged(part):
    """(mu, rs) of the handed partials merged in float64, and RB's merge limits (dmu, drs) -- all [M, 1]."""
    ref, emu = RB.merge_ref(part, EPS), RB.merge_emulation(part, EPS)
    dmu, _ = RB.f32_limits(emu["mean"], ref["mean"], np.abs(A64(part)[:, :, 0]).mean(-1))
    drs, _ = RB.f32_limits(emu["rstd"], ref["rstd"], ref["rstd"])
    return ref["mean"][:, None], ref["rstd"][:, None], dmu[:, None], drs[:, None], ref["share"]


# ================================================================================================================ references and limits
def fold_eval32(acc, mu, rs, cs, b):
    """The fold epilogue's formula in plain float32 on float32 arguments."""
    acc, mu, rs, cs, b = (np.asarray(v, dtype=f32) for v in (acc, mu, rs, cs, b))
    return rs * acc + (-(mu * rs) * cs + b)


def fold_reference(o, N, stats=None, cs=None, bias=None):
    """(ref, lim in front of the store) of the fold kinds on the operands o; stats / cs / bias: replacements (planted faults)."""
    mu, rs, dmu, drs, _ = merged(o["part"])
    if stats is not None:
        mu, rs = stats
    cs = (o["cs"] if cs is None else cs)[None, :N]
    b = (o["bias"] if bias is None else bias)[None, :N]
    acc, S = o["ref"], o["S"]
    ref = rs * acc - rs * mu * cs + b
    T = rs * np.abs(acc) + rs * np.abs(mu) * np.abs(cs) + np.abs(b)
    q = RB._q(fold_eval32(acc, mu, rs, cs, b), ref, T)
    lim = rs * o["f"] * S + drs * np.abs(acc - mu * cs) + rs * dmu * np.abs(cs) + min(SEQ_MARGIN * q, EVAL_CAP * EPS24) * T
    return ref, lim


def stats_out_emulation(x):
    """The producer's statistics tree in float32 on the stored rows x [M, N]: per lane 8 columns (sum, mean, sum of d^2), three
    equal-count Chan steps over the 8 lanes of a row, the four wave columns folded with 64 sum d^2 -> [M, N / 256, 2]."""
    x = np.asarray(x, dtype=f32)
    M, N = x.shape
    v = x.reshape(M, N // 256, 4, 8, 8)
    mn = RB.seq_sum32(v) * f32(0.125)
    d = v - mn[..., None]
    q = RB.seq_sum32(d * d)
    for cnt in (4.0, 8.0, 16.0):
        a, b, qa, qb = mn[..., 0::2], mn[..., 1::2], q[..., 0::2], q[..., 1::2]
        dd = b - a
        mn, q = f32(0.5) * (a + b), (qa + qb) + dd * dd * f32(cnt)
    mn, q = mn[..., 0], q[..., 0]                                     # [M, T, 4]
    mu = f32(0.25) * ((mn[..., 0] + mn[..., 1]) + (mn[..., 2] + mn[..., 3]))
    dd = mn - mu[..., None]
    m2 = ((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])) + f32(64.0) * ((dd[..., 0] ** 2 + dd[..., 1] ** 2) + (dd[..., 2] ** 2 + dd[..., 3] ** 2))
    return np.stack([mu, m2], -1)


def stats_out_limits(stored):
    """Reference [M, N / 256, 2] of the stored rows, the limits of the mean and of M2, and the share of the four-way fold's between-part
    term 64 sum d^2 in every M2."""
    ref = RB.parts_of(stored)
    emu = stats_out_emulation(stored).astype(np.float64)
    x = A64(stored)
    seg = x.reshape(x.shape[0], x.shape[1] // 256, 256)
    Asz = np.abs(seg).mean(-1)
    Sm2 = ref[..., 1] + 2.0 * np.sqrt(256.0 * ref[..., 1]) * Asz
    qm, q2 = RB._q(emu[..., 0], ref[..., 0], Asz), RB._q(emu[..., 1], ref[..., 1], Sm2)
    sub = seg.reshape(seg.shape[0], seg.shape[1], 4, 64).mean(-1)
    share = 64.0 * ((sub - ref[..., 0:1]) ** 2).sum(-1) / np.maximum(ref[..., 1], 1e-300)
    return ref, min(SEQ_MARGIN * qm, MEAN_CAP * EPS24) * Asz, min(SEQ_MARGIN * q2, M2_CAP * EPS24) * Sm2, share


def keep_of(case):
    M, N, p = case["M"], case["N"], case["p"]
    return O.dropout_keep_rows(case.get("seed", SEED), case.get("stream", STREAM), M, N, p) if p > 0 else np.ones((M, N), dtype=bool)


def reference(case, o):
    """name -> (float64 reference, limit in front of the store, bf16 store?) for every output of the case that has a fixed reference
    (C, aux); the statistics and the column sums are taken from what was stored (`check_outputs`)."""
    kind, M, N, K, p = case["kind"], case["M"], case["N"], case["K"], case["p"]
    ref, S, f = o["ref"], o["S"], o["f"]
    out = {}
    if kind in ("fold", "fold-gelu", "fold32"):
        r, lim = fold_reference(o, N)
        if kind == "fold-gelu":
            out["aux"] = (r, lim, True)
            out["C"] = (O.gelu(r), 1.13 * lim + KA.f32_eval_allowance(O.gelu, r), True)
        else:
            out["C"] = (r, lim, kind != "fold32")
        return out
    bb = o["bias"][None, :N] if "bias" in o else 0.0
    if kind in ("none", "f32"):
        out["C"] = (ref, f * S, kind != "f32")
    elif kind == "bias":
        out["C"] = (ref + bb, f * (S + np.abs(bb)), True)
    elif kind == "gelu":
        pre, acc = ref + bb, f * (S + np.abs(bb))
        out["aux"] = (pre, acc, True)
        out["C"] = (O.gelu(pre), 1.13 * acc + KA.f32_eval_allowance(O.gelu, pre), True)
    elif kind == "gelugrad":
        gg = O.gelu_grad(o["pre"])
        out["C"] = (ref * gg, f * S * np.abs(gg) + np.abs(ref) * KA.f32_eval_allowance(O.gelu_grad, o["pre"]), True)
    elif kind == "resid":
        out["C"] = (ref + bb + o["resid"], f * (S + np.abs(bb) + np.abs(o["resid"])), True)
    elif kind == "resid-nobias":
        out["C"] = (ref + o["resid"], f * (S + np.abs(o["resid"])), True)
    elif kind in ("drop", "drop-noresid", "stats"):
        scale = keep_of(case) / (1.0 - p)
        res = o["resid"] if kind != "drop-noresid" else 0.0
        out["C"] = ((ref + bb) * scale + res, f * ((S + np.abs(bb)) * scale + np.abs(res)), True)
    elif kind == "rebuild":
        mu, rs, dmu, drs, _ = merged(o["part"])
        x, g, be = o["resid"], o["gamma"][None, :], o["beta"][None, :]
        t64 = (x - mu) * rs * g + be
        t = _bf(t64)
        scale = keep_of(case) / (1.0 - p)
        out["C"] = ((ref + bb) * scale + t, f * ((S + np.abs(bb)) * scale + np.abs(t)) + 2.0 ** -7 * np.abs(t), True)
    elif kind == "scale-gelugrad":
        mu, rs, dmu, drs, _ = merged(o["part"])
        gg = O.gelu_grad(o["pre"])
        prod = ref * gg
        plim = f * S * np.abs(gg) + np.abs(ref) * KA.f32_eval_allowance(O.gelu_grad, o["pre"])
        out["C"] = (rs * prod, rs * plim + drs * np.abs(prod) + 2 * EPS24 * np.abs(rs * prod), True)
        out["_prod"] = (prod, plim, False)
    elif kind == "scale-resid":
        mu, rs, dmu, drs, _ = merged(o["part"])
        r = ref + rs * o["resid"]
        out["C"] = (r, f * (S + rs * np.abs(o["resid"])) + drs * np.abs(o["resid"]) + 2 * EPS24 * np.abs(r), True)
    elif kind == "wgrad":
        out["C"] = (ref + o["c0"], f * (S + np.abs(o["c0"])), False)
    else:
        raise KeyError(kind)
    return out


_REF = {}


def reference_cached(case, o):
    key = (case["kind"], case["M"], case["N"], case["K"], case["np"], case["p"])
    if key not in _REF:
        _REF.clear()                             # the rows of a case follow each other: one set of references and limits at a time
        _REF[key] = reference(case, o)
    return _REF[key]


def _within(what, name, got, ref, lim, bf16_out, worst):
    lim = np.asarray(lim) + (BF16_OUT * np.abs(ref) if bf16_out else 0.0)
    worst[name] = max(worst.get(name, 0.0), RB.within(what, name, got, ref, lim))


def adhoc(kind, a, b, lnm=0, np_=1, p=0.0, seed=SEED, stream=STREAM, colsum=False, **arrays):
    """(case, operands) for arrays that are not a table row (tests/test_gpu_ln_fused.py holds its own launches to the same limits):
    a [M, K], b [K, N] float64 as stored; arrays: part, cs, bias, resid, pre, gamma, beta as the kind needs them."""
    a, b = A64(a), A64(b)
    o = dict(arrays, a=a, b=b, adhoc=True)
    o["ref"], o["S"], o["f"] = _acc(a, b, a.shape[1])
    case = dict(id="adhoc-" + kind, kind=kind, M=a.shape[0], N=b.shape[1], K=a.shape[1], np=np_, p=p, seed=seed, stream=stream, lnm=lnm,
                colsum=colsum)
    return case, o


def check_outputs(case, o, outs, what=None, colsum_start=None, sums_only=False):
    """Every output of one launch (outs: name -> array as stored, widened) against its reference and limit -> {name: worst error / limit}.
    Raises AssertionError("<what>: <output name>, element ...") on the first element outside its limit.  sums_only: the column sums
    alone (a launch whose other outputs are bitwise those of a launch already checked)."""
    what = what or case["id"]
    worst = {}
    refs = reference(case, o) if o.get("adhoc") else reference_cached(case, o)
    kind, N, p = case["kind"], case["N"], (0.0 if sums_only else case["p"])
    for name in ("aux", "C"):
        if name in refs and not sums_only:
            ref, lim, bf = refs[name]
            _within(what, name, outs[name], ref, lim, bf, worst)
    if p > 0 and kind != "rebuild":          # (a dropped element of the rebuild kind is the rebuilt term alone: inside the limit above)
        keep = keep_of(case)
        want = A64(o["resid"])[~keep] if kind in ("drop", "stats") else 0.0
        assert np.array_equal(A64(outs["C"])[~keep], want + np.zeros(int((~keep).sum()))), "%s: C, a dropped element is not exactly the residual" % what
    if case["lnm"] & 2 and not sums_only:
        stored = A64(outs["C"])
        pref, lmean, lm2, share = stats_out_limits(stored)
        if not o.get("adhoc"):               # (the table rows plant the offsets; a caller's own rows need not)
            assert share.min() >= RB.SEG_SHARE_MIN, "%s: the planted 64-column offsets carry only %.2f of some M2" % (what, share.min())
            assert RB.merge_ref(pref)["share"].min() >= RB.SEG_SHARE_MIN, "%s: the planted 256-column offsets are too small" % what
        part = A64(outs["part"]).reshape(pref.shape)
        worst["part_mean"] = RB.within(what, "part_mean", part[..., 0], pref[..., 0], lmean)
        worst["part_m2"] = RB.within(what, "part_m2", part[..., 1], pref[..., 1], lm2)
    if case["colsum"]:
        start = torch.from_numpy(A64(colsum_start))
        if kind == "scale-gelugrad":
            cref, cS, cf = KA.colsum_bound(torch.from_numpy(refs["_prod"][0]), start)
            lim = cf * cS.numpy()
        else:
            cref, cS, cf = KA.colsum_bound(torch.from_numpy(A64(outs["C"])), start)
            lim = cf * cS.numpy()
        worst["colsum"] = RB.within(what, "colsum", outs["colsum"], cref.numpy(), lim)
    return worst


# ================================================================================================================ staging and arming
class Staged:
    pass


def P(slot):
    return C.c_void_p(slot.ptr()) if slot is not None else None


def colsum_start(N):
    return np.random.default_rng(N).normal(0, 1.0, N).astype(f32)


def stage(case, o, padded, device="cuda"):
    """The arena of one launch: every operand a guarded window, every leading dimension 8 or 16 elements wider than the row when
    `padded`.  -> Staged(ar, slots, args: the cmp_k_gemm argument list behind the stream, ln: the arming call or None)."""
    kind, M, N, K, n, p = case["kind"], case["M"], case["N"], case["K"], case["np"], case["p"]
    ta, tb, flags = case["ta"], case["tb"], case["flags"]
    pa, pb, pc, pu, pr = (8, 16, 16, 8, 8) if padded else (0, 0, 0, 0, 0)
    st = Staged()
    ar = st.ar = Arena(device, 20 << 20)
    T = torch.from_numpy
    kz = kz_of(case)
    A, B = G.stage_ab(ar, BF16, ta, tb, M, N, K, kz, pa, pb, dict(a=T(o["a"]), b=T(o["b"])))
    out_f32 = kind in ("f32", "fold32", "wgrad")
    s = st.slots = dict(A=A, B=B)
    if kind == "wgrad":
        s["C"] = ar.accumulator(T(o["c0"]), F32, M, N, N + pc, name="C")
        s["ws"] = ar.scratch(case["splitk"] * M * N * 4, name="slab workspace")
    else:
        s["C"] = ar.output(F32 if out_f32 else BF, M, N, N + pc, name="C")
    bias = aux = resid = None
    act = 0
    if kind in ("bias", "gelu", "resid", "drop", "drop-noresid", "stats", "rebuild", "fold", "fold-gelu", "fold32"):
        bias = s["bias"] = ar.vector(T(o["bias"]), F32, name="bias")
    if kind in ("gelu", "fold-gelu"):
        aux = s["aux"] = ar.output(BF, M, N, N + pu, name="aux")
        act = 1
    if kind in ("gelugrad", "scale-gelugrad"):
        aux = s["aux_in"] = ar.operand(T(o["pre"]), BF, M, N, N + pu, name="aux")
        act = 2
    if kind in ("resid", "resid-nobias", "drop", "stats", "rebuild", "scale-resid"):
        resid = s["resid"] = ar.operand(T(o["resid"]), BF, M, N, N + pr, name="resid")
    st.ln = None
    if case["lnm"]:
        part = cs = gamma = beta = outp = None
        if case["lnm"] & 1:
            pw = o["part"].shape[1] * 2
            part = s["part_in"] = ar.operand(T(o["part"].reshape(M, pw)), F32, M, pw, pw, name="in_part")
        if kind.startswith("fold"):
            cs = s["cs"] = ar.vector(T(o["cs"]), F32, name="cs")
        if kind == "rebuild":
            gamma, beta = ar.vector(T(o["gamma"]), F32, name="gamma"), ar.vector(T(o["beta"]), F32, name="beta")
        if case["lnm"] & 2:
            w = (N // 256) * 2
            outp = s["part"] = ar.output(F32, M, w, w, name="out_part")
        st.ln = ("scale", (P(part), n, EPS)) if case["lnm"] == 5 else ("ln", (P(part), n if case["lnm"] & 1 else 0, EPS, P(cs), P(gamma), P(beta), P(outp)))
    if case["colsum"]:
        s["colsum"] = ar.vector(T(colsum_start(N)), F32, name="colsum", kind="acc")
    fl = flags | kz | (128 if case["mode"] == "atomic" else 0)
    st.args = G.gemm_args(BF16, ta, tb, M, N, K, A, B, s["C"], bias=bias, act=act, aux=aux, resid=resid, out_fp32=int(out_f32),
                          splitk=case["splitk"], p=p, seed=SEED, rng=STREAM, flags=fl)
    return st


def arm(lib, case, st, cap, rev):
    """The one-shot calls in front of cmp_k_gemm / cmp_gemm_plan."""
    def ck(rc):
        assert rc == 0, lib.cmp_last_error().decode()
    if case["kind"] == "wgrad":
        ws = st.slots["ws"]
        use = case["mode"] != "none"
        ck(lib.cmp_gemm_set_workspace(P(ws) if use else None, ws.nbytes if use else 0))
    if st.ln is not None:
        ck((lib.cmp_gemm_ln_scale_next if st.ln[0] == "scale" else lib.cmp_gemm_ln_next)(*st.ln[1]))
    if case["colsum"]:
        ck(lib.cmp_gemm_colsum_next(P(st.slots["colsum"])))
    ck(lib.cmp_gemm_grid_next(cap, rev))


def outputs_of(case, st):
    s = st.slots
    outs = {"C": s["C"].host().double().numpy()}
    for name in ("aux", "part", "colsum"):
        if name in s:
            outs[name] = s[name].host().double().numpy()
    if "colsum" in outs:
        outs["colsum"] = outs["colsum"].reshape(-1)
    return outs


# ================================================================================================================ the walk, and fakes
def item_tile(item, nitems, ntiles, rev):
    """gemm.hip: item_coords -> (split, tile) of an item."""
    q, r, x = nitems >> 3, nitems & 7, item & 7
    idx = (q + (1 if x < r else 0)) - 1 - (item >> 3) if rev else (item >> 3)
    lin = (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + idx
    return lin // ntiles, lin % ntiles


def static_walk(nitems, grid):
    """Per workgroup the items it runs under static striding."""
    return [list(range(w, nitems, grid)) for w in range(min(grid, nitems))]


def fake_launch(case, o, grid, rev, bug=None):
    """An item-structured numpy statement of a launch of the 256x256 kernel on `grid` workgroups: every workgroup walks its items in
    the kernel's order, each item's epilogue is the CORRECT fp32 formula on the item's own tile (accumulators = the float64 product
    rounded to fp32) -- or wrong in the way `bug` names, which involves the PREVIOUS item of the same workgroup.  -> outs as
    `outputs_of` returns them (elements never written are NaN)."""
    kind, M, N, K, p = case["kind"], case["M"], case["N"], case["K"], case["p"]
    tiles_n = -(-N // 256)
    Mp = -(-M // 256) * 256
    ntiles = tiles_n * (Mp // 256)
    nitems = ntiles
    acc = o["ref"].astype(f32)
    Cw = np.full((Mp, tiles_n * 256), np.nan)
    aux = np.full((Mp, tiles_n * 256), np.nan) if kind in ("gelu", "fold-gelu") else None
    part = np.full((M, tiles_n, 2), np.nan) if case["lnm"] & 2 else None
    colsum = colsum_start(N).copy() if case["colsum"] else None
    keep = keep_of(case) if p > 0 else None
    if case["lnm"] & 1:
        pt = o["part"]
        if bug == "merge_no_between":
            mu32 = RB.seq_sum32(pt[:, :, 0]) / f32(pt.shape[1])
            rs32 = f32(1.0) / np.sqrt(RB.seq_sum32(pt[:, :, 1]) / f32(256.0 * pt.shape[1]) + f32(EPS))
        else:
            me = RB.merge_emulation(pt, EPS)
            mu32, rs32 = me["mean"], me["rstd"]
    csv = (o["cs_unrounded"] if bug == "cs_unrounded" else o["cs"][:N]).astype(f32) if kind.startswith("fold") else None

    def padN(v):
        w = np.zeros(tiles_n * 256, dtype=f32)
        w[:len(v)] = v
        return w
    bias = padN(o["bias"][:N].astype(f32)) if "bias" in o and kind not in ("none", "gelugrad", "resid-nobias", "scale-gelugrad", "scale-resid", "f32") else padN(np.zeros(N, f32))
    if csv is not None:
        csv = padN(csv)

    def opnd(name):
        w = np.zeros((Mp, tiles_n * 256), dtype=f32)
        w[:M, :N] = o[name]
        return w
    resid = opnd("resid") if kind in ("resid", "resid-nobias", "drop", "stats", "rebuild", "scale-resid") else None
    pre = opnd("pre") if kind in ("gelugrad", "scale-gelugrad") else None
    accw = np.zeros((Mp, tiles_n * 256), dtype=f32)
    accw[:M, :N] = acc
    seen = set()
    for items in static_walk(nitems, grid):
        if bug == "last_item_skipped" and len(items) > 1:
            items = items[:-1]
        prev = None
        for k, item in enumerate(items):
            _, tile = item_tile(item, nitems, ntiles, rev)
            if bug == "rev_two_to_one" and rev and (item >> 3) == 1:
                _, tile = item_tile(item - 8, nitems, ntiles, rev)
            seen.add(tile)
            m0, n0 = (tile // tiles_n) * 256, (tile % tiles_n) * 256
            rows, cols = slice(m0, m0 + 256), slice(n0, n0 + 256)
            prow, pcol = (slice(prev[0], prev[0] + 256), slice(prev[1], prev[1] + 256)) if prev is not None else (rows, cols)
            v = accw[rows, cols].copy()
            srow = prow if bug == "stats_prev_item" else rows
            bcol = pcol if bug == "bias_prev_item" else cols
            if case["lnm"] & 1:
                mu, rs = mu32[srow][:, None], rs32[srow][:, None]

            def operand(w):
                t = w[rows, cols].copy()
                if bug == "opnd_chunk0_prev":
                    for wm in (0, 128):
                        t[wm:wm + 8] = w[prow, pcol][wm:wm + 8]
                return t
            if kind.startswith("fold"):
                v = fold_eval32(v, mu, rs, csv[bcol][None, :], bias[bcol][None, :])
            elif kind not in ("gelugrad", "scale-gelugrad"):
                v = v + bias[bcol][None, :]
            if kind in ("gelu", "fold-gelu"):
                aux[rows, cols] = RB.store(v, BF16)
                v = O.gelu(v.astype(np.float64)).astype(f32)
            prodv = None
            if kind in ("gelugrad", "scale-gelugrad"):
                v = v * O.gelu_grad(operand(pre).astype(np.float64)).astype(f32)
                if kind == "scale-gelugrad":
                    prodv = v.copy()
                    v = v * rs
            if keep is not None:
                kp = np.zeros((256, 256), dtype=bool)
                kk = keep[m0:min(m0 + 256, M), n0:min(n0 + 256, N)]
                kp[:kk.shape[0], :kk.shape[1]] = kk
                v = np.where(kp, v * (f32(1.0) / (f32(1.0) - f32(p))), f32(0))
            if kind in ("resid", "resid-nobias", "drop", "stats"):
                v = v + operand(resid)
            elif kind == "scale-resid":
                v = v + rs * operand(resid)
            elif kind == "rebuild":
                g, be = padN(o["gamma"].astype(f32))[cols][None, :], padN(o["beta"].astype(f32))[cols][None, :]
                v = v + RB.store((operand(resid) - mu) * rs * g + be, BF16)
            stored = v if kind in ("f32", "fold32") else RB.store(v, BF16)
            Cw[rows, cols] = stored
            if part is not None:
                full = stats_out_emulation(stored)[:, 0, :].astype(np.float64)
                if bug == "fold_no_64d2":
                    sub = stored.reshape(256, 4, 64).astype(np.float64)
                    full[:, 1] = ((sub - sub.mean(-1, keepdims=True)) ** 2).sum((-1, -2))
                if bug == "part_prev_slot" and prev is not None:
                    part[prow, prev[1] // 256] = full
                else:
                    part[rows, n0 // 256] = full
            if colsum is not None and not (bug == "colsum_once_per_wg" and k > 0):
                src = stored if (kind != "scale-gelugrad" or bug == "colsum_scaled") else prodv
                w = min(256, N - n0)
                colsum[n0:n0 + w] = colsum[n0:n0 + w] + RB.seq_sum32(src[:, :w].T.astype(f32))
            prev = (m0, n0)
    outs = {"C": Cw[:M, :N].astype(np.float64)}
    if aux is not None:
        outs["aux"] = aux[:M, :N].astype(np.float64)
    if part is not None:
        outs["part"] = part.reshape(M, -1)
    if colsum is not None:
        outs["colsum"] = colsum.astype(np.float64)
    return outs
