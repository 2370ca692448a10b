"""Per-element error bounds for the training attention kernels (composer_amd/csrc/attention.hip): a float64 reference written out
without autograd, an emulation that rounds where the kernels round, the bound that the two give, inputs that make every key count,
and `attn_check`, which applies all of it to the arrays of one forward + backward launch.  numpy and torch on the CPU.

One (batch, head) group at a time: q, k, v, do are [T, D]; keep is the [T, T] dropout mask of the group (oracle counter hash) or None.

    s   = q k^T scale,  w = s b - 1e4 (1 - b)  (b = the causal triangle; transformer.py:351-354),  lse = logsumexp_j w,  P = exp(w - lse)
    P~  = P o keep / (1 - p)                     o  = P~ v
    dP  = (do v^T) o keep / (1 - p)              delta_i = sum_d do_id o_id, o = the o that was STORED (the kernels read it back)
    dS  = P o (dP - delta)                       dq = scale dS k,   dk = scale dS^T q,   dv = P~^T do
    rstd-scaled backward (cmp_attn_bwd_ln_next): row t of dq, dk, dv times rstd[t].

Bound.  In bf16 mode the kernels keep scores, probabilities, row sums and accumulators in fp32 and round to bf16 exactly where an fp32
tile becomes an MFMA operand (P in the forward and dK/dV kernels, dS in dQ and dK/dV: attention.hip:230) and where an output is
stored (:306, :330).  Each rounding multiplies ONE summand of an output element by (1 + e), |e| <= u = 2^-9, independently of the
others, so to first order the error of o[i, d] = sum_j P~_ij v_jd is sum_j e_ij P~_ij v_jd: a sum of independent zero-mean terms, whose
size is the quadrature sum

    S2_o [i, d] = sqrt(sum_j (P~_ij v_jd)^2)                       S2_dv[j, d] = sqrt(sum_i (P~_ij do_id)^2)
    S2_dq[i, d] = scale sqrt(sum_j (dS_ij k_jd)^2 + (sd_i sum_j P_ij k_jd)^2)
    S2_dk[j, d] = scale sqrt(sum_i (dS_ij q_id)^2 + sum_i (P_ij sd_i q_id)^2)          sd_i = sqrt(sum_d (do_id o_id)^2)

(times rstd[row] for the rstd-scaled backward).  The second term of dq and dk is what the rounding of the stored o does through
delta: delta_i moves by sum_d e_id do_id o_id (size u sd_i), which shifts the whole row i of dS by -P_ij times that -- ONE draw per
query row, so coherent along the row in dq (|sum_j P_ij k_jd|) and independent from query to query in dk (quadrature over i).  The
reference takes delta from the stored o too, so this term is no error of a kernel against it; it stays in S2 because it is the scale
on which dq of a row with dP = delta (position 0, p = 0: exactly zero) is resolved at all.  fp32 mode: the same S2 with u = 2^-24.
All-terms-absolute S = |P~| |v| (gemm_bound) is ~20 times looser on diffuse rows and is not used.

    q2    = max over the case of |emulation - reference| / S2, measured on the CPU from `attn_emulation`, never from a kernel
    limit = 2 max(q2, u) S2  (+ 2^-8 |reference| for a bf16 store: kernel_arena.BF16_OUT)
            (+ in fp32 mode the allowances of `f32_allowances` for the fp32 chains behind a score and behind dP - delta)

The factor 2: a kernel's roundings (another summation order, v_exp_f32, a stale running maximum under the deferred rescale) are
another draw from the distribution the emulation samples.  q2 came out at 2.4 u .. 4.3 u for every output in bf16 and at tens of u
in fp32, where the rounding of a score is a relative error of its probability (tests/test_gpu_attention_bounds.py lists them).

lse and delta are fp32 quantities in BOTH modes and get the fp32 idiom of tests/test_gpu_decode_logits.py: floor = max |float32
restatement - float64| over the case, limit = 4 floor + 1e-6 max |reference|; delta's reference is the float64 rowsum(do o) of the o
the kernel itself stored.
"""
import math

import numpy as np
import torch

from oracle import transformer_oracle as O
from kernel_arena import BF16_OUT

FP32, BF16 = 0, 1
U = {FP32: 2.0 ** -24, BF16: 2.0 ** -9}
MARGIN = 2.0
F32_MARGIN, F32_ABS = 4.0, 1e-6
LOG2E = 1.4426950408889634
# partner offsets: both sides of every tile size of attention.hip (32-key sub-tile, 64-key tile, 128-row block, 256-row key-split tile)
OFFSETS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256)
PARTNER_TARGET = 0.4
PARTNER_SCORE_MAX = 60.0
OUTPUTS = ("o", "dq", "dk", "dv")
f32 = np.float32


def bf16r(x):
    """float32 -> bf16 (round to nearest even) -> float32, as v_cvt_pk_bf16_f32 / the (bf16_t) casts of the kernels do."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def group_keep(seed, stream, g, T, p):
    """The dropout mask of (batch, head) group g = b * H + h: rows (g T + query), columns keys."""
    return O.dropout_keep_rows(seed, stream, T, T, p, row0=g * T) if p > 0 else None


# ---------------------------------------------------------------------------------------------------------------- reference
def attn_reference(q, k, v, do, keep, p, scale, o_stored=None, rstd=None):
    """float64, everything written out -> dict(lse, P, Pt, o, dP, delta, dS, dq, dk, dv).  delta comes from `o_stored` (the o a kernel
    wrote and reads back) when given, else from the reference's own o."""
    q, k, v, do = (np.asarray(a, dtype=np.float64) for a in (q, k, v, do))
    T = q.shape[0]
    b = np.tril(np.ones((T, T)))
    w = (q @ k.T) * scale * b - 1e4 * (1 - b)
    m = w.max(1, keepdims=True)
    e = np.exp(w - m)
    l = e.sum(1, keepdims=True)
    P = e / l
    f = 1.0 / (1.0 - p)
    kf = f if keep is None else keep * f
    Pt = P * kf
    o = Pt @ v
    dP = (do @ v.T) * kf
    delta = (do * (o if o_stored is None else np.asarray(o_stored, dtype=np.float64))).sum(1)
    dS = P * (dP - delta[:, None])
    r = np.ones((T, 1)) if rstd is None else np.asarray(rstd, dtype=np.float64).reshape(T, 1)
    return dict(lse=(m + np.log(l))[:, 0], P=P, Pt=Pt, o=o, dP=dP, delta=delta, dS=dS,
                dq=scale * (dS @ k) * r, dk=scale * (dS.T @ q) * r, dv=(Pt.T @ do) * r)


def attn_s2(ref, q, k, v, do, scale, o_stored=None, rstd=None):
    """The quadrature sums of the module docstring, per element, float64 -> dict(o, dq, dk, dv)."""
    q, k, v, do = (np.asarray(a, dtype=np.float64) for a in (q, k, v, do))
    T = q.shape[0]
    P, Pt, dS = ref["P"], ref["Pt"], ref["dS"]
    o = ref["o"] if o_stored is None else np.asarray(o_stored, dtype=np.float64)
    sd2 = ((do * o) ** 2).sum(1)                                    # sd_i^2
    r = np.ones((T, 1)) if rstd is None else np.abs(np.asarray(rstd, dtype=np.float64)).reshape(T, 1)
    return dict(o=np.sqrt((Pt ** 2) @ (v ** 2)),
                dv=np.sqrt((Pt.T ** 2) @ (do ** 2)) * r,
                dq=scale * np.sqrt((dS ** 2) @ (k ** 2) + sd2[:, None] * (P @ k) ** 2) * r,
                dk=scale * np.sqrt((dS.T ** 2) @ (q ** 2) + ((P ** 2) * sd2[:, None]).T @ (q ** 2)) * r)


# ---------------------------------------------------------------------------------------------------------------- emulation
def seq_f32_mm(a, b):
    """a [M, K] . b [K, N] in float32, accumulated over k STRICTLY in order: one rank-1 update per k (kernel_arena.seq_fp32_matmul)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    for kk in range(a.shape[1]):
        acc += a[:, kk:kk + 1] * b[kk:kk + 1, :]
    return acc


def attn_emulation(q, k, v, do, keep, p, scale, dtype, rstd=None):
    """The reference's formulas with the kernels' number formats -> dict(lse, delta, o_st, and per output X: X = the value in front of
    the store, X_st = as stored).  bf16 mode rounds where attention.hip rounds (the line each rounding stands for is named beside it);
    fp32 mode is the same formulas in float32 (parity mode: scale, mask to -1e4, expf; attention.hip:588-615, 823, 1045)."""
    q, k, v, do = (np.ascontiguousarray(a, dtype=np.float32) for a in (q, k, v, do))
    T = q.shape[0]
    tri = np.tril(np.ones((T, T), dtype=bool))
    kp = np.ones((T, T), dtype=bool) if keep is None else keep
    f = f32(1.0 / (1.0 - p)) if p > 0 else f32(1.0)                # DropCfg.scale
    sc = f32(scale)
    r = np.ones((T, 1), dtype=np.float32) if rstd is None else np.asarray(rstd, dtype=np.float32).reshape(T, 1)
    if dtype == FP32:
        # parity mode multiplies with v_mfma_f32_32x32x2_f32 (:84): every accumulator is ONE fp32 chain, over the head dimension for
        # the scores and dP (mma_rows, :198), over ALL keys of a query row for o and dq and over all queries of a key for dk and dv
        # (mma_acc_b, :213).  numpy's blocked float32 product rounds less than such a chain, so the products here are sequential too.
        mm = seq_f32_mm
        s = mm(q, k.T)
        dp_raw = mm(do, v.T)
        w = np.where(tri, s * sc, f32(-1e4))
        m = w.max(1, keepdims=True)
        e = np.exp(w - m)
        l = e.sum(1, keepdims=True, dtype=np.float32)
        lse = (m + np.log(l))[:, 0]
        o = mm(e * kp, v) * (f / l)
        o_st = o
        # :784-790 -- NOT the chain of dP: lane half h holds the elements 2 s + h of the row (load_bfrags, :177), sums those in order,
        # and half_sum adds the two halves.  At T = 1, p = 0 (P = 1, o = v, dP = delta in exact arithmetic) dq IS the residue between
        # the two orders, a few ulp of |do.v|; with delta on dP's chain the emulation called it exactly zero.
        prod, one = o_st * do, np.ones((q.shape[1] // 2, 1), dtype=np.float32)
        delta = (mm(prod[:, 0::2], one) + mm(prod[:, 1::2], one))[:, 0]
        del_q = (delta / f)[:, None]
        P = np.where(tri, np.exp(s * sc - lse[:, None]), f32(0))
        dS = P * (np.where(kp, dp_raw, f32(0)) - del_q)
        Pd = P * kp
        out = dict(o=o, dq=mm(dS, k) * (sc * f * r), dk=mm(dS.T, q) * (sc * f * r), dv=mm(Pd.T, do) * (f * r))
        out.update({n + "_st": out[n] for n in OUTPUTS})
        out.update(w=np.where(tri, s * sc, f32(0)), dp=np.where(tri, dp_raw, f32(0)))     # for `f32_allowances`
    else:
        s = q @ k.T                                                 # fp32 MFMA accumulators of exact bf16 products: their order is
        dp_raw = do @ v.T                                           # 2^-24 against the 2^-9 roundings below
        c2 = f32(sc * f32(LOG2E))
        w = np.where(tri, s, f32(-1e4) / sc)                        # throughput mode works on raw scores (:487, :624)
        m = w.max(1, keepdims=True)
        e = np.exp2(w * c2 - m * c2)                                # :253 (v_exp_f32 of one fma)
        l = e.sum(1, keepdims=True, dtype=np.float32)               # the row sum takes the UNROUNDED probabilities (:254-255)
        lse = (m * sc + np.log(l))[:, 0]                            # :705
        pb = bf16r(e * kp)                                          # :230 -- P becomes the bf16 B operand of O^T += V^T P^T
        o = (pb @ v) * (f / l)                                      # :702
        o_st = bf16r(o)                                             # :306 / :330 -- the store
        delta = (o_st * do).sum(1, dtype=np.float32)                # :787 / :989 -- fp32 from the bf16 o that was stored
        del_q = (delta / f)[:, None]                                # :792 / :993
        P = np.where(tri, np.exp2(s * c2 - (lse * f32(LOG2E))[:, None]), f32(0))      # :828 / :1046 from the STORED fp32 lse
        dsq = bf16r(P * (np.where(kp, dp_raw, f32(0)) - del_q))     # :840, then :230 -- dS becomes the B operand of dQ^T += K^T dS^T
        Pd = P * kp
        # dK/dV: with dropout  fma(M p, dP~, -(p delta/f))  (:1077), without  p (dP~ - delta)  (:1070); both -> bf16 at :230
        dsk = bf16r(Pd * dp_raw - P * del_q) if p > 0 else bf16r(P * (dp_raw - del_q))
        out = dict(o=o, dq=(dsq @ k) * (sc * f * r),                # :877
                   dk=(dsk.T @ q) * (sc * f * r),                   # :1128
                   dv=(bf16r(Pd).T @ do) * (f * r))                 # :230 (the dropped P feeds dV), :1129
        out.update({n + "_st": bf16r(out[n]) for n in OUTPUTS})     # :306 / :330
    out.update(lse=lse, delta=delta, o_st=out["o_st"])
    return out


def q2_of(emu, ref, s2):
    """max |emulation (in front of the store) - reference| / S2 per output, over the elements whose S2 is not zero."""
    out = {}
    for n in OUTPUTS:
        nz = s2[n] > 0
        out[n] = float((np.abs(emu[n].astype(np.float64) - ref[n])[nz] / s2[n][nz]).max()) if nz.any() else 0.0
    return out


def attn_limits(ref, s2, q2, dtype, allow=None):
    """limit = 2 max(q2, u) S2 (+ 2^-8 |ref| for a bf16 store) (+ the fp32 allowance of `f32_allowances`), per element."""
    return {n: MARGIN * max(q2[n], U[dtype]) * s2[n] + (BF16_OUT * np.abs(ref[n]) if dtype == BF16 else 0.0)
            + (0.0 if allow is None else allow[n]) for n in OUTPUTS}


def f32_allowances(gb, rho, dtype):
    """fp32 mode only (None in bf16 mode, where the same terms are 2^-15 of the limits).  S2 weighs every summand alike, but in fp32 mode
    what a summand carries is not one rounding of size u: its probability is exp of a score that an fp32 chain of D products computed
    (attention.hip:198, :606, :823, :1045), and dS is P times the difference of two such chains, dP (:198) and delta (:784-790).  Those
    errors follow the chains' own sizes, whatever the summand's, and the elements of a row share them, so a case of a few rows has a
    few draws of them and q2 over the case cannot know their tail (T = 1: P = 1, and dq, dk ARE the residue of the two chains).  They get
    allowances in the form of kernel_arena.f32_eval_allowance -- 4 x the largest deviation of the float32 evaluation (the emulation's)
    from float64 over the case -- with the deviation taken relative to the chain's natural size, so that a row of small scores is not
    given what a row of large ones needs:
        rho_w = max dev(w_ij) / A_ij,    A_ij  = scale sum_d |q_id k_jd|          ew_ij = 4 rho_w A_ij
        rho_p = max dev(dP_ij) / Ap_ij,  Ap_ij = sum_d |do_id v_jd|
        rho_d = max dev(delta_i) / Ad_i, Ad_i  = sum_d |do_id o_id|               ec_ij = 4 (rho_d Ad_i + rho_p Ap_ij / (1 - p))
    A score error e_ij <= ew_ij multiplies P_ij by 1 + e_ij - L_i with |L_i| <= sum_j' P_ij' ew_ij': independent over j on the summands,
    one factor per row through lse.  o: sqrt(sum_j (ew_ij P~_ij v_jd)^2) + L_i |o_id|; dq the same on dS k; dv and dk, whose summands
    run over the queries: sqrt(sum_i ((ew_ij + L_i) summand)^2).  An error c_ij <= ec_ij of dP_ij - delta_i adds scale P_ij c_ij k_jd to dq
    (sum_j P_ij ec_ij |k_jd|) and, independent over the queries, scale sqrt(sum_i (P_ij ec_ij q_id)^2) to dk.  `group_bounds` holds each
    term at rho = 1 (aw, ad, ap); the rhos are the largest over the case (`case_rho`)."""
    if dtype != FP32:
        return None
    z = 0.0
    return {n: 4.0 * (rho["w"] * gb["aw"][n] + rho["d"] * gb["ad"].get(n, z) + rho["p"] * gb["ap"].get(n, z)) for n in OUTPUTS}


def case_rho(gbs):
    """The relative deviations of `f32_allowances` over the groups of a case."""
    return {n: max(gb["rho"][n] for gb in gbs) for n in ("w", "d", "p")}


def _allowance_terms(ref, emu, ref_e, q, k, v, do, o_stored, delta32, p, scale, rstd):
    """-> rho (this group's relative deviations) and the allowance terms at rho = 1: aw, ad, ap (dicts per output)."""
    q, k, v, do, o = (np.asarray(a, dtype=np.float64) for a in (q, k, v, do, o_stored))
    T = q.shape[0]
    tri = np.tril(np.ones((T, T), dtype=bool))
    r = np.ones((T, 1)) if rstd is None else np.abs(np.asarray(rstd, dtype=np.float64)).reshape(T, 1)
    P, Pt, dS = ref["P"], ref["Pt"], ref["dS"]
    A = np.where(tri, (np.abs(q) @ np.abs(k).T) * scale, 0.0)
    Ap = np.where(tri, np.abs(do) @ np.abs(v).T, 0.0) / (1.0 - p)
    Ad = np.abs(do * o).sum(1)
    tiny = 1e-300
    rho = dict(w=float((np.abs(emu["w"] - np.where(tri, (q @ k.T) * scale, 0.0)) / np.maximum(A, tiny))[tri].max()),
               p=float((np.abs(emu["dp"] - np.where(tri, do @ v.T, 0.0)) / np.maximum(Ap * (1.0 - p), tiny))[tri].max()),
               d=float((np.maximum(np.abs(delta32 - ref["delta"]), np.abs(emu["delta"] - ref_e["delta"])) / np.maximum(Ad, tiny)).max()))
    L = (P * A).sum(1, keepdims=True)
    AL = A + L
    aw = dict(o=np.sqrt(((A * Pt) ** 2) @ (v ** 2)) + L * np.abs(ref["o"]),
              dq=scale * np.sqrt(((A * dS) ** 2) @ (k ** 2)) * r + L * np.abs(ref["dq"]),
              dv=np.sqrt(((AL * Pt).T ** 2) @ (do ** 2)) * r,
              dk=scale * np.sqrt(((AL * dS).T ** 2) @ (q ** 2)) * r)
    ad = dict(dq=scale * Ad[:, None] * (P @ np.abs(k)) * r, dk=scale * np.sqrt(((P * Ad[:, None]).T ** 2) @ (q ** 2)) * r)
    ap = dict(dq=scale * ((P * Ap) @ np.abs(k)) * r, dk=scale * np.sqrt(((P * Ap).T ** 2) @ (q ** 2)) * r)
    return rho, aw, ad, ap


def group_bounds(q, k, v, do, keep, p, scale, dtype, o_stored=None, rstd=None):
    """Everything the check of one group needs.  With o_stored = None the emulation's own stored o takes the kernel's place (the CPU
    tests); q2 is always the emulation against the reference that reads the EMULATION's stored o.
    -> dict(ref, emu, s2, q2, lse_floor, delta_floor, delta_ref, rho and, in fp32 mode, aw, ad, ap: `f32_allowances`)."""
    emu = attn_emulation(q, k, v, do, keep, p, scale, dtype, rstd)
    ref_e = attn_reference(q, k, v, do, keep, p, scale, emu["o_st"], rstd)
    q2 = q2_of(emu, ref_e, attn_s2(ref_e, q, k, v, do, scale, emu["o_st"], rstd))
    if o_stored is None:
        ref, o_stored = ref_e, emu["o_st"]
    else:
        ref = attn_reference(q, k, v, do, keep, p, scale, o_stored, rstd)
    s2 = attn_s2(ref, q, k, v, do, scale, o_stored, rstd)
    o32, do32 = np.asarray(o_stored, dtype=np.float32), np.asarray(do, dtype=np.float32)
    delta32 = (o32 * do32).sum(1, dtype=np.float32)
    delta_floor = float(np.abs(delta32 - ref["delta"]).max())
    out = dict(ref=ref, emu=emu, s2=s2, q2=q2, lse_floor=float(np.abs(emu["lse"] - ref["lse"]).max()), delta_floor=delta_floor,
               delta_ref=ref["delta"])
    if dtype == FP32:
        out["rho"], out["aw"], out["ad"], out["ap"] = _allowance_terms(ref, emu, ref_e, q, k, v, do, o_stored, delta32, p, scale, rstd)
    else:
        out["rho"] = dict(w=0.0, d=0.0, p=0.0)
    return out


def f32_limit(floor, ref):
    return F32_MARGIN * floor + F32_ABS * float(np.abs(ref).max())


def _fail(what, g, name, out, ref, lim):
    err = np.abs(out - ref)
    bad = ~(err <= lim)
    idx = tuple(int(i) for i in np.argwhere(bad)[0])
    pos = "row %d, column %d" % idx if len(idx) == 2 else "row %d" % idx
    worst = float((err / np.maximum(lim, 1e-300)).max())
    raise AssertionError("%s: group %d, %s, %s is %.9g, reference %.9g: error %.3g > limit %.3g (worst error/limit of the group %.3g, %d of %d elements)"
                         % (what, g, name, pos, out[idx], ref[idx], err[idx], lim[idx], worst, int(bad.sum()), bad.size))


def within(what, g, name, out, ref, lim):
    """max error / limit of one array of one group; raises with group, output, row, column, error and limit (as assert_within)."""
    out, ref = np.asarray(out, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    lim = np.broadcast_to(np.asarray(lim, dtype=np.float64), ref.shape)
    err = np.abs(out - ref)
    if not bool((err <= lim).all()):              # (a NaN fails)
        _fail(what, g, name, out, ref, lim)
    return float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.0


def _within(fails, what, g, name, out, ref, lim):
    """`within`, with the first failure of every output kept in `fails` instead of raised -> the worst error / limit (inf for a NaN)."""
    try:
        return within(what, g, name, out, ref, lim)
    except AssertionError as e:
        fails.setdefault(name, str(e))
        with np.errstate(invalid="ignore"):
            r = np.abs(np.asarray(out, dtype=np.float64) - ref) / np.maximum(lim, 1e-300)
        return float(np.where(np.isnan(r), np.inf, r).max())


def split_heads(qkv, do, B, T, H, D):
    """[B T, 3E] / [B T, E] tensors as stored -> float64 numpy [B, T, 3, H, D], [B, T, H, D]."""
    return (qkv.detach().double().cpu().numpy().reshape(B, T, 3, H, D), do.detach().double().cpu().numpy().reshape(B, T, H, D))


def attn_check(qkv, do, o, lse, delta, dqkv, B, T, H, D, dtype, p, scale, seed, stream, groups, rstd=None, what="attention",
               raise_on_fail=True):
    """One forward + backward launch against the bound.  qkv [B T, 3E], do, o [B T, E], dqkv [B T, 3E] as stored (any device), lse and
    delta fp32 [B H T]; `groups` = the (batch, head) pairs that get the float64 reference; rstd [B T] for the rstd-scaled backward.
    The per-case quantities (q2, the fp32 floors, max |ref|) are taken over all listed groups first, then every group is held to the
    limits.  -> {"o", "dq", "dk", "dv", "lse", "delta": worst error / limit, "q2": {output: q2}, "fails": {output: message}}; the first
    failure is raised unless raise_on_fail is off (the CPU tests that look at every output of a wrong kernel)."""
    qh, dh = split_heads(qkv, do, B, T, H, D)
    oh = o.detach().double().cpu().numpy().reshape(B, T, H, D)
    gh = dqkv.detach().double().cpu().numpy().reshape(B, T, 3, H, D)
    lh = lse.detach().double().cpu().numpy().reshape(B, H, T)
    dlh = delta.detach().double().cpu().numpy().reshape(B, H, T)
    rs = None if rstd is None else rstd.detach().double().cpu().numpy().reshape(B, T)
    per = []
    for b, h in groups:
        g = b * H + h
        gb = group_bounds(qh[b, :, 0, h], qh[b, :, 1, h], qh[b, :, 2, h], dh[b, :, h], group_keep(seed, stream, g, T, p), p, scale,
                          dtype, o_stored=oh[b, :, h], rstd=None if rs is None else rs[b])
        del gb["emu"]
        for n in ("P", "Pt", "dP", "dS"):
            del gb["ref"][n]
        per.append((b, h, g, gb))
    q2 = {n: max(gb["q2"][n] for *_, gb in per) for n in OUTPUTS}
    lse_lim = f32_limit(max(gb["lse_floor"] for *_, gb in per), np.concatenate([gb["ref"]["lse"] for *_, gb in per]))
    delta_lim = f32_limit(max(gb["delta_floor"] for *_, gb in per), np.concatenate([gb["delta_ref"] for *_, gb in per]))
    rho = case_rho([gb for *_, gb in per])
    worst, fails = dict.fromkeys(OUTPUTS + ("lse", "delta"), 0.0), {}
    for b, h, g, gb in per:
        lim = attn_limits(gb["ref"], gb["s2"], q2, dtype, f32_allowances(gb, rho, dtype))
        got = dict(o=oh[b, :, h], dq=gh[b, :, 0, h], dk=gh[b, :, 1, h], dv=gh[b, :, 2, h])
        worst["lse"] = max(worst["lse"], _within(fails, what, g, "lse", lh[b, h], gb["ref"]["lse"], lse_lim))
        worst["delta"] = max(worst["delta"], _within(fails, what, g, "delta", dlh[b, h], gb["delta_ref"], delta_lim))
        for n in OUTPUTS:
            worst[n] = max(worst[n], _within(fails, what, g, n, got[n], gb["ref"][n], lim[n]))
    worst.update(q2=q2, fails=fails)
    if raise_on_fail:
        raise_first(worst)
    return worst


def raise_first(worst):
    """Raises the first failure that `attn_check` kept (a caller that prints the figures first passes raise_on_fail=False, then this)."""
    if worst["fails"]:
        raise AssertionError(next(worst["fails"][n] for n in ("o", "lse", "dq", "dk", "dv", "delta") if n in worst["fails"]))


def figures(what, worst, dtype):
    """One line: the worst error / limit of every output of a case and its q2 in units of u."""
    return "ATTN_BOUNDS %s | err/limit %s | q2/u %s" % (what, " ".join("%s %.2f" % (n, worst[n]) for n in ("o", "lse", "dq", "dk", "dv", "delta")),
                                                        " ".join("%s %.1f" % (n, worst["q2"][n] / U[dtype]) for n in OUTPUTS))


# ---------------------------------------------------------------------------------------------------------------- inputs
def partner_of(T, off):
    return np.maximum(np.arange(T) - off, 0)


def attn_inputs(B, T, H, D, scale, seed, target=PARTNER_TARGET, device="cpu"):
    """Planted partners on a randn background -> (qkv [B T, 3E], do [B T, E]) float32 CPU tensors (round them to the launch's dtype).

    q ~ N(0, a^2) with a^2 = 1 / (scale sqrt(D)), and the keys are randn directions of length a sqrt(D), so that background scores
    q.k scale are N(0, 1) at either value of `scale`; v, do ~ N(0, 1).  The keys have ONE length because with randn lengths, at D = 16,
    one key in ten has a longer neighbour within 40 degrees, which outgrows it under any multiple of it: no multiple gives such a row
    its partner.

    In group g = b H + h query i carries a multiple c_i of its partner key k_pi(i), pi(i) = max(i - off, 0), off = OFFSETS[g mod 13]:
    q_i = q0_i + c_i k_pi(i).  c_i solves P_{i, pi(i)} = `target` (Newton on the partner's logit, bisecting whenever a step leaves the
    bracket).  It grows like ln(i + 1) / (|k_pi|^2 scale) plus what the cross-talk c_i k_pi.k_j of the other keys adds; at D = 16 that
    cross-talk has a standard deviation of a quarter of the partner's score, and a closed form in ln(i + 1) alone leaves rows at
    probability 0.01 or 0.99.  A row's partner probability is then `target` up to the rounding of q to the launch's dtype, at any
    context length and under either dropout draw: deleting key j moves row j + off of o by a factor 1 / (1 - target) whether or not
    the pair itself was dropped.

    The last key is seen by ONE row, the last, so its dk is a single value of P (dP - delta) q: the last row's do is randn plus its own
    v, which makes do.v of the order of D and that value large in every group (dv of that key is P~ do, large unless dropout removed the
    pair -- then it is zero with or without the key).

    device: where the multiples are solved (the draws themselves always come from the CPU generator); a GPU test with hundreds of
    groups passes "cuda" -- plumbing, nothing of it is under test."""
    E = H * D
    gen = torch.Generator().manual_seed(seed)
    amp = (scale * math.sqrt(D)) ** -0.5
    x = torch.randn(B, T, 3, H, D, generator=gen)
    x[:, :, 0] *= amp
    x[:, :, 1] *= amp * math.sqrt(D) / x[:, :, 1].norm(dim=-1, keepdim=True)       # keys: randn directions at ONE length
    do = torch.randn(B * T, E, generator=gen)
    do.view(B, T, H, D)[:, T - 1] += x[:, T - 1, 2]                 # the last row's do leans on its own v (docstring)
    x = x.to(device)
    q0 = x[:, :, 0].permute(0, 2, 1, 3).reshape(B * H, T, D)
    k = x[:, :, 1].permute(0, 2, 1, 3).reshape(B * H, T, D)
    pi = torch.stack([torch.from_numpy(partner_of(T, OFFSETS[g % len(OFFSETS)])) for g in range(B * H)]).to(device)       # [G, T]
    ar = torch.arange(T, device=device)
    causal = ar[None, :] <= ar[:, None]
    lg = math.log(target / (1 - target))
    step = max(1, (48 << 20) // (T * T))                            # groups per chunk: ~200 MB of float32 per [G, T, T] temporary
    for g0 in range(0, B * H, step):
        sl = slice(g0, min(B * H, g0 + step))
        kk, pp = k[sl], pi[sl]
        kpart = torch.gather(kk, 1, pp[:, :, None].expand(-1, -1, D))                   # k_pi(i)
        A = (q0[sl] @ kk.transpose(1, 2)) * scale                                       # background scores
        Gp = (kpart @ kk.transpose(1, 2)) * scale                                       # what one unit of c adds to row i's scores
        other = causal[None] & (ar[None, None, :] != pp[:, :, None])
        A.masked_fill_(~other, float("-inf"))                                          # rows keep only the OTHER keys; the partner's own:
        a_p = (q0[sl] * kpart).sum(-1) * scale
        g_p = (kpart * kpart).sum(-1) * scale
        c = torch.zeros(kk.shape[0], T, device=device)
        hi = PARTNER_SCORE_MAX / g_p                                                    # the partner's own score stays below 60: no
        lo = -hi                                                                        # fp32 overflow anywhere near
        for _ in range(12):
            w = torch.addcmul(A, c[:, :, None], Gp)
            mx = w.amax(-1, keepdim=True).clamp_min(-1e30)
            w = w.sub_(mx).exp_()
            den = w.sum(-1)
            lse_o = mx[:, :, 0] + den.log()                                             # -inf for row 0 (no other key)
            fval = a_p + c * g_p - lse_o - lg
            fin = torch.isfinite(lse_o)
            if not bool(fin.any()) or float(fval[fin].abs().max()) < 0.1:               # every partner within 0.025 of the target
                break
            slope = g_p - w.mul_(Gp).sum(-1) / den.clamp_min(1e-30)
            lo, hi = torch.where(fval < 0, c, lo), torch.where(fval >= 0, c, hi)
            cn = c - fval / slope
            cn = torch.where((slope > 0) & (cn > lo) & (cn < hi), cn, 0.5 * (lo + hi))  # a Newton step inside the bracket, else bisect
            c = torch.where(torch.isfinite(lse_o), cn, c)
        q0[sl] += c[:, :, None] * kpart
    qkv = torch.empty(B, T, 3, H, D)
    qkv[:, :, 0] = q0.reshape(B, H, T, D).permute(0, 2, 1, 3).cpu()
    qkv[:, :, 1:] = x[:, :, 1:].cpu()
    return qkv.reshape(B * T, 3 * E).contiguous(), do


def randn_inputs(B, T, H, D, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B * T, 3 * H * D, generator=gen), torch.randn(B * T, H * D, generator=gen)


def partner_probability(P, off):
    """P [T, T] of a group with partner offset off -> the partner's probability of every row that has one (another key to share with)."""
    T = P.shape[0]
    return P[np.arange(1, T), partner_of(T, off)[1:]]


def covering_groups(B, H, want=len(OFFSETS)):
    """(batch, head) pairs whose group numbers cover every partner offset the grid holds: the first min(B H, 13) groups and the last."""
    n = B * H
    gs = list(range(min(n, want)))
    if n - 1 not in gs:
        gs.append(n - 1)
    return [(g // H, g % H) for g in gs]
