"""The assertions of tests/attention_bounds.py can fail (CPU; the pattern of tests/test_kernel_checks_host.py).

`fake_attention` is a tile-structured numpy statement of the attention kernels -- 32-row query blocks, 64-key tiles of two 32-key
sub-tiles, a running maximum and sum with a rescale of the accumulator, the bf16 roundings of attention.hip, the oracle's dropout
hash, dQ per query block and dK/dV per key block -- correct, and wrong in the fourteen ways hand-written attention kernels go wrong.
Each wrong one must be rejected by `attn_check` on the output named for it, with that check's message.  To see that a class of error
is caught, edit a copy of `fake_attention` below -- not the library.

Further: the correct fake sits inside every limit; the planted inputs meet their conditions (partner probabilities, no overflow, the
float64 reference alone inside every limit); on every geometry of the GPU cases ANY single deleted key moves o, dq, dk, dv and lse by
ten limits; and the record of what the older global-maximum metric let through."""
import math
import re

import numpy as np
import pytest
import torch

import attention_bounds as AB
import test_gpu_attention_bounds as GB
import test_gpu_kernels as K

FP32, BF16 = AB.FP32, AB.BF16
f32 = np.float32
SEED, STREAM = 77, 9
SKIP_Q0, SKIP_K0 = 64, 32            # the (query block, key sub-tile) and (key block, query block) the skipping bugs leave out
BUGS = ("tail_key", "skip_subtile", "diag_wide", "diag_narrow", "no_rescale", "hash_row_above", "no_keep_scale", "bf16_acc", "lse_bf16",
        "delta_neighbour", "no_delta", "dv_undropped", "dkv_skip_block", "no_rstd")


def fake_group(q, k, v, do, keep, p, scale, dtype, rstd, bug):
    """One (batch, head) group, float32 arrays in, (o, lse, delta, dq, dk, dv) as a kernel would store them."""
    T, D = q.shape
    bf = dtype == BF16
    R = AB.bf16r if bf else (lambda x: x)
    sc = f32(scale)
    c2 = f32(sc * f32(AB.LOG2E))
    f = f32(1.0 / (1.0 - p)) if p > 0 else f32(1.0)
    kp_all = np.ones((T, T), dtype=bool) if keep is None else keep
    kp_fwd = np.concatenate([kp_all[:1], kp_all[:-1]]) if bug == "hash_row_above" else kp_all
    t_keys = T - 1 if bug == "tail_key" else T                     # forward and dQ stop one key short of the ragged tail
    o, lse = np.zeros((T, D), dtype=f32), np.zeros(T, dtype=f32)

    def masked(keys, qi):
        if bug == "diag_wide":
            return keys[None, :] > qi[:, None] + 1
        if bug == "diag_narrow":
            return keys[None, :] > np.maximum(qi[:, None] - 1, 0)
        return keys[None, :] > qi[:, None]

    # ---- forward: a 32-row query block walks its 64-key tiles, two 32-key sub-tiles each
    for q0 in range(0, T, 32):
        qi = np.arange(q0, min(T, q0 + 32))
        m, l, acc = np.full(len(qi), -np.inf, dtype=f32), np.zeros(len(qi), dtype=f32), np.zeros((len(qi), D), dtype=f32)
        kv_end = min(t_keys, q0 + 32)
        for kt in range(0, kv_end, 64):
            for k0 in (kt, kt + 32):
                if k0 >= kv_end or (bug == "skip_subtile" and (q0, k0) == (SKIP_Q0, SKIP_K0)):
                    continue
                keys = np.arange(k0, min(k0 + 32, t_keys))
                s, mk = q[qi] @ k[keys].T, masked(keys, qi)
                with np.errstate(invalid="ignore"):
                    if bf:                                               # throughput mode: raw scores, one fma into exp2
                        s = np.where(mk, f32(-1e4) / sc, s)
                        mnew = np.maximum(m, s.max(1))
                        alpha = np.exp2((m - mnew) * c2)
                        pr = np.exp2(s * c2 - (mnew * c2)[:, None])
                    else:                                                # parity mode: scale, mask to -1e4, exp
                        s = np.where(mk, f32(-1e4), s * sc)
                        mnew = np.maximum(m, s.max(1))
                        alpha = np.exp(m - mnew)
                        pr = np.exp(s - mnew[:, None])
                alpha = np.nan_to_num(alpha, nan=0.0)
                l = l * alpha + pr.sum(1, dtype=f32)
                if bug != "no_rescale":
                    acc *= alpha[:, None]
                m = mnew
                acc += R(pr * kp_fwd[qi][:, keys]) @ v[keys]
            if bug == "bf16_acc":
                acc = AB.bf16r(acc)
        o[qi] = acc * ((f32(1.0) if bug == "no_keep_scale" else f) / l)[:, None]
        lse[qi] = (m * sc if bf else m) + np.log(l)
    o = R(o)
    if bug == "lse_bf16":
        lse = AB.bf16r(lse)
    # ---- backward
    delta = (o * do).sum(1, dtype=f32)
    d_used = np.concatenate([delta[1:], delta[-1:]]) if bug == "delta_neighbour" else delta
    del_q = (np.zeros_like(delta) if bug == "no_delta" else d_used / f)[:, None]
    rs = np.ones((T, 1), dtype=f32) if (rstd is None or bug == "no_rstd") else np.asarray(rstd, dtype=f32).reshape(T, 1)

    def probs(qi, keys):
        s = q[qi] @ k[keys].T
        pr = np.exp2(s * c2 - (lse[qi] * f32(AB.LOG2E))[:, None]) if bf else np.exp(s * sc - lse[qi][:, None])
        return np.where(masked(keys, qi), f32(0), pr)

    dq, dk, dv = (np.zeros((T, D), dtype=f32) for _ in range(3))
    for q0 in range(0, T, 32):                                       # dQ: the forward's walk
        qi = np.arange(q0, min(T, q0 + 32))
        for k0 in range(0, min(t_keys, q0 + 32), 32):
            if bug == "skip_subtile" and (q0, k0) == (SKIP_Q0, SKIP_K0):
                continue
            keys = np.arange(k0, min(k0 + 32, t_keys))
            pr = probs(qi, keys)
            dp = np.where(kp_all[qi][:, keys], do[qi] @ v[keys].T, f32(0))
            dq[qi] += R(pr * (dp - del_q[qi])) @ k[keys]
    for k0 in range(0, T, 32):                                       # dK/dV: a 32-key block walks the query blocks at and below it
        keys = np.arange(k0, min(T, k0 + 32))
        for q0 in range(k0, T, 32):
            if bug == "dkv_skip_block" and (k0, q0) == (SKIP_K0, SKIP_Q0):
                continue
            qi = np.arange(q0, min(T, q0 + 32))
            pr = probs(qi, keys)
            kp = kp_all[qi][:, keys]
            dp = do[qi] @ v[keys].T
            pd = pr * kp
            ds = pd * dp - pr * del_q[qi] if p > 0 else pr * (dp - del_q[qi])
            dv[keys] += R(pr if bug == "dv_undropped" else pd).T @ do[qi]
            dk[keys] += R(ds).T @ q[qi]
    return o, lse, delta, R(dq * (sc * f * rs)), R(dk * (sc * f * rs)), R(dv * (f * rs))


def fake_attention(qkv, do, B, T, H, D, dtype, p, scale, rstd=None, bug=None):
    """The launch pair on [B T, 3E] / [B T, E] tensors as stored -> (o, lse, delta, dqkv) torch tensors in the layouts of the ABI."""
    qh, dh = AB.split_heads(qkv, do, B, T, H, D)
    o, dqkv = np.zeros((B, T, H, D), dtype=f32), np.zeros((B, T, 3, H, D), dtype=f32)
    lse, delta = np.zeros((B, H, T), dtype=f32), np.zeros((B, H, T), dtype=f32)
    for b in range(B):
        for h in range(H):
            a = [np.ascontiguousarray(x, dtype=f32) for x in (qh[b, :, 0, h], qh[b, :, 1, h], qh[b, :, 2, h], dh[b, :, h])]
            r = None if rstd is None else rstd.reshape(B, T)[b].numpy()
            og, lg, dg, dq, dk, dv = fake_group(*a, AB.group_keep(SEED, STREAM, b * H + h, T, p), p, scale, dtype, r, bug)
            o[b, :, h], lse[b, h], delta[b, h] = og, lg, dg
            dqkv[b, :, 0, h], dqkv[b, :, 1, h], dqkv[b, :, 2, h] = dq, dk, dv
    t = torch.from_numpy
    return t(o.reshape(B * T, H * D)), t(lse.reshape(-1)), t(delta.reshape(-1)), t(dqkv.reshape(B * T, 3 * H * D))


def stored(t, dtype):
    return t.to(torch.bfloat16) if dtype == BF16 else t


def run(T, D, dtype, p, bug=None, H=3, ln=False, inputs="planted", raise_on_fail=True):
    """The fake on B = 1, H groups (partner offsets 0, 1, 31) through attn_check -> its result (with "fails": output -> message)."""
    scale = 1.0 / math.sqrt(D)
    qkv, do = AB.attn_inputs(1, T, H, D, scale, seed=T + D) if inputs == "planted" else AB.randn_inputs(1, T, H, D, seed=T + D)
    qkv, do = stored(qkv, dtype), stored(do, dtype)
    rstd = 0.3 + 2.7 * torch.rand(T, generator=torch.Generator().manual_seed(T)) if ln else None
    o, lse, delta, dqkv = fake_attention(qkv, do, 1, T, H, D, dtype, p, scale, rstd=rstd, bug=bug)
    return AB.attn_check(qkv, do, o, lse, delta, dqkv, 1, T, H, D, dtype, p, scale, SEED, STREAM, [(0, h) for h in range(H)], rstd=rstd,
                         what="fake", raise_on_fail=raise_on_fail)


# ------------------------------------------------------------------------------------------ the correct fake, the inputs
@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("D", [16, 64])
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("T", [96, 333])
def test_correct_fake_attention_passes(T, p, D, dtype):
    worst = run(T, D, dtype, p)
    assert max(worst[n] for n in AB.OUTPUTS + ("lse", "delta")) <= 1.0, worst


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_correct_fake_attention_with_rstd_rows_passes(p):
    worst = run(96, 64, BF16, p, ln=True)
    assert max(worst[n] for n in AB.OUTPUTS + ("lse", "delta")) <= 1.0, worst


CONDITION_GEOMETRIES = [(1, 96, 13, 16, 1), (1, 333, 13, 16, 1), (1, 333, 13, 64, 1), (1, 333, 13, 64, 0), (1, 333, 13, 128, 1), (1, 1024, 13, 16, 1),
                        (1, 1000, 13, 64, 1), (1, 2048, 13, 32, 1)]


@pytest.mark.parametrize("B,T,H,D,sflag", CONDITION_GEOMETRIES)
def test_planted_inputs_meet_their_conditions(B, T, H, D, sflag):
    """Partner probability in [0.1, 0.9] for at least 90 % of the rows that have a partner to share with (in every group, after the
    rounding to bf16), scores far from fp32 overflow, the float64 reference alone inside every limit, and q2 of both modes where the
    bound's derivation puts it."""
    scale = 1.0 / math.sqrt(D) if sflag else 1.0
    qkv, do = (stored(t, BF16) for t in AB.attn_inputs(B, T, H, D, scale, seed=T + D))
    assert bool(torch.isfinite(qkv.float()).all())
    qh, dh = AB.split_heads(qkv, do, B, T, H, D)
    assert float(np.abs(qh).max()) ** 2 * D * scale < 1e4                 # |q.k scale| <= that: nowhere near 3.4e38, or the -1e4 mask
    for g in range(H):
        ref = AB.attn_reference(qh[0, :, 0, g], qh[0, :, 1, g], qh[0, :, 2, g], dh[0, :, g], None, 0.0, scale)
        pp = AB.partner_probability(ref["P"], AB.OFFSETS[g % len(AB.OFFSETS)])
        assert float(((pp >= 0.1) & (pp <= 0.9)).mean()) >= 0.9, (g, float(pp.min()), float(np.median(pp)), float(pp.max()))
    g = H - 1
    q, k, v, d = qh[0, :, 0, g], qh[0, :, 1, g], qh[0, :, 2, g], dh[0, :, g]
    keep = AB.group_keep(SEED, STREAM, g, T, 0.2)
    own = AB.attn_reference(q, k, v, d, keep, 0.2, scale)                     # delta from the reference's OWN o
    # where the derivation puts q2.  bf16 mode: a few u.  fp32 mode, in units of u: a probability carries the rounding of its score, an fp32
    # chain of D products -- a random walk of D roundings of partial sums that A = sum_d |q_d k_d| scale bounds: sqrt(D) A, and as much
    # again from lse and the dP chain; then the accumulation of up to T summands in ONE chain -- sqrt(T) roundings of partial sums of a
    # few S2 on these peaked rows: 2 sqrt(T).  An emulation that rounds more than that would loosen every fp32 limit unnoticed.
    a_max = float((np.tril(np.abs(q) @ np.abs(k).T) * scale).max())
    q2_range = {BF16: (2.0, 6.0), FP32: (2.0, 2.0 * (math.sqrt(D) * a_max + math.sqrt(T)))}
    for dtype in (BF16, FP32):
        gb = AB.group_bounds(q, k, v, d, keep, 0.2, scale, dtype)
        lim = AB.attn_limits(gb["ref"], gb["s2"], gb["q2"], dtype, AB.f32_allowances(gb, gb["rho"], dtype))
        for n in AB.OUTPUTS:
            assert bool(np.isfinite(lim[n]).all()) and bool((lim[n] > 0).all()), (dtype, n)
            # the reference alone: with its own o in delta against with the o the emulation stored (what a kernel's check compares with)
            assert AB.within("reference", g, n, own[n], gb["ref"][n], lim[n]) <= 1.0
            lo, hi = q2_range[dtype]
            assert lo * AB.U[dtype] <= gb["q2"][n] <= hi * AB.U[dtype], (dtype, n, gb["q2"][n] / AB.U[dtype], hi)


# ------------------------------------------------------------------------------------------ the wrong fakes
def rejected(res, outputs):
    for n in outputs:
        msg = res["fails"].get(n)
        assert msg is not None, (n, {k: res[k] for k in AB.OUTPUTS + ("lse", "delta")})
        pos = r"row \d+" if n in ("lse", "delta") else r"row \d+, column \d+"
        assert re.match(r"fake: group \d+, %s, %s is \S+, reference \S+: error \S+ > limit " % (n, pos), msg), msg


WRONG = [  # bug, outputs that must reject it, (T, D, dtype, p), extra
    ("tail_key", ("o", "lse", "dq"), (333, 64, BF16, 0.2), {}),
    ("tail_key", ("o", "lse", "dq"), (333, 16, FP32, 0.0), {}),
    ("skip_subtile", ("o", "lse", "dq"), (333, 64, BF16, 0.2), {}),
    ("skip_subtile", ("o", "lse", "dq"), (96, 16, FP32, 0.0), {}),
    ("diag_wide", ("o", "lse"), (96, 64, BF16, 0.0), {}),
    ("diag_narrow", ("o", "lse"), (96, 64, BF16, 0.0), {}),
    ("no_rescale", ("o",), (96, 64, BF16, 0.0), {}),
    ("no_rescale", ("o",), (96, 16, FP32, 0.2), {}),
    ("hash_row_above", ("o",), (96, 64, BF16, 0.2), {}),
    ("no_keep_scale", ("o",), (96, 64, BF16, 0.2), {}),
    ("bf16_acc", ("o",), (1024, 64, BF16, 0.0), dict(H=1, inputs="randn")),
    ("lse_bf16", ("lse",), (96, 64, BF16, 0.0), {}),
    ("delta_neighbour", ("dq", "dk"), (96, 64, BF16, 0.2), {}),
    ("no_delta", ("dq", "dk"), (96, 64, BF16, 0.0), {}),
    ("dv_undropped", ("dv",), (96, 64, BF16, 0.2), {}),
    ("dkv_skip_block", ("dk", "dv"), (333, 64, BF16, 0.2), {}),
    ("dkv_skip_block", ("dk", "dv"), (96, 16, FP32, 0.0), {}),
    ("no_rstd", ("dq", "dk", "dv"), (96, 64, BF16, 0.2), dict(ln=True)),
]


@pytest.mark.parametrize("bug,outputs,shape,kw", WRONG, ids=["%s-%d-%d-%s-%.1f" % (w[0], *w[2][:2], "bf16" if w[2][2] else "fp32", w[2][3]) for w in WRONG])
def test_wrong_fake_attention_is_rejected(bug, outputs, shape, kw):
    T, D, dtype, p = shape
    rejected(run(T, D, dtype, p, bug=bug, raise_on_fail=False, **kw), outputs)
    with pytest.raises(AssertionError, match=r"fake: group \d+, \w+, row \d+.* > limit "):
        run(T, D, dtype, p, bug=bug, **kw)


def test_every_bug_of_the_fake_has_a_test():
    assert {w[0] for w in WRONG} == set(BUGS)


# ------------------------------------------------------------------------------------------ a dropped key moves everything
def without_key(ref, q, k, v, do, scale, j):
    """What deleting key j (invisible to every query; its own dK / dV rows gone) does to the float64 reference, in O(T D): with
    r_i = 1 / (1 - P_ij) for the rows i >= j that saw it,  P'_ij' = r_i P_ij',  o'_i = r_i (o_i - P~_ij v_j),  lse'_i = lse_i + ln(1 - P_ij),
    delta'_i = do_i . o'_i,  dq'_i = scale r_i (A_i - P_ij dP_ij k_j - delta'_i (C_i - P_ij k_j))  with  A = (P o dP) k,  C = P k.
    -> dict(o, lse, dq) of the changed rows' new values plus the index of those rows; dk'_j = dv'_j = 0."""
    P, Pt, dP = ref["P"], ref["Pt"], ref["dP"]
    rows = np.arange(max(j, 1), q.shape[0])             # (row 0 sees key 0 alone: without it there is no row)
    pj = P[rows, j]
    r = 1.0 / (1.0 - pj)
    o2 = r[:, None] * (ref["o"][rows] - Pt[rows, j][:, None] * v[j][None, :])
    d2 = (do[rows] * o2).sum(1)
    A, Cm = ref["_A"][rows], ref["_C"][rows]
    dq2 = scale * r[:, None] * (A - (pj * dP[rows, j])[:, None] * k[j][None, :] - d2[:, None] * (Cm - pj[:, None] * k[j][None, :]))
    return dict(rows=rows, o=o2, lse=ref["lse"][rows] + np.log1p(-pj), dq=dq2)


def test_the_closed_form_of_a_deleted_key_is_the_recomputed_reference():
    T, D, scale, p = 96, 16, 0.25, 0.2
    qkv, do = AB.attn_inputs(1, T, 2, D, scale, seed=5)
    qh, dh = AB.split_heads(qkv, do, 1, T, 2, D)
    q, k, v, d = qh[0, :, 0, 1], qh[0, :, 1, 1], qh[0, :, 2, 1], dh[0, :, 1]
    keep = AB.group_keep(SEED, STREAM, 1, T, p)
    ref = AB.attn_reference(q, k, v, d, keep, p, scale)
    ref["_A"], ref["_C"] = (ref["P"] * ref["dP"]) @ k, ref["P"] @ k
    for j in (0, 40, T - 1):
        got = without_key(ref, q, k, v, d, scale, j)
        # recompute with key j masked out of every row: an extra column pushes the scores of key j to -1e4, like a causally masked key
        qq = np.concatenate([q, np.zeros((T, 1))], 1)
        kk = np.concatenate([k, np.zeros((T, 1))], 1)
        qq[:, -1], kk[j, -1] = 1.0, -1e4 / scale
        ref2 = AB.attn_reference(qq, kk, v, d, keep, p, scale)
        rows = got["rows"]
        assert np.allclose(got["o"], ref2["o"][rows], rtol=1e-9, atol=1e-12) and np.allclose(got["lse"], ref2["lse"][rows], rtol=1e-12)
        assert np.allclose(got["dq"], ref2["dq"][rows][:, :D], rtol=1e-8, atol=1e-11)
        if j > 0:
            assert np.abs(ref2["dk"][j, :D]).max() < 1e-200 and np.abs(ref2["dv"][j]).max() < 1e-200


def gpu_geometries():
    """(dtype, T, D, scale flag, p) of every GPU case that runs planted inputs, once each."""
    out = []
    for table in (GB.TILE_EDGE_CASES, GB.ROWS_333_CASES, GB.KEY_SPLIT_ONE_CASES, GB.KEY_SPLIT_TWO_CASES, GB.LN_ROWS_CASES):
        out += [(dt, T, D, sf, p) for dt, B, T, H, D, sf in table for p in GB.P_DROP]
    out += [(dt, T, K.ATTN_FULL_LENGTH_BHD[2], 1, p) for dt, T, p in K.ATTN_FULL_LENGTH_CASES]
    out += [(dt, T, D, 1, p) for dt, B, H, D, T, p in K.ATTN_BLOCK_PLAN_CASES]
    out += [(BF16, T, D, 1, p) for B, H, D, T, p in K.ATTN_KEY_SPLIT_CASES]
    return sorted(set(out))


def test_a_dropped_key_moves_every_output_by_ten_limits():
    """Float64 only, no kernel.  On every geometry of the GPU cases (length, head size, dtype, scale, p; the planted inputs depend on
    the grid only through the group number mod 13, so one batch of 13 groups stands for it), for key 0, key T - 1, both sides of every
    multiple of 32 and 16 random keys: deleting the key puts some element of o, of dq, of dk and of dv, and some row of lse, at >= 10
    times its limit -- in group 0 (offset 0: every key is its own row's partner) and in one more group where the key is planted (it
    has a row j + off < T), rotating through the offsets.  dk and dv are judged on the deleted key's own row, which a kernel that does
    not see the key never accumulates.  The last key is seen by one row only, so its dk is ONE value of P (dP - delta): attn_inputs
    leans the last row's do on its own v so that this value is large on every geometry."""
    rng = np.random.default_rng(3)
    shortfalls = []
    for idx, (dtype, T, D, sflag, p) in enumerate(gpu_geometries()):
        if T == 1:
            continue                                          # (one key: deleting it leaves no row)
        scale = 1.0 / math.sqrt(D) if sflag else 1.0
        keys = sorted({0, T - 1} | {x for mlt in range(32, T, 32) for x in (mlt - 1, mlt)} | set(rng.integers(0, T, 16).tolist()))
        qkv, do = (stored(t, dtype) for t in AB.attn_inputs(1, T, len(AB.OFFSETS), D, scale, seed=T + D))
        qh, dh = AB.split_heads(qkv, do, 1, T, len(AB.OFFSETS), D)
        g2 = 1 + idx % (len(AB.OFFSETS) - 1)
        gbs = {}
        for g in (0, g2):
            gbs[g] = AB.group_bounds(qh[0, :, 0, g], qh[0, :, 1, g], qh[0, :, 2, g], dh[0, :, g], AB.group_keep(SEED, STREAM, g, T, p), p,
                                     scale, dtype)
        # q2, the lse floor and the fp32 allowances as attn_check takes them: the largest over the groups of the case (here the two looked at)
        rho = AB.case_rho(list(gbs.values()))
        q2 = {n: max(gb["q2"][n] for gb in gbs.values()) for n in AB.OUTPUTS}
        lse_lim = AB.f32_limit(max(gb["lse_floor"] for gb in gbs.values()), np.concatenate([gb["ref"]["lse"] for gb in gbs.values()]))
        for g in (0, g2):
            off = AB.OFFSETS[g]
            q, k, v, d = qh[0, :, 0, g], qh[0, :, 1, g], qh[0, :, 2, g], dh[0, :, g]
            gb = gbs[g]
            ref, lim = gb["ref"], AB.attn_limits(gb["ref"], gb["s2"], q2, dtype, AB.f32_allowances(gb, rho, dtype))
            ref["_A"], ref["_C"] = (ref["P"] * ref["dP"]) @ k, ref["P"] @ k
            for j in keys:
                if j != 0 and j + off > T - 1:
                    continue                                  # not planted in this group: no row has it as its partner
                new = without_key(ref, q, k, v, d, scale, j)
                rows = new["rows"]
                moved = dict(o=(np.abs(new["o"] - ref["o"][rows]) / np.maximum(lim["o"][rows], 1e-300)).max(),
                             dq=(np.abs(new["dq"] - ref["dq"][rows]) / np.maximum(lim["dq"][rows], 1e-300)).max(),
                             dk=(np.abs(ref["dk"][j]) / np.maximum(lim["dk"][j], 1e-300)).max(),
                             dv=(np.abs(ref["dv"][j]) / np.maximum(lim["dv"][j], 1e-300)).max(),
                             lse=np.abs(new["lse"] - ref["lse"][rows]).max() / lse_lim)
                # the one exemption: a key whose every (row, key) pair dropout removed (the last key, seen by one row) has P~ = 0 in its
                # whole column, so its dv row is identically zero with and without the key -- no input can make a kernel show that
                dv_is_zero = not ref["Pt"][:, j].any()
                for n, x in moved.items():
                    need = 0.0 if (n == "dv" and dv_is_zero) else 10.0
                    if not x >= need:
                        shortfalls.append((dtype, T, D, sflag, p, g, j, n, float(x)))
    assert not shortfalls, (len(shortfalls), shortfalls[:20])


# ------------------------------------------------------------------------------------------ the record
def test_old_metric_would_have_passed_a_skipped_tile():
    """What max |d| / max |ref| (3.6e-2 for o, 2e-2 for lse, 7.2e-2 for dq, dk, dv: tests/test_gpu_kernels.py) could not see: float64
    attention on bf16-rounded randn inputs, T = 1024, D = 64, with one 64-key tile invisible to the last 128-query block -- every output
    passes the old metric, while the same arrays fail the new limits on o, lse and dq by a wide margin."""
    T, D, scale = 1024, 64, 0.125
    qkv, do = (stored(t, BF16) for t in AB.randn_inputs(1, T, 1, D, seed=11))
    qh, dh = AB.split_heads(qkv, do, 1, T, 1, D)
    q, k, v, d = qh[0, :, 0, 0], qh[0, :, 1, 0], qh[0, :, 2, 0], dh[0, :, 0]
    ref = AB.attn_reference(q, k, v, d, None, 0.0, scale)
    # the faulty evaluation: queries 896 .. 1023 do not see keys 832 .. 895 (an extra column pushes those scores to -1e4)
    qq, kk = np.concatenate([q, np.zeros((T, 1))], 1), np.concatenate([k, np.zeros((T, 1))], 1)
    qq[896:, -1], kk[832:896, -1] = 1.0, -1e4 / scale
    bad = AB.attn_reference(qq, kk, v, d, None, 0.0, scale)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    old = dict(o=rel(bad["o"], ref["o"]), lse=rel(bad["lse"], ref["lse"]), dq=rel(bad["dq"][:, :D], ref["dq"]), dk=rel(bad["dk"][:, :D], ref["dk"]),
               dv=rel(bad["dv"], ref["dv"]))
    assert old["o"] < 3.6e-2 and old["lse"] < 2e-2 and max(old["dq"], old["dk"], old["dv"]) < 7.2e-2, old
    assert old["o"] > 1e-2 and old["dq"] > 1e-2, old                        # ... and not by being small: a third of the tolerance and more
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    dqkv = torch.cat([t(bad["dq"][:, :D]), t(bad["dk"][:, :D]), t(bad["dv"])], 1)
    res = AB.attn_check(qkv, do, t(bad["o"]), t(bad["lse"]), t((d * bad["o"]).sum(1)), dqkv, 1, T, 1, D, BF16, 0.0, scale, SEED, STREAM, [(0, 0)],
                        what="fake", raise_on_fail=False)
    rejected(res, ("o", "lse", "dq"))
    assert min(res["o"], res["dq"]) > 10.0 and res["lse"] > 100.0, res
