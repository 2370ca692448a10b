"""Checks for the embedding kernels of composer_amd/csrc/elementwise.hip (forward, forward with partial statistics, the three forms of
the backward pass) and for the atomic-free column sums: float64 references, float32 emulations that round where the kernels round, the
bounds the two give, and `embed_fwd_check` / `embed_stats_check` / `embed_bwd_check` / `colsum_det_check`, which hold the arrays of one
launch to all of it.  numpy and torch on the CPU; no GPU, no library.  Every element is checked: no sampling, no share left out.

Forward.  The result is exactly determined: wte[id] + wpe[pos] in fp32 (then + wte[type], in the written order (a + p) + t), one multiply
by the float32 scale 1 / (1 - p) where the mask keeps the element (+0 where it does not), one round-to-nearest-even to bf16.  It is held
BIT FOR BIT to `embed_fwd_emulation` (integer views: a -0.0 or a NaN counts).

Partial statistics.  (mean, M2) of every 256-column segment against float64 of the STORED bf16 values, the fp32 idiom of row_bounds:
floor = max |float32 emulation - float64| over the case, relative to mean_e |x| for a mean and to the value itself for an M2;
limit = F32_MARGIN floor + F32_ABS (row_bounds.f32_limits).  Two emulations, the larger floor counts: the kernel's order (eight values in a lane, five xor rounds
over the half-wave, two passes, the squares through an fma) and a strictly sequential sum (the worst case).

dwte.  Per element  limit = MARGIN max(q, u) S,  S = S2 + |ref|,  S2 = sqrt(start^2 + sum t^2) over the rows of that id: the
accumulating-sum bound row_bounds derives for dgamma / dbeta / colsum.  The float64 reference takes the stored dh times keep times the
float32 scale.  q is the largest |emulation - reference| / S over the case, from an fp32 emulation of the form's own tree (the summand
is the ROUNDED product dh * scale: both roundings are in q), never from a kernel:
    atomic       one add per token, under the N_ORDERS arrival orders of row_bounds.atomics_fold (`arrival`)
    sorted       the tokens of an id in N_ORDERS orders (the order within a token block comes from LDS atomics: not defined), cut into
                 chunks of 128; in a chunk thread group rs sums the rows rs, rs + RP, ... and the RP groups are folded in order; one
                 atomic per chunk, each token order again under N_ORDERS arrival orders (100 runs: with bf16 gradients the chunk sums
                 are nearly exact, the error is the five or six atomics of a hot id alone, and it takes few distinct values -- under
                 ten runs q of the V = 8192 case came to 1.0 u, under a hundred to 1.7 u, and the kernel's own order gave 2.0 u)
    atomic-free  fully defined: 64 token segments in token order, a fold over the 64 in order, then +=
An id that never occurs keeps its start value bit for bit.

dwpe, the atomic-free dwte, the atomic-free column sums.  No atomics: the order is defined (sequential over the batch in
embed_bwd_kernel / embed_bwd_wpe_kernel; pairs (b, b + RP) with stride 2 RP, then the group fold, in embed_wpe_sum_kernel; in
colsum_kernel the wave's (v0 + v1) + (v2 + v3) groups, the tail, the four-wave fold, the splits in order).  At p = 0 they are held BIT FOR
BIT to the emulation.  At p > 0 the compiler may contract acc += v * scale into an fma (one rounding where the emulation has two), so
there they are held to the bound above.  Rows of dwpe outside [pos0, pos0 + T) are untouched bit for bit.  The column sums are also held
to kernel_arena.colsum_bound against float64, which checks the emulation itself.

`reach_*` write out the launcher's arithmetic: which form, CPR, RP, idle threads, trips of every loop a case is meant to reach.
"""
import numpy as np
import torch

from attention_bounds import MARGIN, BF16
from row_bounds import seq_sum32, store, A64, N_ORDERS, U, _q, f32_limits, within, raise_first, parts_of, drop_scale
from kernel_arena import colsum_bound, assert_within
from oracle.transformer_oracle import dropout_keep_rows

f32 = np.float32
EMB_CH, EMB_SEG, EMB_NB = 128, 64, 64          # elementwise.hip


def cdiv(a, b):
    return -(-a // b)


def A32(a):
    """Values as float32 numpy (a bf16 tensor widened: exact)."""
    if torch.is_tensor(a):
        a = a.detach().cpu().float().numpy()
    return np.ascontiguousarray(a, dtype=f32)


def bits(a):
    return A32(a).view(np.uint32)


def same_bits(what, name, out, want, fails=None):
    """Bit equality of two float arrays (fp32 views; bf16 values widen exactly) -> 0.0, or inf and a message."""
    o, w = bits(out), bits(want)
    assert o.shape == w.shape, (what, name, o.shape, w.shape)
    bad = o != w
    if bool(bad.any()):
        idx = tuple(int(i) for i in np.argwhere(bad)[0])
        msg = "%s: %s, element %s is %.9g (0x%08x), must be bit for bit %.9g (0x%08x) (%d of %d elements differ)" % (
            what, name, idx, A32(out)[idx], o[idx], A32(want)[idx], w[idx], int(bad.sum()), bad.size)
        if fails is None:
            raise AssertionError(msg)
        fails.setdefault(name, msg)
        return float("inf")
    return 0.0


def keep_of(ntok, E, p, seed, stream):
    """The mask of dropout site 0 with the threshold the kernels use: p as the float32 the ABI receives (common.h: drop_threshold)."""
    return dropout_keep_rows(seed, stream, ntok, E, float(f32(p))) if p > 0 else None


# ================================================================================================================ forward
def embed_rows(ids, wte, wpe, T, pos0, pos_ids=None, type_ids=None):
    """The fp32 rows a token's sum is made of: wte[id], wpe[pos] (pos = pos_ids or pos0 + t), wte[type] or None."""
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    wte, wpe = A32(wte), A32(wpe)
    pos = pos0 + np.arange(ids.size) % T if pos_ids is None else np.asarray(pos_ids).reshape(-1).astype(np.int64)
    ty = None if type_ids is None else wte[np.asarray(type_ids).reshape(-1).astype(np.int64)]
    return wte[ids], wpe[pos], ty


def embed_fwd_emulation(ids, wte, wpe, T, pos0, dtype, p=0.0, seed=0, stream=0, pos_ids=None, type_ids=None):
    """embed_fwd_kernel / embed_fwd_stats_kernel: (a + p) (+ t) in fp32, times the float32 scale where kept, one rounding -> values as stored."""
    a, pz, ty = embed_rows(ids, wte, wpe, T, pos0, pos_ids, type_ids)
    v = a + pz
    if ty is not None:
        v = v + ty
    if p > 0:
        v = np.where(keep_of(v.shape[0], v.shape[1], p, seed, stream), v * drop_scale(p), f32(0))
    return store(v, dtype)


def embed_fwd_check(dtype, out, ids, wte, wpe, T, pos0, p=0.0, seed=0, stream=0, pos_ids=None, type_ids=None, what="embed_fwd", fails=None):
    return same_bits(what, "out", out, embed_fwd_emulation(ids, wte, wpe, T, pos0, dtype, p, seed, stream, pos_ids, type_ids), fails)


def _butterfly32(a):
    """Five xor rounds (16, 8, 4, 2, 1) over the 32 lanes of the last axis, in float32: every lane ends with the total."""
    lane = np.arange(32)
    for o in (16, 8, 4, 2, 1):
        a = a + a[..., lane ^ o]
    return a[..., 0]


def stats_emulations(x):
    """(mean, M2) [rows, E / 256, 2] of the stored values in float32, two ways: the kernel's order and strictly sequential."""
    x = A32(x)
    seg = x.reshape(x.shape[0], x.shape[1] // 256, 32, 8)
    mu = _butterfly32(seq_sum32(seg)) * f32(1.0 / 256.0)
    d = seg - mu[..., None, None]
    q = np.zeros(seg.shape[:-1], dtype=f32)
    for j in range(8):
        q = (d[..., j].astype(np.float64) ** 2 + q.astype(np.float64)).astype(f32)          # fmaf(d, d, q): d * d is exact in float64
    kern = np.stack([mu, _butterfly32(q)], -1)
    flat = x.reshape(x.shape[0], x.shape[1] // 256, 256)
    mu_s = seq_sum32(flat) / f32(256.0)
    ds = flat - mu_s[..., None]
    return kern, np.stack([mu_s, seq_sum32(ds * ds)], -1)


def embed_stats_check(out, part, ids, wte, wpe, T, pos0, p=0.0, seed=0, stream=0, what="embed_fwd_stats", raise_on_fail=True):
    """cmp_k_embed_fwd_stats: the rows bit for bit, the partials per element against float64 of the rows as STORED."""
    worst, q, fails = {}, {}, {}
    worst["out"] = embed_fwd_check(BF16, out, ids, wte, wpe, T, pos0, p, seed, stream, what=what, fails=fails)
    x = A32(out)
    ref = parts_of(x)
    part = A64(part).reshape(ref.shape)
    size = np.stack([np.abs(x.astype(np.float64)).reshape(ref.shape[0], ref.shape[1], 256).mean(-1), ref[..., 1]], -1)
    for k, n in enumerate(("mean", "M2")):
        lims = [f32_limits(e[..., k], ref[..., k], size[..., k]) for e in stats_emulations(x)]
        lim, q[n] = max(lims, key=lambda lf: lf[1])
        worst[n] = within(what, n, part[..., k], ref[..., k], lim, fails)
    res = dict(worst=worst, q=q, fails=fails)
    if raise_on_fail:
        raise_first(res)
    return res


# ================================================================================================================ backward: summands, bound
def summands(dh, p=0.0, seed=0, stream=0, keep=None):
    """-> (t32, t64): the kernel's fp32 summand (dh * scale ROUNDED, +0 where dropped) and the float64 one (stored dh times keep times the
    float32 scale, unrounded).  keep: a mask to use in place of the oracle's (the host test's planted bugs)."""
    d = A32(dh)
    if p <= 0:
        return d, d.astype(np.float64)
    if keep is None:
        keep = keep_of(d.shape[0], d.shape[1], p, seed, stream)
    sc = drop_scale(p)
    return np.where(keep, d * sc, f32(0)), np.where(keep, d.astype(np.float64) * float(sc), 0.0)


def acc_ref(start, t64, index=None):
    """Rows of t64 added onto `start` (row index[k] for summand k; None: all onto the rows in place, t64 [n, rows, E]) ->
    float64 reference and S = sqrt(start^2 + sum t^2) + |ref|."""
    s = torch.from_numpy(A64(start).copy())
    s2 = s * s
    t = torch.from_numpy(np.ascontiguousarray(t64))
    if index is None:
        ref, s2 = s + t.sum(0), s2 + (t * t).sum(0)
    else:
        ix = torch.from_numpy(np.asarray(index, dtype=np.int64))
        ref = s.index_add(0, ix, t)
        s2 = s2.index_add(0, ix, t * t)
    return ref.numpy(), (s2.sqrt() + ref.abs()).numpy()


def arrival(n, order, rng=None):
    """The arrival orders of row_bounds.atomics_fold: 0 ascending, 1 descending, k the permutation of seed k."""
    if order == 0:
        return np.arange(n)
    if order == 1:
        return np.arange(n)[::-1]
    return (rng if rng is not None else np.random.default_rng(order)).permutation(n)


def fold_by_id(acc, ids, rows, seq):
    """acc[ids[k]] += rows[k] for k = seq[0], seq[1], ... one after the other, in float32 (vectorised: the j-th addend of every id at once)."""
    seq = np.asarray(seq, dtype=np.int64)
    if seq.size == 0:
        return acc
    key = np.asarray(ids)[seq]
    o = np.argsort(key, kind="stable")
    sk = key[o]
    first = np.r_[0, np.flatnonzero(np.diff(sk)) + 1]
    counts = np.diff(np.r_[first, sk.size])
    rank = np.arange(sk.size) - np.repeat(first, counts)
    by = np.argsort(rank, kind="stable")
    edge = np.searchsorted(rank[by], np.arange(int(counts.max()) + 1))
    for j in range(int(counts.max())):
        sel = seq[o[by[edge[j]:edge[j + 1]]]]
        acc[ids[sel]] = acc[ids[sel]] + rows[sel]
    return acc


def rp_of(E, dtype):
    """CPR (16-byte chunks per row), RP (rows side by side) of embed_segsum_kernel / embed_wpe_sum_kernel."""
    cpr = E // (8 if dtype == BF16 else 4)
    return cpr, (1 if cpr >= 256 else 256 // cpr)


# ================================================================================================================ backward: inputs
PLANTED = ((1, 0), (2, 1), (3, 127), (4, 128), (5, 129))          # (id, tokens) where the vocabulary has room: both sides of a chunk


def planted_ids(ntok, V, seed):
    """ids [ntok] int32 at shuffled positions.  V >= 8: ids 1 .. 5 occur exactly 0, 1, 127, 128, 129 times (PLANTED), ids 0 and V - 1
    occur, half of the rest goes to the hot ids 0, 6, 7 and half anywhere but 1 .. 5.  3 <= V < 8: ids 1 and 2 occur 128 and 129 times,
    the rest is id 0 (and V - 1 once).  Short streams (ntok < 1024) and V < 3: uniform draws with ids 0 and V - 1 present."""
    rng = np.random.default_rng(seed)
    if V < 3 or ntok < 1024:
        ids = rng.integers(0, V, ntok)
        ids[0], ids[-1] = 0, V - 1
        return ids.astype(np.int32)
    if V >= 8:
        fixed = np.concatenate([np.full(n, v) for v, n in PLANTED] + [np.array([0, V - 1])])
        rest = ntok - fixed.size
        free = np.concatenate([[0], np.arange(6, V)])
        hot = rng.random(rest) < 0.5
        body = np.where(hot, rng.choice(np.array([0, 6, 7]), rest), rng.choice(free, rest))
    else:
        fixed = np.concatenate([np.full(128, 1), np.full(129, 2), np.array([V - 1] if V > 3 else [], dtype=np.int64)])
        body = np.zeros(ntok - fixed.size, dtype=np.int64)
    ids = np.concatenate([fixed, body])
    return ids[rng.permutation(ntok)].astype(np.int32)


def bwd_inputs(B, T, E, V, dtype, pos0, seed):
    """-> ids [B * T] int32 (planted_ids), dh [B * T, E] as stored, the non-zero start values dwte0 [V, E], dwpe0 [pos0 + T, E]."""
    rng = np.random.default_rng(seed + 1)
    return dict(ids=planted_ids(B * T, V, seed), dh=store(rng.normal(0, 1.0, (B * T, E)), dtype),
                dwte0=rng.normal(0, 3.0, (V, E)).astype(f32), dwpe0=rng.normal(0, 3.0, (pos0 + T, E)).astype(f32))


# ================================================================================================================ backward: emulations
def dwte_atomic_emulation(ids, t32, start, order=0):
    """embed_bwd_kernel: one atomic per token and element."""
    return fold_by_id(A32(start).copy(), ids, t32, arrival(ids.size, order))


def sorted_chunks(ids, V, order=0, tamper=None):
    """The counting sort: the tokens of every id (in the order `order` gives them), cut into chunks of EMB_CH ->
    chunk ids [nchunks], token indices [nchunks, EMB_CH] (-1: none).  tamper(v, tokens) -> tokens: the host test's planted bugs."""
    o = np.argsort(ids, kind="stable")
    counts = np.bincount(ids, minlength=V)
    starts = np.r_[0, np.cumsum(counts)]
    rng = np.random.default_rng(order)
    cid, rows = [], []
    for v in np.flatnonzero(counts):
        toks = o[starts[v]:starts[v + 1]]
        toks = toks[arrival(toks.size, order, rng)]
        if tamper is not None:
            toks = tamper(int(v), toks)
        for c0 in range(0, toks.size, EMB_CH):
            cid.append(v)
            rows.append(toks[c0:c0 + EMB_CH])
    mat = np.full((len(rows), EMB_CH), -1, dtype=np.int64)
    for k, r in enumerate(rows):
        mat[k, :r.size] = r
    return np.asarray(cid, dtype=np.int64), mat


def chunk_partials(mat, t32, RP):
    """embed_segsum_kernel up to its atomics: thread group rs chains the chunk's rows rs, rs + RP, ...; the groups are folded in order."""
    tz = np.concatenate([t32, np.zeros((1, t32.shape[1]), dtype=f32)])           # index -1: a zero row (x + 0 is exact)
    ng = min(RP, EMB_CH)
    G = np.zeros((mat.shape[0], ng, t32.shape[1]), dtype=f32)
    for j in range(EMB_CH):
        if not (mat[:, j] >= 0).any():
            break
        G[:, j % RP] = G[:, j % RP] + tz[mat[:, j]]
    acc = G[:, 0].copy()
    for g in range(1, ng):
        acc = acc + G[:, g]
    return acc


def dwte_sorted_parts(ids, t32, V, dtype, order=0, tamper=None, round_partial=None):
    """The addends of the sorted form's atomics with the tokens of every id in the order `order`: chunk ids, chunk partials."""
    cid, mat = sorted_chunks(ids, V, order, tamper)
    parts = chunk_partials(mat, t32, rp_of(t32.shape[1], dtype)[1])
    return cid, (parts if round_partial is None else round_partial(parts))


def dwte_sorted_emulation(ids, t32, start, dtype, order=0, tamper=None, round_partial=None, arrive=None):
    """The sorted form: token order `order`, the chunks' atomics in the arrival order `arrive` (default: the same index)."""
    start = A32(start)
    cid, parts = dwte_sorted_parts(ids, t32, start.shape[0], dtype, order, tamper, round_partial)
    return fold_by_id(start.copy(), cid, parts, arrival(cid.size, order if arrive is None else arrive))


def dwte_emulations(form, ids, t32, start, dtype):
    """Every run of the form's emulation that q is taken over: N_ORDERS arrival orders of the atomic form; for the sorted form N_ORDERS
    token orders, each under N_ORDERS arrival orders of its chunks' atomics; the one defined order of the atomic-free form."""
    start = A32(start)
    if form == 2:
        yield dwte_det_emulation(ids, t32, start)
    elif form == 0:
        for k in range(N_ORDERS):
            yield dwte_atomic_emulation(ids, t32, start, k)
    else:
        for k in range(N_ORDERS):
            cid, parts = dwte_sorted_parts(ids, t32, start.shape[0], dtype, k)
            for j in range(N_ORDERS):
                yield fold_by_id(start.copy(), cid, parts, arrival(cid.size, j))


def dwte_det_emulation(ids, t32, start):
    """embed_bwd_det_part_kernel + embed_bwd_det_reduce_kernel: EMB_SEG token segments in token order, folded in order, then +=."""
    start = A32(start)
    ntok, E = t32.shape
    per = cdiv(ntok, EMB_SEG)
    part = np.zeros((start.shape[0], EMB_SEG, E), dtype=f32)
    g = np.arange(EMB_SEG)
    for s in range(per):
        tok = g * per + s
        ok = tok < ntok
        part[ids[tok[ok]], g[ok]] = part[ids[tok[ok]], g[ok]] + t32[tok[ok]]
    a = np.zeros_like(start)
    for k in range(EMB_SEG):
        a = a + part[:, k]
    return start + a


def dwte_emulation(form, ids, t32, start, dtype, order=0):
    if form == 0:
        return dwte_atomic_emulation(ids, t32, start, order)
    if form == 1:
        return dwte_sorted_emulation(ids, t32, start, dtype, order)
    return dwte_det_emulation(ids, t32, start)


def dwpe_seq_emulation(t32, B, T, start_rows):
    """embed_bwd_kernel / embed_bwd_wpe_kernel: the batch in order."""
    t = t32.reshape(B, T, -1)
    acc = np.zeros(t.shape[1:], dtype=f32)
    for b in range(B):
        acc = acc + t[b]
    return A32(start_rows) + acc


def dwpe_pairs_emulation(t32, B, T, start_rows, dtype, tail_bug=False):
    """embed_wpe_sum_kernel: thread group rs takes the pairs (b, b + RP) for b = rs, rs + 2 RP, ...; the groups are folded in order.
    tail_bug: a pair whose second row is past the batch adds its first row again (the host test's planted bug)."""
    t = t32.reshape(B, T, -1)
    RP = rp_of(t.shape[2], dtype)[1]
    tot = None
    for rs in range(min(RP, B)):                       # (the groups past the batch hold zeros)
        acc = np.zeros(t.shape[1:], dtype=f32)
        for b in range(rs, B, 2 * RP):
            x1 = t[b + RP] if b + RP < B else (t[b] if tail_bug else np.zeros_like(acc))
            acc = acc + (t[b] + x1)
        tot = acc if tot is None else tot + acc
    return A32(start_rows) + tot


def dwpe_emulation(form, t32, B, T, start_rows, dtype):
    return dwpe_pairs_emulation(t32, B, T, start_rows, dtype) if form == 1 else dwpe_seq_emulation(t32, B, T, start_rows)


# ================================================================================================================ backward: the check
def embed_bwd_check(form, dtype, ids, dh, B, T, pos0, p, seed, stream, dwte0, dwpe0, dwte, dwpe, what="embed_bwd", raise_on_fail=True):
    """The arrays of one launch of the form `form` (0 atomic, 1 sorted, 2 atomic-free): dh [B * T, E] as stored, the start values and the
    results of dwte [V, E] and dwpe [W, E].  -> dict(worst, q, fails)."""
    worst, q, fails = {}, {}, {}
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    dwte0, dwpe0 = A32(dwte0), A32(dwpe0)
    V = dwte0.shape[0]
    t32, t64 = summands(dh, p, seed, stream)
    # ---- dwte
    ref, S = acc_ref(dwte0, t64, ids)
    q["dwte"] = max(_q(e, ref, S) for e in dwte_emulations(form, ids, t32, dwte0, dtype))
    if form == 2 and p == 0:
        worst["dwte"] = same_bits(what, "dwte", dwte, dwte_det_emulation(ids, t32, dwte0), fails)
    else:
        worst["dwte"] = within(what, "dwte", dwte, ref, MARGIN * max(q["dwte"], U) * S, fails)
    absent = np.bincount(ids, minlength=V) == 0
    if absent.any():
        worst["absent"] = same_bits(what, "dwte rows of ids that never occur", A32(dwte)[absent], dwte0[absent], fails)
    # ---- dwpe
    rows = slice(pos0, pos0 + T)
    refp, Sp = acc_ref(dwpe0[rows], t64.reshape(B, T, -1))
    emu = dwpe_emulation(form, t32, B, T, dwpe0[rows], dtype)
    q["dwpe"] = _q(emu, refp, Sp)
    if p == 0:
        worst["dwpe"] = same_bits(what, "dwpe", A32(dwpe)[rows], emu, fails)
    else:
        worst["dwpe"] = within(what, "dwpe", A32(dwpe)[rows], refp, MARGIN * max(q["dwpe"], U) * Sp, fails)
    out = np.ones(dwpe0.shape[0], dtype=bool)
    out[rows] = False
    if out.any():
        worst["outside"] = same_bits(what, "dwpe rows outside [pos0, pos0 + T)", A32(dwpe)[out], dwpe0[out], fails)
    res = dict(worst=worst, q=q, fails=fails)
    if raise_on_fail:
        raise_first(res)
    return res


# ================================================================================================================ atomic-free column sums
def colsum_splits(rows, cols, dtype):
    gx = cdiv(cols, 64 * (8 if dtype == BF16 else 4))
    return max(1, min(min(rows // 64, 128), max(1, 1024 // gx)))


def colsum_det_emulation(x, start, dtype):
    """colsum_kernel with `part` + colsum_fold_kernel: per split, wave w chains (x[r] + x[r + 4]) + (x[r + 8] + x[r + 12]) from r = r0 + w in
    steps of 16 while r + 12 < r1, then single rows in steps of 4; the four waves are folded in order, the splits in order, then +=."""
    x = A32(x)
    rows, cols = x.shape
    splits = colsum_splits(rows, cols, dtype)
    per = cdiv(rows, splits)
    tot = np.zeros(cols, dtype=f32)
    for s in range(splits):
        r0, r1 = s * per, min(rows, s * per + per)
        v = None
        for w in range(4):
            acc = np.zeros(cols, dtype=f32)
            r = r0 + w
            while r + 12 < r1:
                acc = acc + ((x[r] + x[r + 4]) + (x[r + 8] + x[r + 12]))
                r += 16
            while r < r1:
                acc = acc + x[r]
                r += 4
            v = acc if v is None else v + acc
        tot = tot + v
    return A32(start) + tot


def colsum_det_check(dtype, x, start, out, what="colsum_det"):
    """cmp_k_colsum_det: bit for bit the emulation, and inside kernel_arena.colsum_bound of the float64 sum.  -> error / limit of the latter."""
    same_bits(what, "out", out, colsum_det_emulation(x, start, dtype))
    ref, S, factor = colsum_bound(torch.from_numpy(A64(x)), torch.from_numpy(A64(start)))
    return assert_within(torch.from_numpy(A32(out)), ref, factor * S, False, what)


# ================================================================================================================ the launcher's arithmetic
def reach_embed_bwd(B, T, E, dtype, V, sort_ws_words, det=False):
    """embed_bwd_run -> dict: form (0 atomic, 1 sorted, 2 atomic-free); for the sorted form CPR, RP, idle threads of a workgroup, trips
    of the c0 loop, `per` of embed_scan2_kernel; for the atomic-free form `per` and the segments without a token."""
    ntok, vn = B * T, (8 if dtype == BF16 else 4)
    if det and V > 0:
        per = cdiv(ntok, EMB_SEG)
        return dict(form=2, per=per, empty=EMB_SEG - cdiv(ntok, per))
    need = sort_ws_words_of(ntok, V)
    if V > 0 and need > 0 and sort_ws_words >= need and ntok >= 4096 and E % vn == 0 and ntok < 2 ** 31:
        cpr, rp = rp_of(E, dtype)
        return dict(form=1, CPR=cpr, RP=rp, idle=256 - rp * cpr if rp > 1 else max(0, 256 * cdiv(cpr, 256) - cpr), trips=cdiv(cpr, 256),
                    scan_per=cdiv(V, 1024))
    return dict(form=0)


def sort_ws_words_of(ntok, V):
    """embed_bwd_sort_ws_words."""
    if V <= 0 or V > 8192:
        return 0
    return 16 + 2 * EMB_NB * V + V + 2 * (V + 1) + (ntok // EMB_CH + V + 1) + ntok + 16


def reach_embed_fwd(ntok, E, dtype):
    """embed_fwd_run -> (grid, trips of the grid-stride loop)."""
    total = ntok * (E // (8 if dtype == BF16 else 4))
    grid = min(cdiv(total, 256), 4096)
    return grid, cdiv(total, grid * 256)


def reach_embed_stats(ntok, E):
    """embed_fwd_stats_run -> (MAXI, trips of the row loop, a ragged last slot)."""
    grid, maxi = min(cdiv(ntok, 4), 8192), cdiv(E // 8, 64)
    return (1 if maxi == 1 else 2 if maxi == 2 else 4), cdiv(ntok, 4 * grid), (E // 8) % 64 != 0


def reach_colsum(rows, cols, dtype):
    """colsum_run -> (splits, rows per split, splits without a row, the split count is the column grid's cap 1024 / gx)."""
    gx = cdiv(cols, 64 * (8 if dtype == BF16 else 4))
    splits = colsum_splits(rows, cols, dtype)
    per = cdiv(rows, splits)
    return splits, per, splits - cdiv(rows, per), splits == max(1, 1024 // gx) and splits < min(rows // 64, 128)
