"""Per-element error bounds for the row kernels of composer_amd/csrc/elementwise.hip: the LayerNorm family (forward, backward with its
fused prologue, the prescaled form, ln_stats_merge, wgrad_ln_fix) and the fused softmax cross-entropy.
float64 references written out, float32 emulations that round where the kernels round, the bounds the two give, planted inputs, and
`ln_check` / `xent_check`, which hold the arrays of one launch to all of it.  numpy and torch on the CPU; no GPU, no library.

Bound, per element, in the idiom of tests/attention_bounds.py:

    limit = MARGIN max(q, u) S  (+ BF16_OUT |reference| for a bf16 store),       MARGIN = 2 (attention_bounds), BF16_OUT = 2^-8 (kernel_arena)
    q     = max over the case of |emulation in front of the store - reference| / S, measured on the CPU from the emulations below,
            never from a kernel
    u     = 2^-24 in BOTH modes: the row kernels widen a bf16 operand on load and compute in fp32; bf16 enters only through the values
            as stored (the references read those) and the final store (the BF16_OUT term)

S is the size on which an fp32 evaluation of the element is resolved:

    y            |gamma_e| rstd_r (|x_re| + |mu_r|) + |beta_e| + |y_re|                 (|mu|: the cancellation in x - mu)
    dx           rstd (|g| + A1 + |xhat| A2 + rstd (|x| + |mu|) |s2|) + |resid| + |dx|,   g = dy gamma, A1 = mean_e |g|,
                 A2 = mean_e |g| rstd (|x| + |mu|): s1 and s2 are sums of E terms of those sizes, and xhat carries the cancellation of
                 x - mu both where it multiplies s2 and inside s2.  (The issue's starting form rstd (|g| + |s1| + |xhat s2|) + |resid|
                 has the VALUES of s1 and s2 where their summands' sizes belong: on rows whose s1 or s2 cancels the emulation's q
                 ran to 27 .. 223 u on the GPU geometries, against 0.6 .. 4.3 u with the sizes; |dx| is the result's own rounding.)
    dgamma, dbeta, colsum    S2 + |ref|: the quadrature sum S2 = sqrt(start^2 + sum_r t_r^2) of the summands t_r = dy xhat, dy, dmask (the
                 roundings of a long fp32 sum are independent draws) plus the size of the result itself.  The issue's starting form is S2
                 alone; the emulation shows what it misses: every atomic rounds the ACCUMULATOR, so the error comes in ulps of the result
                 (1 to 2 of them under any arrival order) whatever the summands, and in a column whose sum is coherent, |ref| = 3.5 S2 in one
                 of 1024, two ulps of the result are 12 u S2 where the summands' own q is 5 u.  The all-absolute sum is ~100 times looser at
                 these row counts and is not used.
    dlogits      inv_n (p_c (1 + |z_c| + |lse|) + [c = y])                               (the error of lse scales with |lse|)
    wgrad_ln_fix |gamma_k| (|G_kj| + 2 mean_k' |G_k'j|) + |beta_k colsum_j| + |ref_kj|   (the column mean is a sum of `rows` terms)

mean, rstd (fp32 in both modes), the merged statistics and the per-row loss get the fp32 idiom of tests/test_gpu_decode_logits.py:
floor = max |float32 restatement - float64| over the case, limit = 4 floor + 1e-6 -- with both taken RELATIVE to the element's natural
size (mean_e |x_re| for a row's mean, the reference itself for rstd, |lse_r| + |z_ry| for a loss), so that a row of small values is
not given what a row of large ones needs.  dmask is exact: the STORED dx times keep / (1 - p) in fp32, rounded once.  row_correct is exact
(ties go to the lowest column).  Padding columns of dlogits are exactly zero.

Emulations.  LayerNorm rows and cross-entropy rows: a strictly sequential fp32 row sum, the worst order a wave reduction can take.  Parameter
gradients: the kernel's own tree -- per-wave chains over the rows w, w + stride, ..., the 4-wave fold of a workgroup, then either `grid`
atomics onto the accumulator or 32 slices p, p + 32, ... of the partials and 32 atomics (`param_partials`), the atomics under ten
arrival orders (`atomics_fold`: their order is not defined; q is the largest over the ten).  All of it is
vectorised over rows, so q is measured on EVERY row of a case, also at 65539 rows: no sampling.
"""
import numpy as np
import torch

from attention_bounds import MARGIN, U as _U, FP32, BF16, bf16r, F32_MARGIN, F32_ABS
from kernel_arena import BF16_OUT

U = _U[FP32]
f32 = np.float32
EPS = 1e-5
LN_KINDS = ("off0.5", "off24", "off300", "const", "zero", "outlier", "off0.5", "off24")     # row r is of kind LN_KINDS[r % 8]
SEG_SHARE_MIN = 0.3           # planted per-segment offsets: the between-segment term is at least this share of a random row's M2
XENT_TARGET = 0.4
XENT_SPREAD = 3.0
SHIFT = 80.0


def A64(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().double().numpy() if a.dtype.is_floating_point else a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def store(a, dtype):
    """fp32 -> the launch's dtype -> fp32."""
    a = np.ascontiguousarray(a, dtype=f32)
    return bf16r(a) if dtype == BF16 else a


def seq_sum32(a):
    """Sum over the last axis in float32, strictly in order."""
    a = np.asarray(a, dtype=f32)
    acc = np.zeros(a.shape[:-1], dtype=f32)
    for e in range(a.shape[-1]):
        acc = acc + a[..., e]
    return acc


# ================================================================================================================ LayerNorm: references
def ln_fwd_ref(x, gamma, beta, eps=EPS):
    x, gamma, beta = A64(x), A64(gamma), A64(beta)
    mu = x.mean(-1)
    var = ((x - mu[:, None]) ** 2).mean(-1)
    rs = 1.0 / np.sqrt(var + eps)
    return dict(mean=mu, rstd=rs, y=(x - mu[:, None]) * rs[:, None] * gamma + beta)


def merge_ref(part, eps=EPS):
    """[rows][np][2] partials (mean, M2 per 256-column segment) -> mean, rstd, and the share of the between-segment term in M2."""
    part = A64(part)
    npart = part.shape[1]
    mu = part[:, :, 0].mean(-1)
    between = 256.0 * ((part[:, :, 0] - mu[:, None]) ** 2).sum(-1)
    m2 = part[:, :, 1].sum(-1) + between
    return dict(mean=mu, rstd=1.0 / np.sqrt(m2 / (256.0 * npart) + eps), share=between / np.maximum(m2, 1e-300))


def parts_of(x):
    """(mean, M2) of every 256-column segment of every row of the values as stored: float64 [rows, E / 256, 2]."""
    x = A64(x)
    seg = x.reshape(x.shape[0], x.shape[1] // 256, 256)
    mu = seg.mean(-1)
    return np.stack([mu, ((seg - mu[..., None]) ** 2).sum(-1)], -1)


def ln_bwd_ref(dy, x, gamma, mean, rstd, resid=None, prescaled=False):
    """dx = resid + rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma, on the statistics GIVEN (the arrays the kernel reads);
    prescaled: dy holds rstd o gradient.  Also the summands of dgamma (dy xhat) and dbeta (dy)."""
    dy, x, gamma, mu, rs = A64(dy), A64(x), A64(gamma), A64(mean)[:, None], A64(rstd)[:, None]
    if prescaled:
        dy = dy / rs
    xh = (x - mu) * rs
    g = dy * gamma
    s1, s2 = g.mean(-1, keepdims=True), (g * xh).mean(-1, keepdims=True)
    dx = rs * (g - s1 - xh * s2)
    r = 0.0 if resid is None else A64(resid)
    A1 = np.abs(g).mean(-1, keepdims=True)
    cx = rs * (np.abs(x) + np.abs(mu))
    A2 = (np.abs(g) * cx).mean(-1, keepdims=True)
    return dict(dx=dx + r, tg=dy * xh, tb=dy, xh=xh,
                S_dx=rs * (np.abs(g) + A1 + np.abs(xh) * A2 + cx * np.abs(s2)) + np.abs(r) + np.abs(dx + r))


def y_S(x, gamma, beta, ref):
    x, gamma, beta = A64(x), A64(gamma), A64(beta)
    return np.abs(gamma) * ref["rstd"][:, None] * (np.abs(x) + np.abs(ref["mean"])[:, None]) + np.abs(beta) + np.abs(ref["y"])


def drop_scale(p):
    return f32(1.0) / (f32(1.0) - f32(p)) if p > 0 else f32(1.0)


def dmask_of(dx_stored, keep, p, dtype):
    """The masked copy: the STORED dx times keep / (1 - p) in fp32, rounded once to the launch's dtype."""
    v = np.asarray(dx_stored, dtype=f32) * drop_scale(p)
    if keep is not None:
        v = np.where(keep, v, f32(0))
    return store(v, dtype)


def quad(t, start):
    """sqrt(start^2 + sum_r t_r^2) + |start + sum_r t_r| per column: the quadrature sum of the summands and the size of the result."""
    return np.sqrt(A64(start) ** 2 + (A64(t) ** 2).sum(0)) + np.abs(A64(start) + A64(t).sum(0))


def wgrad_ln_fix_ref(G, gamma, beta, colsum):
    G, gamma, beta, cs = A64(G), A64(gamma)[:, None], A64(beta)[:, None], A64(colsum)[None, :]
    m = G.mean(0, keepdims=True)
    ref = gamma * (G - m) + beta * cs
    S = np.abs(gamma) * (np.abs(G) + 2.0 * np.abs(G).mean(0, keepdims=True)) + np.abs(beta * cs) + np.abs(ref)
    return ref, S


# ================================================================================================================ LayerNorm: emulations
def ln_fwd_emulation(x, gamma, beta, eps=EPS):
    """elementwise.hip: layernorm_fwd_kernel in float32 with sequential row sums -> mean, rstd, y in front of the store."""
    x, gamma, beta = (np.asarray(a, dtype=f32) for a in (x, gamma, beta))
    E = f32(x.shape[1])
    mu = seq_sum32(x) / E
    d = x - mu[:, None]
    var = seq_sum32(d * d) / E
    rs = f32(1.0) / np.sqrt(var + f32(eps))
    return dict(mean=mu, rstd=rs, y=d * rs[:, None] * gamma + beta)


def merge_emulation(part, eps=EPS):
    """The in-kernel merge (ln_stats_merge_kernel; common.h: ln_merge_parts) with its fp32 roundings."""
    part = np.asarray(part, dtype=f32)
    npart = part.shape[1]
    mu = seq_sum32(part[:, :, 0]) / f32(npart)
    m2 = np.zeros(part.shape[0], dtype=f32)
    for s in range(npart):
        d = part[:, s, 0] - mu
        m2 = m2 + (part[:, s, 1] + f32(256.0) * d * d)
    return dict(mean=mu, rstd=f32(1.0) / np.sqrt(m2 / (f32(256.0) * f32(npart)) + f32(eps)))


def ln_bwd_emulation(dy, x, gamma, mean, rstd, resid=None, prescaled=False):
    """layernorm_bwd_kernel in float32 with sequential row sums -> dx (in front of the store), the fp32 summands tg, tb."""
    dy, x, gamma = (np.asarray(a, dtype=f32) for a in (dy, x, gamma))
    mu, rs = np.asarray(mean, dtype=f32)[:, None], np.asarray(rstd, dtype=f32)[:, None]
    E = f32(x.shape[1])
    d = dy * (f32(1.0) / rs) if prescaled else dy
    xh = (x - mu) * rs
    g = d * gamma
    s1, s2 = (seq_sum32(g) / E)[:, None], (seq_sum32(g * xh) / E)[:, None]
    v = rs * (g - s1 - xh * s2)
    if resid is not None:
        v = v + np.asarray(resid, dtype=f32)
    return dict(dx=v, tg=d * xh, tb=d)


def ln_bwd_grid(rows):
    return max(1, min(-(-rows // 8), 1024))


N_ORDERS = 10          # arrival orders of the atomics the emulation is run under: ascending, descending, 8 fixed permutations


def param_partials(t, grid=None):
    """The addends of the final atomics for the fp32 summands t [rows, E], in the kernel's own tree: wave w of the launch (stride = 4 grid)
    chains the rows w, w + stride, ...; a workgroup folds its 4 waves in order; up to 256 workgroups each add their partial to the
    accumulator, more are folded by ln_param_reduce_kernel -- slice b of 32 chains the partials b, b + 32, ... -- and the 32 slices are
    added.  -> [grid or 32, E]."""
    t = np.asarray(t, dtype=f32)
    rows, E = t.shape
    grid = ln_bwd_grid(rows) if grid is None else grid
    stride = 4 * grid
    steps = -(-rows // stride)
    pad = np.zeros((steps * stride, E), dtype=f32)
    pad[:rows] = t
    pad = pad.reshape(steps, stride, E)
    wave = np.zeros((stride, E), dtype=f32)
    for s in range(steps):
        wave = wave + pad[s]
    wave = wave.reshape(grid, 4, E)
    wg = np.zeros((grid, E), dtype=f32)
    for w in range(4):
        wg = wg + wave[:, w]
    if grid <= 256:
        return wg
    sl = np.zeros((32, E), dtype=f32)
    for b in range(32):
        for p in range(b, grid, 32):
            sl[b] = sl[b] + wg[p]
    return sl


def atomics_fold(parts, start, order=0):
    """The atomics: the partials added onto the accumulator one after the other.  Their arrival order is not defined, so the emulation
    is run under N_ORDERS of them (0: ascending, 1: descending, k: the permutation of seed k) and q is the largest they give -- under a
    single order q of the 2049 x 64 case (against S2 alone) ranged from 5.1 u to 11.2 u over these ten."""
    n = parts.shape[0]
    seq = np.arange(n) if order == 0 else np.arange(n)[::-1] if order == 1 else np.random.default_rng(order).permutation(n)
    acc = np.array(start, dtype=f32).reshape(-1).copy()
    for p in seq:
        acc = acc + parts[p]
    return acc


def param_grad_emulation(t, start, grid=None, order=0):
    return atomics_fold(param_partials(t, grid), start, order)


def param_grad_q(t32, start, grid, ref, S2):
    parts = param_partials(t32, grid)
    return max(_q(atomics_fold(parts, start, k), ref, S2) for k in range(N_ORDERS))


def wgrad_ln_fix_emulation(G, gamma, beta, colsum):
    G, gamma, beta, cs = (np.asarray(a, dtype=f32) for a in (G, gamma, beta, colsum))
    m = seq_sum32(G.T) / f32(G.shape[0])
    return gamma[:, None] * (G - m[None, :]) + beta[:, None] * cs[None, :]


# ================================================================================================================ checking
def _q(emu, ref, S):
    nz = S > 0
    return float((np.abs(A64(emu) - ref)[nz] / S[nz]).max()) if nz.any() else 0.0


def limit_of(q, S, ref, dtype):
    return MARGIN * max(q, U) * S + (BF16_OUT * np.abs(ref) if dtype == BF16 else 0.0)


def f32_limits(emu, ref, size):
    """The fp32 idiom, relative to the element's natural size: (4 floor + 1e-6) size, floor = max |emu - ref| / size."""
    ref, size = A64(ref), A64(size)
    nz = size > 0
    floor = float((np.abs(A64(emu) - ref)[nz] / size[nz]).max()) if nz.any() else 0.0
    return (F32_MARGIN * floor + F32_ABS) * size, floor


def within(what, name, out, ref, lim, fails=None):
    """max error / limit of one array; raises (or keeps in `fails`) with output, element, value, reference, error and limit."""
    out, ref = A64(out), A64(ref)
    lim = np.broadcast_to(A64(lim), ref.shape)
    err = np.abs(out - ref)
    ok = err <= lim                     # (a NaN fails)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(ok & (lim == 0), 0.0, err / np.maximum(lim, 1e-300))
    worst = float(np.where(np.isnan(ratio), np.inf, ratio).max()) if err.size else 0.0
    if not bool(ok.all()):
        idx = tuple(int(i) for i in np.argwhere(~ok)[0])
        msg = ("%s: %s, element %s is %.9g, reference %.9g: error %.3g > limit %.3g (worst error/limit of the case %.3g, %d of %d elements)"
               % (what, name, idx, out[idx], ref[idx], err[idx], lim[idx], worst, int((~ok).sum()), ok.size))
        if fails is None:
            raise AssertionError(msg)
        fails.setdefault(name, msg)
    return worst


def exact(what, name, out, ref, fails=None):
    out, ref = np.asarray(out), np.asarray(ref)
    bad = ~(out == ref)
    if bool(bad.any()):
        idx = tuple(int(i) for i in np.argwhere(bad)[0])
        msg = "%s: %s, element %s is %r, must be exactly %r (%d of %d elements differ)" % (what, name, idx, out[idx].item(), ref[idx].item(),
                                                                                          int(bad.sum()), bad.size)
        if fails is None:
            raise AssertionError(msg)
        fails.setdefault(name, msg)
        return float("inf")
    return 0.0


def raise_first(res):
    if res["fails"]:
        raise AssertionError(next(iter(res["fails"].values())))


def figures(what, res):
    return "ROW_BOUNDS %s | err/limit %s | q/u %s" % (what, " ".join("%s %.2f" % kv for kv in res["worst"].items()),
                                                     " ".join("%s %.1f" % (k, v / U) for k, v in res["q"].items()))


def ln_check(dtype, x, gamma, beta=None, eps=EPS, y=None, mean=None, rstd=None, dy=None, stats=None, resid=None,
             prescaled=False, dx=None, dgamma=None, dbeta=None, start_g=None, start_b=None, grid=None, dmask=None,
             keep=None, p=0.0, colsum=None, start_cs=None, what="layernorm", raise_on_fail=True):
    """The arrays of one launch against the bounds.  Operands as stored (numpy or torch; bf16 values widened).

    forward   y, mean, rstd given: against ln_fwd_ref of x.
    backward  dx (+ dgamma, dbeta and their start values; + dmask with keep / p, + colsum with its start) given: the statistics the
              kernel read are `stats` = (mean, rstd) arrays;
              prescaled: dy holds rstd o gradient.  The masked copy and the column sums come from the dx that was STORED.
    -> dict(worst = {output: error / limit}, q = {output: q}, fails = {output: message}); raises the first failure unless told not to."""
    worst, q, fails = {}, {}, {}
    x64 = A64(x)
    if y is not None:
        ref, emu = ln_fwd_ref(x64, gamma, beta, eps), ln_fwd_emulation(x64, gamma, beta, eps)
        S = y_S(x64, gamma, beta, ref)
        q["y"] = _q(emu["y"], ref["y"], S)
        worst["y"] = within(what, "y", y, ref["y"], limit_of(q["y"], S, ref["y"], dtype), fails)
        for n, size in (("mean", np.abs(x64).mean(-1)), ("rstd", ref["rstd"])):
            lim, q[n] = f32_limits(emu[n], ref[n], size)
            worst[n] = within(what, n, {"mean": mean, "rstd": rstd}[n], ref[n], lim, fails)
    if dx is not None:
        mu, rs = A64(stats[0]), A64(stats[1])
        ref = ln_bwd_ref(dy, x64, gamma, mu, rs, resid, prescaled)
        emu = ln_bwd_emulation(A64(dy), x64, gamma, mu, rs, None if resid is None else A64(resid), prescaled)
        q["dx"] = _q(emu["dx"], ref["dx"], ref["S_dx"])
        worst["dx"] = within(what, "dx", dx, ref["dx"], limit_of(q["dx"], ref["S_dx"], ref["dx"], dtype), fails)
        for n, got, t64, t32, st in (("dgamma", dgamma, ref["tg"], emu["tg"], start_g), ("dbeta", dbeta, ref["tb"], emu["tb"], start_b)):
            if got is None:
                continue
            r, S2 = A64(st) + t64.sum(0), quad(t64, st)
            q[n] = param_grad_q(t32, st, grid, r, S2)
            worst[n] = within(what, n, got, r, limit_of(q[n], S2, r, FP32), fails)
        if dmask is not None or colsum is not None:
            want = dmask_of(A64(dx), keep, p, dtype)
            if dmask is not None:
                worst["dmask"] = exact(what, "dmask", A64(dmask), want.astype(np.float64), fails)
            if colsum is not None:
                r, S2 = A64(start_cs) + want.astype(np.float64).sum(0), quad(want, start_cs)
                q["colsum"] = param_grad_q(want, start_cs, grid, r, S2)
                worst["colsum"] = within(what, "colsum", colsum, r, limit_of(q["colsum"], S2, r, FP32), fails)
    res = dict(worst=worst, q=q, fails=fails)
    if raise_on_fail:
        raise_first(res)
    return res


def merge_check(part, mean, rstd, eps=EPS, what="ln_stats_merge", raise_on_fail=True):
    """cmp_k_ln_stats_merge: mean and rstd of every row from its partials, the fp32 idiom against the float64 merge."""
    ref, emu = merge_ref(part, eps), merge_emulation(part, eps)
    worst, q, fails = {}, {}, {}
    for n, got, size in (("mean", mean, np.abs(A64(part)[:, :, 0]).mean(-1)), ("rstd", rstd, ref["rstd"])):
        lim, q[n] = f32_limits(emu[n], ref[n], size)
        worst[n] = within(what, n, got, ref[n], lim, fails)
    res = dict(worst=worst, q=q, fails=fails)
    if raise_on_fail:
        raise_first(res)
    return res


def fix_check(G0, gamma, beta, colsum, G, what="wgrad_ln_fix", raise_on_fail=True):
    ref, S = wgrad_ln_fix_ref(G0, gamma, beta, colsum)
    q = _q(wgrad_ln_fix_emulation(G0, gamma, beta, colsum), ref, S)
    fails = {}
    res = dict(worst={"G": within(what, "G", G, ref, limit_of(q, S, ref, FP32), fails)}, q={"G": q}, fails=fails)
    if raise_on_fail:
        raise_first(res)
    return res


# ================================================================================================================ LayerNorm: inputs
def ln_inputs(rows, E, dtype, seed, segments=False):
    """Planted rows -> dict of float32 arrays as stored: x, dy, resid [rows, E] (rounded to the launch's dtype), gamma, beta [E], and
    `kinds` [rows].  Row r is of kind LN_KINDS[r % 8]: unit-variance draws around 0.5, 24 and 300 (|mean| >> sigma: the cancellation in
    x - mu), a constant row (3.25: var = 0, rstd = eps^-1/2), a zero row, a row with one outlier of 200 sigma.  segments (E a multiple
    of 256): every random row gets per-segment offsets +1.5, -1.5, +1.5 ... sigma on top, so that the between-segment term 256 d^2 of the
    statistics merge is more than SEG_SHARE_MIN of the row's M2 (about 2/3; `merge_ref` returns the share)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (rows, E))
    kinds = np.array([LN_KINDS[r % len(LN_KINDS)] for r in range(rows)])
    if segments:
        assert E % 256 == 0
        x += np.repeat(1.5 * (-1.0) ** np.arange(E // 256), 256)[None, :]
    for kind, off in (("off0.5", 0.5), ("off24", 24.0), ("off300", 300.0)):
        x[kinds == kind] += off
    x[kinds == "const"] = 3.25
    x[kinds == "zero"] = 0.0
    out_rows = np.flatnonzero(kinds == "outlier")
    x[out_rows, (7 * out_rows + 3) % E] = 200.0
    gamma = (1 + 0.3 * rng.normal(size=E)).astype(f32)
    beta = rng.normal(0, 0.2, E).astype(f32)
    return dict(x=store(x, dtype), dy=store(rng.normal(0, 1.0, (rows, E)), dtype), resid=store(rng.normal(0, 1.0, (rows, E)), dtype),
                gamma=gamma, beta=beta, kinds=kinds)


def fix_inputs(rows, cols, seed):
    """wgrad_ln_fix: column means of the order of 100 times the column spread."""
    rng = np.random.default_rng(seed)
    G = (rng.normal(0, 1.0, (rows, cols)) + 100.0 * rng.normal(0, 1.0, (1, cols)) + 50.0).astype(f32)
    return dict(G=G, gamma=(1 + 0.3 * rng.normal(size=rows)).astype(f32), beta=rng.normal(0, 0.2, rows).astype(f32),
                colsum=rng.normal(0, 30.0, cols).astype(f32))


# ================================================================================================================ cross-entropy
def xent_ref(z, y, inv_n):
    """float64: lse, row loss, argmax (ties to the lowest column), probabilities, dlogits over the V valid columns, and S of dlogits."""
    z, y = A64(z), np.asarray(y).astype(np.int64).reshape(-1)
    rows = z.shape[0]
    m = z.max(-1)
    e = np.exp(z - m[:, None])
    lse = m + np.log(e.sum(-1))
    p = np.exp(z - lse[:, None])
    hot = np.zeros_like(z)
    hot[np.arange(rows), y] = 1.0
    zy = z[np.arange(rows), y]
    inv = float(f32(inv_n))
    return dict(lse=lse, loss=lse - zy, arg=z.argmax(-1), correct=(z.argmax(-1) == y).astype(np.int64), p=p, dz=(p - hot) * inv,
                S=inv * (p * (1.0 + np.abs(z) + np.abs(lse)[:, None]) + hot), size=np.abs(lse) + np.abs(zy))


def xent_emulation(z, y, inv_n):
    """softmax_xent*_kernel in float32 with a sequential row sum -> loss and both forms of the gradient in front of the store: exp(z - lse)
    (generic and wide kernels) and exp(z - max) / sum (the 8-column kernel)."""
    z, y = np.asarray(z, dtype=f32), np.asarray(y).astype(np.int64).reshape(-1)
    rows = z.shape[0]
    m = z.max(-1)
    e = np.exp(z - m[:, None])
    s = seq_sum32(e)
    lse = m + np.log(s)
    hot = np.zeros_like(z)
    hot[np.arange(rows), y] = 1.0
    k = f32(inv_n)
    return dict(loss=lse - z[np.arange(rows), y], dz_a=(np.exp(z - lse[:, None]) - hot) * k, dz_b=(e * (f32(1.0) / s)[:, None] - hot) * k)


def xent_check(dtype, z, y, inv_n, dz, loss, correct, V, what="softmax_xent", raise_on_fail=True):
    """One launch: z [rows, V] the valid logits, dz [rows, ldz] as stored (padding included), loss [rows], correct [rows]."""
    ref, emu = xent_ref(z, y, inv_n), xent_emulation(z, y, inv_n)
    worst, q, fails = {}, {}, {}
    dz = A64(dz)
    q["dlogits"] = max(_q(emu["dz_a"], ref["dz"], ref["S"]), _q(emu["dz_b"], ref["dz"], ref["S"]))
    worst["dlogits"] = within(what, "dlogits", dz[:, :V], ref["dz"], limit_of(q["dlogits"], ref["S"], ref["dz"], dtype), fails)
    if dz.shape[1] > V:
        worst["padding"] = exact(what, "padding", dz[:, V:], np.zeros_like(dz[:, V:]), fails)
    lim, q["row_loss"] = f32_limits(emu["loss"], ref["loss"], ref["size"])
    worst["row_loss"] = within(what, "row_loss", loss, ref["loss"], lim, fails)
    worst["row_correct"] = exact(what, "row_correct", np.asarray(A64(correct)).astype(np.int64).reshape(-1), ref["correct"], fails)
    res = dict(worst=worst, q=q, fails=fails)
    if raise_on_fail:
        raise_first(res)
    return res


XENT_BLOCK = 64         # the planted pattern repeats every 64 rows where it names rows (ties, shifts, labels 0 and V - 1)


def xent_inputs(rows, V, seed):
    """Planted logits -> z float32 [rows, V], y int32 [rows], info (dict of row index arrays).

    Background XENT_SPREAD N(0, 1).  Row r raises column r mod V until its probability is XENT_TARGET, its label elsewhere: with rows >= V
    every column carries weight in some row, so a column left out of a sum shows.  In every block of 64 rows (the rows a launch of
    many rows gives to different waves, and -- past 32768 rows -- to a wave's later trips):
        rows 8, 9    columns 7 and 8 tie exactly at the top with probability 0.3 each (0.4 where the row has no other raised column) (a lane boundary of the 8-column kernel); label 7 in row 8 (correct), 8 in
                     row 9 (the higher index: correct = 0)
        rows 10, 11  the same on columns 63 and 64 (a slot boundary of the generic kernel, a lane boundary of the wide one)
        rows 16-23   all logits + 80;  rows 24-31: all logits - 80
        row 0        label V - 1;  row 1: label 0
    everywhere else a random label, so that a label taken from another row shows."""
    rng = np.random.default_rng(seed)
    z = XENT_SPREAD * rng.normal(size=(rows, V))
    y = rng.integers(0, V, rows)
    r = np.arange(rows)
    c = r % V
    b = r % XENT_BLOCK
    info = {}
    if V > 1:
        y = np.where(y == c, (y + 1) % V, y)
        y[b == 0], y[b == 1] = V - 1, 0
        y[(b == 0) & (c == V - 1)] = 0
        y[(b == 1) & (c == 0)] = V - 1

        def raise_to(rows_, cols_, targets):
            """column cols_[n, j] of row rows_[n] gets probability targets[j]: the logit lse(other columns) + log(targets[j] / (1 - sum targets))"""
            zz = z[rows_].copy()
            np.put_along_axis(zz, cols_, -np.inf, 1)
            m = zz.max(-1)
            lse_o = m + np.log(np.exp(zz - m[:, None]).sum(-1))
            for j, t in enumerate(targets):
                z[rows_, cols_[:, j]] = lse_o + np.log(t / (1.0 - sum(targets)))
        raise_to(r, c[:, None], (XENT_TARGET,))
        for name, lo, rr in (("tie7", 7, 8), ("tie63", 63, 10)):
            if V > lo + 1:
                t0, t1 = np.flatnonzero(b == rr), np.flatnonzero(b == rr + 1)
                both = np.concatenate([t0, t1])
                own = ~np.isin(c[both], (lo, lo + 1))           # the row's own column stays raised (0.28) unless it is one of the pair
                pair = np.tile(np.array([[lo, lo + 1]]), (both.size, 1))
                raise_to(both[~own], pair[~own], (0.4, 0.4))
                raise_to(both[own], np.concatenate([pair[own], c[both][own, None]], 1), (0.3, 0.3, 0.28))
                y[t0], y[t1] = lo, lo + 1
                info[name] = (t0, t1)
        up, down = np.flatnonzero((b >= 16) & (b < 24)), np.flatnonzero((b >= 24) & (b < 32))
        z[up] += SHIFT
        z[down] -= SHIFT
        info.update(up=up, down=down)
    else:
        y[:] = 0
    return z.astype(f32), y.astype(np.int32), info
