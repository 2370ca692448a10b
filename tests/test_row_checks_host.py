"""The assertions of tests/row_bounds.py can fail (CPU; the pattern of tests/test_attention_checks_host.py).

`fake_ln_fwd`, `fake_ln_bwd`, `fake_merge` and `fake_xent` are chunk- and wave-structured numpy statements of the row kernels of elementwise.hip: a
lane owns the 16-byte chunks lane + 64 i of a row (eight consecutive columns in the cross-entropy kernel) and the lanes are folded by
the xor butterfly; a wave strides over the rows w, w + stride, ... with the next row prefetched; the parameter-gradient partials go
through the 4-wave fold and then the atomics or the 32-slice reduce with its 8-way unrolled loop and tail.  Each is correct, and wrong
in the ways such kernels go wrong (BUGS).  Every wrong one must be rejected by the check on the output named for it, with that check's
message.  To see that a class of error is caught, edit a copy of a fake below -- not the library.

Further: the correct fakes sit inside every limit; on every geometry of tests/test_gpu_row_bounds.py the float64 reference as stored
sits inside every limit, the planted inputs meet their conditions, any single row removed from dgamma / dbeta / colsum moves some
column by ten limits, any single element that carries weight removed from a row's mean moves some element of the row by ten limits
(fp32; two limits in bf16); the cases reach the kernel forms their tables name; and the record of what the whole-tensor metric let
through."""
import math
import re

import numpy as np
import pytest

import row_bounds as RB
import test_gpu_row_bounds as GB
from oracle import transformer_oracle as O

FP32, BF16 = 0, 1
f32 = np.float32
EPS = RB.EPS
# bug -> (the kernel it lives in, the output whose check must reject it, the dtypes it can show in)
BUGS = {
    "mean_last_chunk": ("fwd", "mean", (FP32, BF16)), "var_e_minus_1": ("fwd", "rstd", (FP32, BF16)), "eps_outside": ("fwd", "rstd", (FP32, BF16)),
    "second_row_stale": ("fwd", "y", (FP32, BF16)), "stats_neighbour": ("fwd", "mean", (FP32, BF16)),
    "s2_last_chunk": ("bwd", "dx", (FP32, BF16)), "ragged_row_dropped": ("bwd", "dgamma", (FP32, BF16)),
    "fold_three_waves": ("bwd", "dbeta", (FP32, BF16)), "reduce_tail_dropped": ("bwd", "dgamma", (FP32, BF16)),
    "resid_before_rstd": ("bwd", "dx", (FP32, BF16)), "mask_unrounded": ("bwd", "dmask", (BF16,)),       # (an fp32 store rounds nothing)
    "colsum_unmasked": ("bwd", "colsum", (FP32, BF16)), "no_prescale": ("prescaled", "dx", (BF16,)), "merge_no_between": ("merge", "rstd", (BF16,)),
    "last_col": ("xent", "dlogits", (FP32, BF16)), "lane_col7": ("xent", "dlogits", (FP32, BF16)), "pad_included": ("xent", "dlogits", (FP32, BF16)),
    "tie_high": ("xent", "row_correct", (FP32, BF16)), "next_label": ("xent", "row_loss", (FP32, BF16)), "no_max": ("xent", "row_loss", (FP32, BF16)),
    "label_no_inv_n": ("xent", "dlogits", (FP32, BF16)),
}
SEED, STREAM = GB.SEED, GB.STREAM


# ---------------------------------------------------------------------------------------------------------------- the fakes
def lane_sum(a, VN, drop_last_chunk=False):
    """Row sums of a [rows, E] float32 as a wave forms them: lane l adds its chunks l, l + 64, ... element by element, then the
    butterfly over xor 32, 16, ..., 1."""
    rows, E = a.shape
    chunks = E // VN
    maxi = -(-chunks // 64)
    pad = np.zeros((rows, maxi * 64 * VN), dtype=f32)
    pad[:, :E] = a
    if drop_last_chunk:
        pad[:, (chunks - 1) * VN:chunks * VN] = 0
    pad = pad.reshape(rows, maxi, 64, VN)
    lane = np.zeros((rows, 64), dtype=f32)
    for i in range(maxi):
        for j in range(VN):
            lane = lane + pad[:, i, :, j]
    for o in (32, 16, 8, 4, 2, 1):
        lane = lane + lane[:, np.arange(64) ^ o]
    return lane[:, 0]


def fake_ln_fwd(x, gamma, beta, dtype, grid, bug=None):
    """layernorm_fwd_kernel -> y as stored, mean, rstd."""
    x, gamma, beta = (np.asarray(a, dtype=f32) for a in (x, gamma, beta))
    rows, E = x.shape
    VN, stride = (8 if dtype == BF16 else 4), 4 * grid
    if bug == "second_row_stale":                        # v[i] = nx[i] forgotten: a wave's later rows are computed from its first row
        x = x[np.arange(rows) % stride]
    mu = lane_sum(x, VN, bug == "mean_last_chunk") / f32(E)
    d = x - mu[:, None]
    var = lane_sum(d * d, VN) / f32(E - 1 if bug == "var_e_minus_1" else E)
    rs = f32(1.0) / (np.sqrt(var) + f32(EPS)) if bug == "eps_outside" else f32(1.0) / np.sqrt(var + f32(EPS))
    y = RB.store(d * rs[:, None] * gamma + beta, dtype)
    if bug == "stats_neighbour":
        mu, rs = np.concatenate([mu[:1], mu[:-1]]), np.concatenate([rs[:1], rs[:-1]])
    return y, mu, rs


def fake_param_grads(t, start, rows, grid, bug, ragged_bug):
    """The partial sums of layernorm_bwd_kernel and their way into the accumulator (direct atomics up to 256 workgroups, else
    ln_param_reduce_kernel: 32 slices, 8 partials per unrolled pass, then the tail)."""
    t = np.asarray(t, dtype=f32)
    E = t.shape[1]
    stride = 4 * grid
    steps = -(-rows // stride)
    pad = np.zeros((steps * stride, E), dtype=f32)
    pad[:rows] = t
    if ragged_bug and rows % stride:                     # the last trip, which only some waves take, is left out
        pad[(steps - 1) * stride:] = 0
    pad = pad.reshape(steps, stride, E)
    wave = np.zeros((stride, E), dtype=f32)
    for s in range(steps):
        wave = wave + pad[s]
    wave = wave.reshape(grid, 4, E)
    wg = np.zeros((grid, E), dtype=f32)
    for w in range(3 if bug == "fold_three_waves" else 4):
        wg = wg + wave[:, w]
    acc = np.array(start, dtype=f32).copy()
    if grid <= 256:
        for p in range(grid):
            acc = acc + wg[p]
        return acc
    for b in range(32):
        a, p = f32(0) * np.zeros(E, dtype=f32), b
        while p + 7 * 32 < grid:
            for u in range(8):
                a = a + wg[p + u * 32]
            p += 8 * 32
        while p < grid and bug != "reduce_tail_dropped":
            a = a + wg[p]
            p += 32
        acc = acc + a
    return acc


def fake_merge(part, bug=None):
    """ln_stats_merge_kernel (common.h: ln_merge_parts) -> mean, rstd of every row from its partials."""
    pt = np.asarray(part, dtype=f32)
    npart = pt.shape[1]
    mu = RB.seq_sum32(pt[:, :, 0]) / f32(npart)
    m2 = np.zeros(pt.shape[0], dtype=f32)
    for s in range(npart):
        dd = pt[:, s, 0] - mu
        m2 = m2 + (pt[:, s, 1] if bug == "merge_no_between" else pt[:, s, 1] + f32(256.0) * dd * dd)
    return mu, f32(1.0) / np.sqrt(m2 / (f32(256.0) * f32(npart)) + f32(EPS))


def fake_ln_bwd(dy, x, gamma, dtype, grid, start, stats, resid=None, prescaled=False, keep=None, p=0.0, bug=None):
    """layernorm_bwd_kernel (plain / fused prologue / prescaled) -> dict of the arrays as stored."""
    dy, x, gamma = (np.asarray(a, dtype=f32) for a in (dy, x, gamma))
    rows, E = x.shape
    VN = 8 if dtype == BF16 else 4
    mu, rs = np.asarray(stats[0], dtype=f32)[:, None], np.asarray(stats[1], dtype=f32)[:, None]
    d = dy * (f32(1.0) / rs) if (prescaled and bug != "no_prescale") else dy
    xh = (x - mu) * rs
    g = d * gamma
    s1 = (lane_sum(g, VN) / f32(E))[:, None]
    s2 = (lane_sum(g * xh, VN, bug == "s2_last_chunk") / f32(E))[:, None]
    r = np.zeros_like(x) if resid is None else np.asarray(resid, dtype=f32)
    v = rs * (g - s1 - xh * s2 + r) if bug == "resid_before_rstd" else rs * (g - s1 - xh * s2) + r
    dx = RB.store(v, dtype)
    dmask = RB.dmask_of(v if bug == "mask_unrounded" else dx, keep, p, dtype)
    out = dict(dx=dx, dmask=dmask)
    for n, t in (("dgamma", d * xh), ("dbeta", d), ("colsum", dx if bug == "colsum_unmasked" else dmask)):
        out[n] = fake_param_grads(t, start[n], rows, grid, bug, bug == "ragged_row_dropped" and n == "dgamma")
    return out


def fake_xent(z, y, V, ldz, inv_n, dtype, grid, bug=None, pad_value=0.0):
    """softmax_xent8_kernel: lane l owns the columns 8 l .. 8 l + 7 -> dz [rows, ldz] as stored, loss, correct."""
    rows = z.shape[0]
    zf = np.full((rows, 512), f32(pad_value), dtype=f32)
    zf[:, :V] = z
    col = np.arange(512)
    valid = col < (ldz if bug == "pad_included" else V)
    stride = 4 * grid
    yy = np.asarray(y).astype(np.int64)
    if bug == "next_label":                              # yy read after the prefetch overwrote it
        nxt = np.arange(rows) + stride
        yy = np.where(nxt < rows, yy[np.minimum(nxt, rows - 1)], yy)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        v = np.where(valid[None, :], zf, -np.inf).astype(f32)
        gmx = v.max(-1)
        top = v == gmx[:, None]
        arg = (511 - np.argmax(top[:, ::-1], -1)) if bug == "tie_high" else np.argmax(top, -1)
        e = np.exp(v) if bug == "no_max" else np.exp(v - gmx[:, None])
        es = e.copy()
        if bug == "last_col":
            es[:, V - 1] = 0
        if bug == "lane_col7":
            es[:, 7::8] = 0
        lane = np.zeros((rows, 64), dtype=f32)
        es = es.reshape(rows, 64, 8)
        for j in range(8):
            lane = lane + es[:, :, j]
        for o in (32, 16, 8, 4, 2, 1):
            lane = lane + lane[:, np.arange(64) ^ o]
        ssum = lane[:, 0]
        lse = np.log(ssum) if bug == "no_max" else gmx + np.log(ssum)
        hot = (col[None, :] == yy[:, None]).astype(f32)
        k = f32(inv_n)
        g = e * (f32(1.0) / ssum)[:, None] * k - hot if bug == "label_no_inv_n" else (e * (f32(1.0) / ssum)[:, None] - hot) * k
        g = np.where((col < V)[None, :], g, f32(0))
        loss = lse - zf[np.arange(rows), yy]
    return RB.store(g[:, :ldz], dtype), loss, (arg == yy).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- running a fake through its check
def keep_of(rows, E, p):
    return O.dropout_keep_rows(SEED, STREAM, rows, E, p) if p > 0 else None


def starts(E, seed=5):
    rng = np.random.default_rng(seed)
    return {n: rng.normal(0, 3.0, E).astype(f32) for n in ("dgamma", "dbeta", "colsum")}


def stats32(inp):
    ref = RB.ln_fwd_ref(inp["x"], inp["gamma"], inp["beta"], EPS)
    return ref["mean"].astype(f32), ref["rstd"].astype(f32)


def check_fwd(dtype, rows, E, grid, bug=None):
    inp = RB.ln_inputs(rows, E, dtype, seed=rows + E)
    y, mu, rs = fake_ln_fwd(inp["x"], inp["gamma"], inp["beta"], dtype, grid, bug)
    return RB.ln_check(dtype, inp["x"], inp["gamma"], inp["beta"], EPS, y=y, mean=mu, rstd=rs, raise_on_fail=False)


def check_bwd(dtype, rows, E, grid, form="bwd", bug=None, p=0.25):
    inp = RB.ln_inputs(rows, E, dtype, seed=rows + E + 1, segments=form != "bwd")
    st, keep = starts(E), keep_of(rows, E, p)
    dy, s, pre = inp["dy"], stats32(inp), form == "prescaled"
    if pre:
        dy = RB.store(inp["dy"].astype(np.float64) * s[1][:, None].astype(np.float64), dtype)
    out = fake_ln_bwd(dy, inp["x"], inp["gamma"], dtype, grid, st, s, resid=inp["resid"], prescaled=pre, keep=keep, p=p, bug=bug)
    return RB.ln_check(dtype, inp["x"], inp["gamma"], dy=dy, stats=s, prescaled=pre, resid=inp["resid"], dx=out["dx"], dgamma=out["dgamma"],
                       dbeta=out["dbeta"], start_g=st["dgamma"], start_b=st["dbeta"], grid=grid, dmask=out["dmask"], keep=keep, p=p,
                       colsum=out["colsum"], start_cs=st["colsum"], raise_on_fail=False)


def check_merge(rows, E, grid=None, bug=None):
    """The merge of the partial statistics on the planted per-segment offsets (the geometry's grid plays no part in it)."""
    part = RB.parts_of(RB.ln_inputs(rows, E, BF16, seed=rows + E + 1, segments=True)["x"]).astype(f32)
    mu, rs = fake_merge(part, bug)
    return RB.merge_check(part, mu, rs, raise_on_fail=False)


def check_xent(dtype, rows, V, ldz, grid, bug=None):
    z, y, _ = RB.xent_inputs(rows, V, seed=rows + V + ldz)
    dz, loss, corr = fake_xent(z, y, V, ldz, 1.0 / rows, dtype, grid, bug)
    return RB.xent_check(dtype, z, y, 1.0 / rows, dz, loss, corr, V, raise_on_fail=False)


# (geometry, grid): small grids give a wave several rows; 2049 rows reach the reduce with its tail (grid 257)
FWD_GEO = [(37, 768, 3), (13, 1032, 1), (3, 8, 1)]
BWD_GEO = [(2049, 64, 257), (37, 768, 2), (13, 64, 1)]
PARTS_GEO = [(66, 512, 3)]
XENT_GEO = [(520, 390, 448, 20), (70, 50, 56, 2)]


def run_bug(kernel, dtype, bug):
    if kernel == "fwd":
        return [check_fwd(dtype, *g, bug=bug) for g in FWD_GEO[:1]]
    if kernel == "bwd":
        return [check_bwd(dtype, *g, bug=bug) for g in BWD_GEO[:2]]
    if kernel == "prescaled":
        return [check_bwd(dtype, *g, form=kernel, bug=bug) for g in PARTS_GEO]
    if kernel == "merge":
        return [check_merge(*g, bug=bug) for g in PARTS_GEO]
    return [check_xent(dtype, *g, bug=bug) for g in XENT_GEO]


@pytest.mark.parametrize("dtype", [FP32, BF16])
def test_the_correct_fakes_sit_inside_every_limit(dtype):
    res = [check_fwd(dtype, *g) for g in FWD_GEO] + [check_bwd(dtype, *g) for g in BWD_GEO] + [check_xent(dtype, *g) for g in XENT_GEO]
    if dtype == BF16:
        res += [check_bwd(dtype, *g, form="prescaled") for g in PARTS_GEO] + [check_merge(*g) for g in PARTS_GEO]
    for r in res:
        assert not r["fails"], r["fails"]
        assert max(r["worst"].values()) <= 1.0


@pytest.mark.parametrize("bug", sorted(BUGS))
def test_a_wrong_kernel_is_rejected_by_the_check_named_for_it(bug):
    kernel, output, dtypes = BUGS[bug]
    for dtype in dtypes:
        res = run_bug(kernel, dtype, bug)
        msgs = [r["fails"][output] for r in res if output in r["fails"]]
        assert msgs, "%s (dtype %d) passed the check of %s: %s" % (bug, dtype, output, [r["worst"] for r in res])
        assert re.search(r": %s, element \(\d+,( \d+)?\) is .*(> limit|must be exactly)" % output, msgs[0]), msgs[0]


def test_every_bug_has_a_test_and_every_issue_bug_is_listed():
    want = {"mean_last_chunk", "s2_last_chunk", "var_e_minus_1", "eps_outside", "second_row_stale", "stats_neighbour", "ragged_row_dropped",
            "fold_three_waves", "reduce_tail_dropped", "resid_before_rstd", "mask_unrounded", "colsum_unmasked", "no_prescale",
            "merge_no_between", "last_col", "lane_col7", "pad_included", "tie_high", "next_label", "no_max", "label_no_inv_n"}
    assert want <= set(BUGS)
    import inspect
    src = "".join(inspect.getsource(f) for f in (fake_ln_fwd, fake_merge, fake_ln_bwd, fake_param_grads, fake_xent))
    for bug in BUGS:
        assert '"%s"' % bug in src, "%s is in BUGS but no fake implements it" % bug


# ---------------------------------------------------------------------------------------------------------------- the GPU geometries
def ln_fwd_geometries():
    return [(d, c[0], c[1]) for c in GB.LN_FWD for d in (FP32, BF16)]


def ln_bwd_geometries():
    return [(d, c[0], c[1]) for c in GB.LN_BWD for d in c[2]]


def stored_reference_bwd(dtype, rows, E, form, p):
    """The float64 reference, rounded where an output is stored, in the place of a kernel -> the arguments of ln_check."""
    inp = RB.ln_inputs(rows, E, dtype, seed=rows + E + (1 if form == "bwd" else 2), segments=form != "bwd")
    keep, st = keep_of(rows, E, p), starts(E)
    dy, s = inp["dy"], stats32(inp)
    kw = dict(stats=s)
    if form == "prescaled":
        dy = RB.store(inp["dy"].astype(np.float64) * s[1][:, None].astype(np.float64), dtype)
        kw["prescaled"] = True
    ref = RB.ln_bwd_ref(dy, inp["x"], inp["gamma"], s[0], s[1], inp["resid"], form == "prescaled")
    dx = RB.store(ref["dx"], dtype)
    dmask = RB.dmask_of(dx, keep, p, dtype)
    args = dict(dy=dy, resid=inp["resid"], dx=dx, dgamma=st["dgamma"] + ref["tg"].sum(0), dbeta=st["dbeta"] + ref["tb"].sum(0),
                start_g=st["dgamma"], start_b=st["dbeta"], dmask=dmask, keep=keep, p=p, colsum=st["colsum"] + dmask.astype(np.float64).sum(0),
                start_cs=st["colsum"], **kw)
    return inp, ref, args


@pytest.mark.parametrize("dtype,rows,E", ln_fwd_geometries())
def test_forward_geometry_reference_planted_rows_and_a_removed_element(dtype, rows, E):
    inp = RB.ln_inputs(rows, E, dtype, seed=rows + E)
    x = inp["x"].astype(np.float64)
    ref = RB.ln_fwd_ref(x, inp["gamma"], inp["beta"])
    res = RB.ln_check(dtype, x, inp["gamma"], inp["beta"], y=RB.store(ref["y"], dtype), mean=ref["mean"].astype(f32), rstd=ref["rstd"].astype(f32))
    assert max(res["worst"].values()) <= 1.0
    # the planted conditions
    kinds, sd = inp["kinds"], x.std(-1)
    for kind, ratio in (("off24", 15.0), ("off300", 100.0)):
        assert (np.abs(ref["mean"][kinds == kind]) >= ratio * sd[kinds == kind]).all()
    assert (sd[kinds == "const"] == 0).all() and (x[kinds == "const"] != 0).all() and (x[kinds == "zero"] == 0).all()
    if E >= 64:
        assert (np.abs(x[kinds == "outlier"]).max(-1) >= 5 * sd[kinds == "outlier"]).all()
    if rows >= 6:
        assert set(RB.LN_KINDS) <= set(kinds)
    # an element that carries weight (|x| at least a quarter of the row's rms) left out of the row's mean moves the mean by |x| / E and,
    # to first order, every y of the row by gamma rstd |x| / E: that is ten limits of some element (fp32), two in bf16.  A zero row has
    # no such element.
    emu = RB.ln_fwd_emulation(x, inp["gamma"], inp["beta"])
    S = RB.y_S(x, inp["gamma"], inp["beta"], ref)
    lim_y = RB.limit_of(res["q"]["y"], S, ref["y"], dtype)
    lim_m, _ = RB.f32_limits(emu["mean"], ref["mean"], np.abs(x).mean(-1))
    live = kinds != "zero"
    shift = 0.25 * np.sqrt((x ** 2).mean(-1)) / E
    with np.errstate(divide="ignore", invalid="ignore"):
        moved = np.maximum((np.abs(inp["gamma"]) * ref["rstd"][:, None] * shift[:, None] / lim_y).max(-1), shift / lim_m)
    assert (moved[live] >= (10.0 if dtype == FP32 else 2.0)).all(), moved[live].min()


@pytest.mark.parametrize("dtype,rows,E", ln_bwd_geometries())
@pytest.mark.parametrize("p", [0.0, GB.P_FUSED])
def test_backward_geometry_reference_and_a_removed_row(dtype, rows, E, p):
    inp, ref, args = stored_reference_bwd(dtype, rows, E, "bwd", p)
    res = RB.ln_check(dtype, inp["x"], inp["gamma"], **args)
    assert max(res["worst"].values()) <= 1.0
    # any single row left out of a parameter gradient moves some column by ten limits (a row whose xhat is zero -- the constant and the
    # zero row -- has no summand in dgamma)
    dm = args["dmask"].astype(np.float64)
    for n, t, st in (("dgamma", ref["tg"], args["start_g"]), ("dbeta", ref["tb"], args["start_b"]), ("colsum", dm, args["start_cs"])):
        lim = RB.limit_of(res["q"][n], RB.quad(t, st), 0.0, FP32)
        live = np.abs(t).max(-1) > 0
        if n == "dgamma":
            assert (live == ~np.isin(inp["kinds"], ("const", "zero"))).all()
        else:
            assert live.all()
        assert ((np.abs(t) / lim).max(-1)[live] >= 10.0).all(), n


@pytest.mark.parametrize("rows,E", GB.PARTS)
@pytest.mark.parametrize("form", ["prescaled"])
def test_partials_geometry_reference_and_the_between_segment_share(rows, E, form):
    inp, ref, args = stored_reference_bwd(BF16, rows, E, form, GB.P_FUSED)
    res = RB.ln_check(BF16, inp["x"], inp["gamma"], **args)
    assert max(res["worst"].values()) <= 1.0
    m = RB.merge_ref(RB.parts_of(inp["x"]).astype(f32))
    res = RB.merge_check(RB.parts_of(inp["x"]).astype(f32), m["mean"].astype(f32), m["rstd"].astype(f32))
    assert max(res["worst"].values()) <= 1.0
    if E > 256:                                          # (one segment has no between-segment term)
        rnd = np.isin(inp["kinds"], ("off0.5", "off24", "off300"))
        assert (m["share"][rnd] >= RB.SEG_SHARE_MIN).all(), m["share"][rnd].min()


@pytest.mark.parametrize("rows,cols", GB.FIX)
def test_fix_geometry_reference_and_column_means(rows, cols):
    inp = RB.fix_inputs(rows, cols, seed=rows + cols)
    ref, _ = RB.wgrad_ln_fix_ref(inp["G"], inp["gamma"], inp["beta"], inp["colsum"])
    assert RB.fix_check(inp["G"], inp["gamma"], inp["beta"], inp["colsum"], ref.astype(f32))["worst"]["G"] <= 1.0
    G = inp["G"].astype(np.float64)
    assert np.median(np.abs(G.mean(0)) / G.std(0)) >= 30.0
    # the mean term forgotten
    wrong = inp["gamma"][:, None].astype(np.float64) * G + inp["beta"][:, None] * inp["colsum"][None, :].astype(np.float64)
    assert "G" in RB.fix_check(inp["G"], inp["gamma"], inp["beta"], inp["colsum"], wrong, raise_on_fail=False)["fails"]


@pytest.mark.parametrize("dtype", [FP32, BF16])
@pytest.mark.parametrize("rows,V,ldz", sorted({c[:3] for c in GB.XENT}))
def test_xent_geometry_reference_and_planted_logits(dtype, rows, V, ldz):
    z, y, info = RB.xent_inputs(rows, V, seed=rows + V + ldz)
    ref = RB.xent_ref(z, y, 1.0 / rows)
    dz = np.zeros((rows, ldz), dtype=f32)
    dz[:, :V] = RB.store(ref["dz"], dtype)
    res = RB.xent_check(dtype, z, y, 1.0 / rows, dz, ref["loss"].astype(f32), ref["correct"], V)
    assert max(res["worst"].values()) <= 1.0
    assert np.isfinite(RB.xent_emulation(z, y, 1.0 / rows)["loss"]).all()
    if V == 1:
        return
    r = np.arange(rows)
    special = np.zeros(rows, dtype=bool)
    for n in ("tie7", "tie63"):
        if n in info:
            t0, t1 = info[n]
            lo = 7 if n == "tie7" else 63
            special[t0] = special[t1] = True
            both = np.concatenate([t0, t1])
            assert (z[both, lo] == z[both, lo + 1]).all() and (z[both].argmax(-1) == lo).all() and (z[both].max(-1) == z[both, lo]).all()
            assert (ref["correct"][t0] == 1).all() and (ref["correct"][t1] == 0).all() and (y[t1] == lo + 1).all()
    assert (V > 8) == ("tie7" in info) and (V > 64) == ("tie63" in info)
    pr = ref["p"][r, r % V]
    assert (np.abs(pr[~special] - RB.XENT_TARGET) < 0.05).all()            # the raised column, up to the rounding of the logits to fp32
    assert (y[~special] != (r % V)[~special]).all()
    if V <= 1384:
        assert rows >= V and (ref["p"].max(0) >= 0.25).all()             # every column carries weight in some row
    assert (z[info["up"]].min(-1) > 40).all() and (z[info["down"]].max(-1) < -40).all()
    assert (y == 0).any() and (y == V - 1).any()
    # a label taken from the row `stride` further on differs almost everywhere
    stride = 4 * min(-(-rows // 4), 8192)
    if rows > stride:
        assert (y[:rows - stride] != y[stride:]).mean() > 0.9


# ---------------------------------------------------------------------------------------------------------------- dispatch
def test_every_case_reaches_the_kernel_form_its_table_names():
    for rows, E, maxi, per_wave, idle in GB.LN_FWD:
        for d in (FP32, BF16):
            assert GB.reach_ln_fwd(rows, E, d) == (maxi[d], per_wave, idle), (rows, E, d)
    assert any(c[3] == 3 for c in GB.LN_FWD) and {1, 2, 4, 8} == {m for c in GB.LN_FWD for m in c[2].values()}
    for rows, E, dtypes, grid, direct, per_wave, tail, optin in GB.LN_BWD:
        for d in dtypes:
            assert GB.reach_ln_bwd(rows, E, d) == (grid, direct, per_wave, tail, optin), (rows, E, d)
    assert GB.reach_ln_bwd(2048, 64, FP32)[1] and not GB.reach_ln_bwd(2049, 64, FP32)[1]
    assert any(c[7] and FP32 in c[2] and GB.ln_maxi(c[1], FP32) == 8 for c in GB.LN_BWD)
    for rows, V, ldz, off, kernel in GB.XENT:
        assert GB.reach_xent(ldz, off) == kernel, (rows, V, ldz, off)
        if kernel == "xent8" and rows > 32768:
            assert -(-rows // (4 * 8192)) == 3            # waves with 3 and 2 rows: the prefetch
    assert {c[4] for c in GB.XENT} == {"xent8", "generic", "wide"}
    # bf16 rows of at most 2048 columns never need MAXI 8: those instances of the kernels are unreachable
    assert max(GB.ln_maxi(E, BF16) for E in range(8, 2049, 8)) == 4


# ---------------------------------------------------------------------------------------------------------------- what the old metric let through
def rel_err(a, b):
    """tests/test_gpu_kernels.py: max |diff| over max |ref| of the whole tensor."""
    return np.abs(np.asarray(a, np.float64) - b).max() / (np.abs(b).max() + 1e-30)


def test_the_whole_tensor_metric_passed_a_dropped_row_at_32776_rows():
    rows, E = 32776, 64
    inp = RB.ln_inputs(rows, E, FP32, seed=1)
    st = stats32(inp)
    ref = RB.ln_bwd_ref(inp["dy"], inp["x"], inp["gamma"], st[0], st[1])
    start = np.zeros(E, dtype=f32)
    total = ref["tg"].sum(0)
    old_tol = 3e-5 * math.sqrt(rows) * np.abs(total).max()            # test_gpu_kernels / test_gpu_kernel_guards: vtol max |dgamma|
    passed_old = (np.abs(ref["tg"]).max(-1) < old_tol).mean()
    assert passed_old > 0.25                                          # three in ten of all single dropped rows passed (0.30 here)
    q = RB._q(RB.param_grad_emulation(RB.ln_bwd_emulation(inp["dy"], inp["x"], inp["gamma"], st[0], st[1])["tg"], start), total, RB.quad(ref["tg"], start))
    assert q <= 16 * RB.U
    lim = RB.limit_of(q, RB.quad(ref["tg"], start), total, FP32)
    live = ~np.isin(inp["kinds"], ("const", "zero"))
    assert ((np.abs(ref["tg"]) / lim).max(-1)[live] > 1000.0).all()    # ... each of them is a thousand limits now


def test_the_whole_tensor_metric_passed_a_merge_without_its_between_segment_term():
    rows, E = 1500, 1024                                              # a shape of test_gpu_ln_fused
    rng = np.random.default_rng(3)
    old = dict(x=RB.store(rng.normal(1.0, 2.0, (rows, E)), BF16), dy=RB.store(rng.normal(0, 1, (rows, E)), BF16),
               resid=RB.store(rng.normal(0, 1, (rows, E)), BF16), gamma=(1 + 0.3 * rng.normal(size=E)).astype(f32), beta=rng.normal(0, 0.2, E).astype(f32))
    new = RB.ln_inputs(64, E, BF16, seed=3, segments=True)
    seen = {}
    for name, inp in (("old", old), ("new", new)):
        part = RB.parts_of(inp["x"]).astype(f32)
        m = RB.merge_ref(part)
        good = (m["mean"], m["rstd"])
        ref = RB.ln_bwd_ref(inp["dy"], inp["x"], inp["gamma"], good[0], good[1], inp["resid"])
        bad = fake_merge(part, bug="merge_no_between")               # the flawed merge, and the LayerNorm backward on what it wrote
        out = fake_ln_bwd(inp["dy"], inp["x"], inp["gamma"], BF16, 2, starts(E), bad, resid=inp["resid"])
        fails = dict(RB.merge_check(part, bad[0], bad[1], raise_on_fail=False)["fails"])
        fails.update(RB.ln_check(BF16, inp["x"], inp["gamma"], dy=inp["dy"], stats=good, resid=inp["resid"], dx=out["dx"], raise_on_fail=False)["fails"])
        seen[name] = (rel_err(out["dx"], ref["dx"]), np.abs(bad[1] / good[1] - 1.0), fails)
    assert seen["old"][0] < 6e-3                                      # the tolerance of test_gpu_ln_fused on its i.i.d. N(1, 2) rows
    rnd = np.isin(new["kinds"], ("off0.5", "off24", "off300"))        # planted: the rstd of EVERY random row is off by more than that
    assert "rstd" in seen["new"][2] and "dx" in seen["new"][2] and seen["new"][1][rnd].min() > 6e-3
