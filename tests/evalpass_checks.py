"""What the kernel-level tests of the validation pass (cmp_k_eval_rows, composer_amd/csrc/evalpass.hip) assert about one launch, apart
from the launch itself: the inputs, the NumPy restatement of the table and the comparison.  tests/test_gpu_evalpass_kernel.py runs
them on the device, tests/test_evalpass_checks_host.py on deliberately wrong fakes (no GPU).

Inputs (`make_case`): fp32 logits N(0, 3) [rows, V]; about half the targets are the row's argmax (so `correct` is not all zero), the
others uniform in [0, V - 1) -- id V - 1 is never a target, so with the six event classes the last class has no row.  From 8 rows on,
the special rows: an exact tie at the maximum with the target on the higher index (two rows, not correct) and on the lower (one row,
correct; two against one, so that breaking ties the other way changes the sum of every class set), a row with one -inf column, and
targets -1 and V (counted nowhere).

Expected (`expected_table`): count and correct exactly -- correct = (rank == 0), rank = #{c : z[c] > z[y] or (z[c] == z[y] and c < y)}
on the fp32 values; nll[c] = the float64 sum of the fp32 -logp values handed in (on the device: what cmp_k_score_rows returns for the
same logits).  Bound on nll: count[c] * 2^-52 relative, which holds for ANY order of a float64 sum of count non-negative terms
(tests/test_gpu_train_clip_accum.py uses the same for the gradient norm's squares)."""
import numpy as np

SLOTS = 9
V_DEFAULT = 390
# n -> the disjoint half-open id ranges of the case (inside [0, 390)): none; the six event classes of the default vocabulary; eight ranges
# that leave 288 .. 299 to the "every other id" slot
CLASS_SETS = {
    0: [],
    6: [(0, 128), (128, 256), (256, 288), (288, 388), (388, 389), (389, 390)],
    8: [(300, 388), (0, 50), (50, 100), (100, 128), (128, 256), (256, 288), (388, 389), (389, 390)],
}
R_TIE_HI, R_TIE_LO, R_INF, R_NEG, R_V, R_TIE_HI2 = 1, 2, 3, 4, 5, 6


def make_case(rows, V=V_DEFAULT, seed=0):
    rng = np.random.default_rng([rows, V, seed])
    z = (rng.standard_normal((rows, V)) * 3).astype(np.float32)
    y = rng.integers(0, V - 1, rows).astype(np.int32)
    best = rng.random(rows) < 0.5
    y[best] = np.minimum(z.argmax(-1)[best], V - 2)
    if rows >= 8:
        z[R_TIE_HI, 10] = z[R_TIE_HI, 20] = 50.0; y[R_TIE_HI] = 20
        z[R_TIE_LO, 10] = z[R_TIE_LO, 20] = 50.0; y[R_TIE_LO] = 10
        z[R_INF, 7] = -np.inf; y[R_INF] = 200
        y[R_NEG] = -1
        y[R_V] = V
        z[R_TIE_HI2, 30] = z[R_TIE_HI2, 300] = 50.0; y[R_TIE_HI2] = 300
    return z, y


def class_of(y, ranges, V):
    """Slot of every target: the range that holds it, len(ranges) for every other id, -1 outside [0, V)."""
    y = np.asarray(y, np.int64)
    cls = np.full(y.shape, len(ranges), np.int64)
    for c, (lo, hi) in enumerate(ranges):
        cls[(y >= lo) & (y < hi)] = c
    cls[(y < 0) | (y >= V)] = -1
    return cls


def rank0(z, y, V):
    """correct per row: no column above z[y], none equal to it at a lower index (False where y is outside [0, V))."""
    z = np.asarray(z, np.float32)
    valid = (y >= 0) & (y < V)
    yc = np.where(valid, y, 0)
    zy = z[np.arange(len(y)), yc]
    col = np.arange(z.shape[1])
    rank = ((z > zy[:, None]) | ((z == zy[:, None]) & (col[None, :] < yc[:, None]))).sum(-1)
    return valid & (rank == 0)


def logp_fp32(z, y, V):
    """-logp restated in numpy fp32 (the host fakes' stand-in for cmp_k_score_rows): 0 where y is outside [0, V)."""
    z = np.asarray(z, np.float32)
    valid = (y >= 0) & (y < V)
    yc = np.where(valid, y, 0)
    mx = z.max(-1)
    ls = np.log(np.exp(z - mx[:, None]).sum(-1, dtype=np.float32))
    return np.where(valid, z[np.arange(len(y)), yc] - (mx + ls), 0).astype(np.float32)


def expected_table(z, y, ranges, logp, V):
    """(nll float64 [9], count int64 [9], correct int64 [9]) of the restatement; logp: fp32 per row."""
    cls = class_of(y, ranges, V)
    ok = rank0(z, y, V)
    nll, count, correct = np.zeros(SLOTS), np.zeros(SLOTS, np.int64), np.zeros(SLOTS, np.int64)
    terms = -np.asarray(logp, np.float32).astype(np.float64)
    for c in range(len(ranges) + 1):
        sel = cls == c
        nll[c], count[c], correct[c] = terms[sel].sum(), sel.sum(), (ok & sel).sum()
    return nll, count, correct


def check_table(got, want, n, what=""):
    """got, want: (nll, count, correct).  Integers exactly, slots above n zero, nll within count * 2^-52 relative."""
    g_nll, g_cnt, g_cor = (np.asarray(a) for a in got)
    w_nll, w_cnt, w_cor = (np.asarray(a) for a in want)
    assert g_cnt.tolist() == w_cnt.tolist(), "%s: count %s, restatement %s" % (what, g_cnt.tolist(), w_cnt.tolist())
    assert g_cor.tolist() == w_cor.tolist(), "%s: correct %s, restatement %s" % (what, g_cor.tolist(), w_cor.tolist())
    assert not g_cnt[n + 1:].any() and not g_cor[n + 1:].any() and not g_nll[n + 1:].any(), "%s: a slot above n = %d is not zero" % (what, n)
    lim = w_cnt * 2.0 ** -52 * np.abs(w_nll)
    bad = ~(np.abs(g_nll - w_nll) <= lim)
    assert not bad.any(), "%s: nll %s, restatement %s (limit %s)" % (what, g_nll[bad].tolist(), w_nll[bad].tolist(), lim[bad].tolist())
