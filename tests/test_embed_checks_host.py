"""CPU proof that the embedding checks of tests/embed_bounds.py bite: numpy "kernels" with one planted bug each must fail the check
named for them, the correct ones must pass, every row of the GPU case tables (tests/test_gpu_embed_bounds.py) must reach the path it names
(`reach_*` against the tables, the form against the library's own cmp_embed_bwd_form), and the planted token counts must be what the
tables promise.  One test measures what the whole-tensor metric the older tests use lets through.  No GPU."""
import numpy as np
import pytest
import torch

import embed_bounds as EB
import row_bounds as RB
import test_gpu_embed_bounds as GB
from attention_bounds import bf16r

FP32, BF16 = 0, 1
f32 = np.float32
SEED, STREAM, POS0 = 5, 2, 3
# the backward case of the planted bugs: 4125 tokens, B odd, planted counts (embed_bounds.PLANTED), p > 0
B_, T_, E_, V_, P_ = 33, 125, 64, 390, 0.2
COLD, HOT = 2, 5                   # ids with exactly 1 and exactly 129 tokens

BWD_BUGS = ("cold_token_dropped", "token_credited_to_next_id", "row_128_dropped", "row_128_twice", "chunk_partial_bf16", "dwte_overwritten",
            "last_batch_row_twice", "pos0_ignored", "mask_row_is_t")
FWD_BUGS = ("truncating_store", "scale_before_add", "type_on_the_wrong_side")
ISSUE_BUGS = BWD_BUGS + FWD_BUGS


@pytest.fixture(scope="module")
def inp():
    return EB.bwd_inputs(B_, T_, E_, V_, BF16, POS0, seed=11)


def fake_bwd(inp, B, T, pos0, p, dtype, bug=None, order=3, cold=COLD, hot=HOT):
    """The sorted form in numpy (embed_bounds' emulation under arrival order `order`) with one planted bug -> dwte, dwpe."""
    ids = np.asarray(inp["ids"]).astype(np.int64).copy()
    ntok, E = inp["dh"].shape
    keep = None
    if bug == "mask_row_is_t":
        keep = np.tile(EB.keep_of(T, E, p, SEED, STREAM), (B, 1))
    t32, _ = EB.summands(inp["dh"], p, SEED, STREAM, keep=keep)
    t32 = t32.copy()
    tok = int(np.flatnonzero(ids == cold)[0])
    start, tamper, rounder = inp["dwte0"], None, None
    if bug == "cold_token_dropped":
        t32[tok] = 0
    elif bug == "token_credited_to_next_id":
        ids[tok] = cold + 1
    elif bug == "row_128_dropped":
        tamper = lambda v, toks: np.delete(toks, 128) if v == hot else toks
    elif bug == "row_128_twice":
        tamper = lambda v, toks: np.insert(toks, 128, toks[128]) if v == hot else toks
    elif bug == "chunk_partial_bf16":
        rounder = bf16r
    elif bug == "dwte_overwritten":
        start = np.zeros_like(inp["dwte0"])
    dwte = EB.dwte_sorted_emulation(ids, t32, start, dtype, order, tamper, rounder)
    dwpe = inp["dwpe0"].copy()
    rows = slice(0, T) if bug == "pos0_ignored" else slice(pos0, pos0 + T)
    dwpe[rows] = EB.dwpe_pairs_emulation(t32, B, T, dwpe[rows], dtype, tail_bug=bug == "last_batch_row_twice")
    return dwte, dwpe


def check_bwd(inp, B, T, p, dtype, dwte, dwpe):
    return EB.embed_bwd_check(1, dtype, inp["ids"], inp["dh"], B, T, POS0, p, SEED, STREAM, inp["dwte0"], inp["dwpe0"], dwte, dwpe,
                              raise_on_fail=False)


def small_rp1():
    """B = 3 at RP = 1 (fp32, E = 1024): the pair loop's odd tail is the last batch row."""
    return EB.bwd_inputs(3, 5, 1024, 20, FP32, POS0, seed=3), 3, 5, FP32


def run_bwd_bug(inp, bug, p=P_):
    if bug == "last_batch_row_twice":
        sm, B, T, dt = small_rp1()
        assert EB.rp_of(1024, dt)[1] == 1
        return check_bwd(sm, B, T, p, dt, *fake_bwd(sm, B, T, POS0, p, dt, bug, cold=int(sm["ids"][0]), hot=-1))
    return check_bwd(inp, B_, T_, p, BF16, *fake_bwd(inp, B_, T_, POS0, p, BF16, bug))


# ---------------------------------------------------------------------------------------------------------------- forward fakes
def fwd_case(dtype=BF16):
    rng = np.random.default_rng(7)
    B, T, E, V = 3, 17, 64, 390
    ids = rng.integers(0, V, B * T).astype(np.int32)
    wte, wpe = rng.normal(0, 1, (V, E)).astype(f32), rng.normal(0, 1, (POS0 + T, E)).astype(f32)
    return dict(ids=ids, wte=wte, wpe=wpe, T=T, type_ids=rng.integers(0, V, B * T).astype(np.int32), p=0.3, dtype=dtype)


def fake_fwd(c, bug=None):
    a, pz, ty = EB.embed_rows(c["ids"], c["wte"], c["wpe"], c["T"], POS0, None, c["type_ids"])
    sc = RB.drop_scale(c["p"])
    keep = EB.keep_of(a.shape[0], a.shape[1], c["p"], SEED, STREAM)
    if bug == "scale_before_add":
        v = (a * sc + pz * sc) + ty * sc
    elif bug == "type_on_the_wrong_side":
        v = ((a + ty) + pz) * sc
    else:
        v = ((a + pz) + ty) * sc
    v = np.where(keep, v, f32(0))
    if bug == "truncating_store" and c["dtype"] == BF16:
        return (np.ascontiguousarray(v).view(np.uint32) & np.uint32(0xFFFF0000)).view(f32)
    return EB.store(v, c["dtype"])


def check_fwd(c, out):
    fails = {}
    EB.embed_fwd_check(c["dtype"], out, c["ids"], c["wte"], c["wpe"], c["T"], POS0, c["p"], SEED, STREAM, None, c["type_ids"], fails=fails)
    return fails


# ---------------------------------------------------------------------------------------------------------------- the checks bite
@pytest.mark.parametrize("p", [0.0, P_])
@pytest.mark.parametrize("order", [0, 3, 7])
def test_the_correct_sorted_fake_sits_inside_every_limit(inp, order, p):
    res = check_bwd(inp, B_, T_, p, BF16, *fake_bwd(inp, B_, T_, POS0, p, BF16, None, order))
    assert not res["fails"], res["fails"]
    assert res["worst"]["dwte"] <= 1.0 and res["worst"]["dwpe"] <= 1.0


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("form", [0, 2])
def test_the_correct_atomic_and_atomic_free_fakes_sit_inside_every_limit(form, p):
    c = EB.bwd_inputs(4, 25, 64, 50, FP32, POS0, seed=5)
    t32, _ = EB.summands(c["dh"], p, SEED, STREAM)
    ids = c["ids"].astype(np.int64)
    dwte = EB.dwte_emulation(form, ids, t32, c["dwte0"], FP32, order=4)
    dwpe = c["dwpe0"].copy()
    dwpe[POS0:] = EB.dwpe_seq_emulation(t32, 4, 25, dwpe[POS0:])
    res = EB.embed_bwd_check(form, FP32, c["ids"], c["dh"], 4, 25, POS0, p, SEED, STREAM, c["dwte0"], c["dwpe0"], dwte, dwpe, raise_on_fail=False)
    assert not res["fails"], res["fails"]
    # a one-ulp change of one element of the atomic-free dwte is caught at p = 0 (bit equality), not by the bound
    if form == 2 and p == 0:
        dwte[ids[0], 0] = np.nextafter(dwte[ids[0], 0], f32(np.inf))
        bad = EB.embed_bwd_check(2, FP32, c["ids"], c["dh"], 4, 25, POS0, p, SEED, STREAM, c["dwte0"], c["dwpe0"], dwte, dwpe, raise_on_fail=False)
        assert "dwte" in bad["fails"]


@pytest.mark.parametrize("bug", BWD_BUGS)
def test_a_wrong_backward_kernel_is_rejected(inp, bug):
    res = run_bwd_bug(inp, bug)
    assert res["fails"], "the planted bug %s passed: %s" % (bug, res["worst"])
    want = {"last_batch_row_twice": "dwpe", "mask_row_is_t": "dwte"}.get(bug, "dwpe" if bug == "pos0_ignored" else "dwte")
    assert any(k.startswith(want) for k in res["fails"]), (bug, list(res["fails"]))


@pytest.mark.parametrize("bug", FWD_BUGS)
def test_a_wrong_forward_kernel_is_rejected(bug):
    """The store bug in bf16; the two arithmetic bugs in fp32, where every differing sum shows.  (In bf16 a one-ulp fp32 difference reaches
    the stored value only where it straddles a rounding boundary, about one element in 2^16: none of this case's 3264, some hundred of
    the 8.4 million of the GPU suite's 4100 x 2048 case.)"""
    c = fwd_case(BF16 if bug == "truncating_store" else FP32)
    good, bad = fake_fwd(c), fake_fwd(c, bug)
    assert not check_fwd(c, good), "the correct forward fake must pass"
    assert check_fwd(c, bad), "the planted bug %s passed" % bug
    # ... and the whole-tensor tolerance of the older tests (1e-2 of the largest element in bf16, 1e-6 in fp32) lets it through
    old = np.abs(bad.astype(np.float64) - good).max() / np.abs(good).max()
    assert 0 < old < (1e-2 if c["dtype"] == BF16 else 1e-6), old


@pytest.mark.parametrize("dtype", [FP32, BF16])
def test_the_forward_check_counts_a_negative_zero(dtype):
    c = fwd_case(dtype)
    out = fake_fwd(c).copy()
    z = np.argwhere(out == 0)[0]
    out[tuple(z)] = f32(-0.0)
    assert check_fwd(c, out)


def test_every_issue_bug_has_a_test():
    assert len(ISSUE_BUGS) == 12 and len(set(ISSUE_BUGS)) == 12


def test_the_statistics_check_passes_both_emulations_and_rejects_a_segment_taken_from_the_neighbour():
    c = fwd_case()
    rng = np.random.default_rng(1)
    wte, wpe = (rng.normal(0, 1, (390, 512)) + 0.75).astype(f32), rng.normal(0, 1, (POS0 + 17, 512)).astype(f32)
    out = EB.embed_fwd_emulation(c["ids"], wte, wpe, 17, POS0, BF16, 0.1, SEED, STREAM)
    for emu in EB.stats_emulations(out):
        res = EB.embed_stats_check(out, emu, c["ids"], wte, wpe, 17, POS0, 0.1, SEED, STREAM, raise_on_fail=False)
        assert not res["fails"], res["fails"]
    bad = EB.stats_emulations(out)[0].copy()
    bad[5, 0] = bad[5, 1]
    assert EB.embed_stats_check(out, bad, c["ids"], wte, wpe, 17, POS0, 0.1, SEED, STREAM, raise_on_fail=False)["fails"]
    # an M2 summed as sum x^2 - 256 mu^2 in float32 (the cancellation the kernel's two passes avoid) is outside the limit
    shifted = EB.embed_fwd_emulation(c["ids"], wte + f32(40), wpe, 17, POS0, BF16, 0.0)
    nv = EB.stats_emulations(shifted)[0].copy()
    xs = shifted.reshape(shifted.shape[0], 2, 256)
    nv[..., 1] = RB.seq_sum32(xs * xs) - f32(256) * nv[..., 0] * nv[..., 0]
    assert EB.embed_stats_check(shifted, nv, c["ids"], wte + f32(40), wpe, 17, POS0, 0.0, raise_on_fail=False)["fails"]


def test_fold_by_id_is_atomics_fold_per_id():
    rng = np.random.default_rng(2)
    rows = rng.normal(0, 1, (300, 8)).astype(f32)
    ids = rng.integers(0, 3, 300)
    start = rng.normal(0, 1, (3, 8)).astype(f32)
    for order in (0, 1, 5):
        seq = EB.arrival(300, order)
        got = EB.fold_by_id(start.copy(), ids, rows, seq)
        for v in range(3):
            mine = seq[ids[seq] == v]
            want = RB.atomics_fold(rows[mine], start[v], 0)
            assert np.array_equal(got[v], want)


def test_colsum_emulation_is_inside_the_float64_bound_and_a_dropped_row_is_not():
    rng = np.random.default_rng(4)
    for rows, cols, dtype in ((37, 392, BF16), (130, 64, FP32), (8193, 64, BF16)):
        x = EB.store(rng.normal(0.3, 1, (rows, cols)), dtype)
        start = rng.normal(0, 3, cols).astype(f32)
        good = EB.colsum_det_emulation(x, start, dtype)
        assert EB.colsum_det_check(dtype, x, start, good) <= 1.0
        y = x.copy()
        y[rows - 1] = 0                                    # the last row never read
        with pytest.raises(AssertionError):
            EB.colsum_det_check(dtype, x, start, EB.colsum_det_emulation(y, start, dtype))


# ---------------------------------------------------------------------------------------------------------------- the tables reach what they name
@pytest.fixture(scope="module")
def lib():
    from composer_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def lib_form(lib, B, T, E, dtype, V, sort_ws, det):
    words = int(lib.cmp_embed_bwd_sort_ws_words(B * T, V)) if sort_ws else 0
    assert words == (EB.sort_ws_words_of(B * T, V) if sort_ws else 0)
    return int(lib.cmp_embed_bwd_form(B, T, E, dtype, V, words, int(det)))


def test_every_backward_case_takes_the_form_its_table_names(lib):
    for B, T, E, V, geo, scan_per in GB.SORTED:
        assert B * T in (4096, 4097, 4098, 4100)
        for d in (FP32, BF16):
            r = EB.reach_embed_bwd(B, T, E, d, V, EB.sort_ws_words_of(B * T, V))
            assert r["form"] == 1 == lib_form(lib, B, T, E, d, V, True, False)
            assert (r["CPR"], r["RP"], r["idle"], r["trips"]) == geo[d] and r["scan_per"] == scan_per, (B, T, E, V, d, r)
    for B, T, E, V, form in GB.THRESHOLD:
        for d in (FP32, BF16):
            assert EB.reach_embed_bwd(B, T, E, d, V, EB.sort_ws_words_of(B * T, V))["form"] == form == lib_form(lib, B, T, E, d, V, True, False)
    assert [c[0] * c[1] for c in GB.THRESHOLD] == [4095, 4096, 4096] and GB.THRESHOLD[2][3] == 8193
    for B, T, E, V in GB.ATOMIC:
        for d in (FP32, BF16):
            assert EB.reach_embed_bwd(B, T, E, d, V, 0)["form"] == 0 == lib_form(lib, B, T, E, d, V, False, False)
            # what test_embedding_guarded used to call its sorted launch: 51 tokens with a sort workspace are the atomic form again
            assert lib_form(lib, B, T, E, d, V, True, False) == 0
    for B, T, E, V, per, empty in GB.DET:
        for d in (FP32, BF16):
            r = EB.reach_embed_bwd(B, T, E, d, V, 0, det=True)
            assert (r["form"], r["per"], r["empty"]) == (2, per, empty) and lib_form(lib, B, T, E, d, V, False, True) == 2
            assert int(lib.cmp_k_embed_bwd_det_ws(V, E)) == V * EB.EMB_SEG * E * 4
    # the remaining fall-backs of the launcher: a short workspace, E no multiple of the vector width
    words = EB.sort_ws_words_of(4096, 390)
    assert int(lib.cmp_embed_bwd_form(4, 1024, 64, FP32, 390, words - 1, 0)) == 0 == EB.reach_embed_bwd(4, 1024, 64, FP32, 390, words - 1)["form"]
    assert int(lib.cmp_embed_bwd_form(4, 1024, 12, BF16, 390, words, 0)) == 0 == EB.reach_embed_bwd(4, 1024, 12, BF16, 390, words)["form"]
    assert int(lib.cmp_embed_bwd_form(4, 1024, 12, FP32, 390, words, 0)) == 1 == EB.reach_embed_bwd(4, 1024, 12, FP32, 390, words)["form"]


def test_the_sorted_cases_cover_what_the_issue_lists():
    seen = dict(cpr1=False, cpr_odd=False, cpr_over=False, b1=False, b_2rp1=False)
    for B, T, E, V, geo, scan_per in GB.SORTED:
        for d in (FP32, BF16):
            cpr, rp, idle, trips = geo[d]
            seen["cpr1"] |= cpr == 1
            seen["cpr_odd"] |= 256 % cpr != 0 and cpr < 256
            seen["cpr_over"] |= d == FP32 and cpr > 256 and trips == 2
            seen["b1"] |= B == 1
            seen["b_2rp1"] |= B == 2 * rp + 1
        assert B == 1 or B % 2 == 1
    assert all(seen.values()), seen
    assert {c[3] for c in GB.SORTED} == {1, 3, 390, 1024, 1025, 8192} and {c[2] for c in GB.SORTED} == {8, 24, 64, 768, 2048}
    assert {EB.cdiv(V, 1024) for V in (1024, 1025, 8192)} == {1, 2, 8}


@pytest.mark.parametrize("B,T,E,V", [c[:4] for c in GB.SORTED])
def test_the_planted_token_counts(B, T, E, V):
    ids = EB.bwd_inputs(B, T, 8, V, FP32, POS0, seed=B * T + E + V)["ids"]
    n = np.bincount(ids, minlength=V)
    assert ids.min() == 0 and ids.max() == V - 1 and n[0] > 0 and n[V - 1] > 0
    if V >= 8:
        assert [int(n[v]) for v, _ in EB.PLANTED] == [c for _, c in EB.PLANTED] == [0, 1, 127, 128, 129]
        assert n.max() > 2 * EB.EMB_CH                     # a hot id of several chunks
    elif V == 3:
        assert n[1] == 128 and n[2] == 129
    else:
        assert n[0] == B * T


def test_every_forward_and_column_sum_case_reaches_the_path_its_table_names(lib):
    for B, T, E, V, trips in GB.FWD:
        for d in (FP32, BF16):
            assert EB.reach_embed_fwd(B * T, E, d)[1] == trips[d], (B, T, E, d)
    assert EB.reach_embed_fwd(5 * 820, 2048, BF16)[0] == 4096 and 4100 * 2048 // 8 > 4096 * 256
    for B, T, E, maxi, trips, ragged in GB.STATS:
        assert EB.reach_embed_stats(B * T, E) == (maxi, trips, ragged), (B, T, E)
    assert {c[2] for c in GB.STATS} == {256, 512, 768, 1280, 1536, 2048}
    for rows, cols, ldx, dts, splits, empty, capped in GB.COLSUM:
        for d in dts:
            r = EB.reach_colsum(rows, cols, d)
            assert (r[0], r[2], r[3]) == (splits, empty, capped), (rows, cols, d, r)
            assert int(lib.cmp_k_colsum_det_ws(rows, cols, d)) == splits * cols * 4


# ---------------------------------------------------------------------------------------------------------------- the old metric
OLD_METRIC_PASSED = ()


def test_the_whole_tensor_metric_on_the_sorted_form_inputs_measured():
    """The metric of test_gpu_kernels.py::test_embedding_bwd_sorted_form -- max |out - ref| / max |ref| < 2e-5 over the whole of dwte and of
    dwpe -- on that test's own inputs, case (B, T, E, V, p) = (8, 512, 512, 390, 0.3) in fp32 (half of the 4096 tokens on three ids),
    applied to the planted bugs above (the batch is even, so the odd-batch bug does not apply).

    Measured: it lets NONE of them through.  The gradients are N(0, 1) draws, so the hottest row is a sum of some 700 rows of random sign
    and max |ref| is 127, not 700: the allowance 2e-5 max |ref| = 2.5e-3 is, on the rows of ids with a dozen tokens or fewer, a median
    of 21 000 fp32 ulps of the element (asserted below: more than 1 000) -- loose, but a whole token row (error about 4.7, metric
    3.7e-2), a chunk partial kept in bf16 (1.5e-3), an overwritten accumulator (3.7e-2) and a mask taken from the wrong row (0.55) all
    exceed it.  What the old metric cannot see is an error below those thousands of ulps on a cold row; the per-element check holds
    every element to MARGIN max(q, u) S, a few ulps of its own accumulation, rejects every planted bug here too, and names the element."""
    B, T, E, V, p = 8, 512, 512, 390, 0.3
    g = torch.Generator().manual_seed(B * T + V)
    ids = torch.randint(0, V, (B, T), generator=g, dtype=torch.int32)
    hot = torch.rand(B, T, generator=g) < 0.5
    ids[hot] = torch.randint(0, min(V, 3), (int(hot.sum()),), generator=g, dtype=torch.int32)
    W = T + 5
    dh = torch.randn(B * T, E, generator=g)
    dwte0, dwpe0 = torch.randn(V, E, generator=g), torch.randn(W, E, generator=g)
    c = dict(ids=ids.reshape(-1).numpy(), dh=dh.numpy(), dwte0=dwte0.numpy(), dwpe0=dwpe0.numpy())
    n = np.bincount(c["ids"], minlength=V)
    cold = int(np.flatnonzero(n[:V - 1] == n[:V - 1][n[:V - 1] > 0].min())[0])
    hot_id = int(n.argmax())
    assert n[hot_id] > 129 and n[cold] <= 12
    _, t64 = EB.summands(c["dh"], p, SEED, STREAM)
    rw, _ = EB.acc_ref(c["dwte0"], t64, c["ids"].astype(np.int64))
    rp = c["dwpe0"].astype(np.float64).copy()
    rp[2:2 + T] += t64.reshape(B, T, E).sum(0)

    def old_metric_passes(dwte, dwpe):
        rel = lambda a, b: float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())
        return rel(dwte, rw) < 2e-5 and rel(dwpe, rp) < 2e-5

    passed, figures = [], {}
    for bug in (None,) + BWD_BUGS:
        if bug == "last_batch_row_twice":
            continue
        dwte, dwpe = fake_bwd(c, B, T, 2, p, FP32, bug, order=3, cold=cold, hot=hot_id)
        ok = old_metric_passes(dwte, dwpe)
        figures[bug] = float(np.abs(dwte.astype(np.float64) - rw).max() / np.abs(rw).max())
        if bug is None:
            assert ok, "the correct fake must pass the old metric"
        else:
            if ok:
                passed.append(bug)
            # ... and the per-element check rejects every one of them on the same inputs
            res = EB.embed_bwd_check(1, FP32, c["ids"], c["dh"], B, T, 2, p, SEED, STREAM, c["dwte0"], c["dwpe0"], dwte, dwpe, raise_on_fail=False)
            assert res["fails"], bug
    coldrows = (n > 0) & (n <= 12)
    ulps = 2e-5 * np.abs(rw).max() / np.spacing(np.abs(rw[coldrows]).astype(f32)).astype(np.float64)
    print("OLD_METRIC passed:", passed, {k: "%.2e" % v for k, v in figures.items()}, "max |ref| %.1f" % np.abs(rw).max(),
          "allowance on cold rows, median fp32 ulps %.0f" % np.median(ulps))
    assert tuple(passed) == OLD_METRIC_PASSED, passed
    assert np.median(ulps) > 1000
