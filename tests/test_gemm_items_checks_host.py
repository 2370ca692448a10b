"""The cases of tests/test_gpu_gemm_items.py on the CPU: what they reach, that their limits hold what is correct, and that their checks
can fail (the pattern of tests/test_row_checks_host.py).  No device: plans through cmp_gemm_plan on host arenas, kernels as the
item-structured numpy fake of tests/gemm_items_bounds.py (`fake_launch`): every workgroup of the capped grid walks its items in the
kernel's order, static and reversed; each item's epilogue is the correct fp32 formula on its own tile, or wrong in one of the ways the
code between two items can go wrong (BUGS) -- and then the check named beside the bug must reject it.

Record: the whole-tensor metric of tests/test_gpu_ln_fused.py (max |error| over max |reference|, 6e-3 for the fold kinds, 8e-3 for the
residual and scale kinds) on the same planted faults, measured here (`test_record_of_what_the_whole_tensor_metric_lets_through`):
on THESE inputs -- every tile its own offset and scale, so that a fault lands far away -- it lets through only the previous item's
statistics in the residual scale kind (2.8e-3: the rstd of rows whose tile scales are equal every third tile, times a residual of
size 1, against a largest reference of 10) and rejects the rest (0.08 for the dropped between-segment term in the rebuilt residual,
0.3 to 7e3 otherwise; an element never written is NaN and fails any comparison).  On the inputs of test_gpu_ln_fused.py itself (one
offset for all rows, 6 to 12 tiles, one item per workgroup) none of these faults can occur at all.  The metric has no statement about
the column sums beyond 2e-4 of the largest sum (colsum_scaled, colsum_once_per_wg) and none about which slot a partial went to; the
per-element checks reject all eleven.  To see that a class of error is
caught, edit a copy of the fake -- not the library."""
import ctypes as C

import numpy as np
import pytest

import gemm_items_bounds as IB
import row_bounds as RB

# bug -> [(case id, the output whose check must reject it, walked reversed?)]
BUGS = {
    "stats_prev_item": [("A-fold-np2", "C", 0), ("A-fold-gelu-np3", "aux", 1), ("A-scale-resid-np2-K64", "C", 0)],
    "bias_prev_item": [("A-fold-np3", "C", 0), ("A-fold32-np2", "C", 1)],
    "opnd_chunk0_prev": [("A-resid-K320", "C", 0), ("A-gelugrad-K64", "C", 1), ("A-rebuild-np2-p0.1", "C", 0)],
    "merge_no_between": [("A-fold-np2", "C", 0), ("A-rebuild-np3-p0", "C", 1)],
    "fold_no_64d2": [("A-stats-N512-p0", "part_m2", 0), ("A-rebuild-np3-p0.1", "part_m2", 1)],
    "part_prev_slot": [("A-stats-N768-p0.1", "part_mean", 0), ("A-rebuild-np2-p0", "part_mean", 1)],
    "cs_unrounded": [("A-fold32-np3", "C", 0), ("A-fold-np2", "C", 1)],
    "colsum_scaled": [("A-scale-gelugrad-np2-K64", "colsum", 0), ("A-scale-gelugrad-np3-K320", "colsum", 1)],
    "colsum_once_per_wg": [("A-gelugrad+sums-K64", "colsum", 0), ("A-scale-gelugrad-np3-K64", "colsum", 1)],
    "last_item_skipped": [("A-bias-K64", "C", 0), ("A-fold-gelu-np2", "aux", 1)],
    "rev_two_to_one": [("A-none-K64", "C", 1), ("A-stats-N512-p0", "C", 1)],
}
BUG_ROWS = [(b, *row) for b, rows in BUGS.items() for row in rows]
LETS_THROUGH = {("stats_prev_item", "A-scale-resid-np2-K64")}


def mix_cap(case):
    return 6 if case["cap"] == 8 else case["cap"]


def case_of(cid):
    return next(c for c in IB.CASES if c["id"] == cid)


@pytest.fixture(scope="module")
def lib():
    from composer_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def plan_of(lib, case, st, cap, rev):
    from composer_amd import _lib
    IB.arm(lib, case, st, cap, rev)
    info = _lib.GemmPlanInfo()
    rc = lib.cmp_gemm_plan(*st.args, C.byref(info))
    assert rc == 0, (case["id"], lib.cmp_last_error().decode())
    return {n: getattr(info, n) for n, _ in info._fields_}


# ------------------------------------------------------------------------------------------ the plans
@pytest.mark.parametrize("case", IB.CASES, ids=IB.CASE_IDS)
def test_every_case_reaches_its_kernel_form_with_three_items_in_a_workgroup(lib, case):
    o = IB.operands(case)
    try:
        for padded in (True, False):
            st = IB.stage(case, o, padded, device="cpu")
            for rev in case["revs"]:
                p = plan_of(lib, case, st, case["cap"], rev)
                what = (case["id"], padded, p)
                assert (p["family"], p["kind"], p["lnm"], p["np"]) == case["want"], what
                per_cu = 2 if p["family"] == IB.P4_128 else 1
                items = p["ntiles"] * p["nsplit"]
                assert p["grid_x"] == per_cu * case["cap"] and p["sched"] == 1, what
                assert items >= 2 * p["grid_x"] + 1, what                      # some workgroup runs three items
                assert items % p["grid_x"] != 0, what                          # ... and not all of them equally many
                assert p["nsplit"] == case["splitk"], what
                assert p["colsum_fused"] == int(case["colsum"]) and p["colsum_pass"] == 0, what
                if case["kind"] == "wgrad":
                    slabs = p["family"] in (IB.P4_256, IB.P4_128) and case["mode"] == "slab" and not padded
                    assert (p["slabs"], p["swap"]) == (int(slabs), int(slabs)), what
            for cap in IB.caps_of(case)[1:]:
                assert plan_of(lib, case, st, cap, 0)["grid_x"] == min(items, (cap or 256) * per_cu)
        if case["splitk"] == 1:
            # at 8 a workgroup stays inside one XCD group's consecutive tiles; the mixing cap changes the tile row (the rows whose
            # statistics, residual and partial slots an epilogue uses) on every transition between two items of a workgroup
            for rev in case["revs"]:
                ch, n = IB.row_changes(case, mix_cap(case), rev)
                assert n >= 8 and ch == n, (case["id"], rev, ch, n)
    finally:
        assert lib.cmp_gemm_set_workspace(None, 0) == 0


def test_the_walk_covers_every_tile_once_in_both_directions():
    for nitems, ntiles, grid in ((14, 14, 6), (21, 21, 8), (24, 24, 9), (32, 4, 12), (21, 21, 3), (21, 21, 24)):
        for rev in (0, 1):
            seen = [IB.item_tile(i, nitems, ntiles, rev) for w in IB.static_walk(nitems, grid) for i in w]
            assert sorted(seen) == [(s, t) for s in range(nitems // ntiles) for t in range(ntiles)], (nitems, grid, rev)
        counts = [len(w) for w in IB.static_walk(nitems, grid)]
        if nitems >= 2 * grid + 1 and nitems % grid:
            assert max(counts) >= 3 and min(counts) < max(counts)


def test_the_hook_refuses_a_grid_outside_the_scheduler(lib):
    for bad in (-1, 257, 1 << 20):
        assert lib.cmp_gemm_grid_next(bad, 0) != 0 and b"gemm_grid_next" in lib.cmp_last_error()
    assert lib.cmp_gemm_grid_next(256, 1) == 0 and lib.cmp_gemm_grid_next(0, 0) == 0


# ------------------------------------------------------------------------------------------ what is correct is inside every limit
def stored_reference(case, o):
    """The float64 references as a perfect kernel would store them."""
    refs = IB.reference_cached(case, o)
    outs = {}
    for name in ("C", "aux"):
        if name in refs:
            ref, _, bf = refs[name]
            outs[name] = RB.store(ref, IB.BF16).astype(np.float64) if bf else ref.astype(np.float32).astype(np.float64)
    if case["lnm"] & 2:
        outs["part"] = RB.parts_of(outs["C"]).astype(np.float32).astype(np.float64).reshape(case["M"], -1)
    if case["colsum"]:
        src = refs["_prod"][0] if case["kind"] == "scale-gelugrad" else outs["C"]
        outs["colsum"] = (IB.colsum_start(case["N"]).astype(np.float64) + src.sum(0)).astype(np.float32).astype(np.float64)
    return outs


@pytest.mark.parametrize("case", IB.CASES, ids=IB.CASE_IDS)
def test_reference_and_correct_emulation_sit_inside_every_limit(case):
    o = IB.operands(case)
    start = IB.colsum_start(case["N"]) if case["colsum"] else None
    w = IB.check_outputs(case, o, stored_reference(case, o), case["id"] + " reference as stored", colsum_start=start)
    assert all(v <= 1.0 for v in w.values()), w
    if case["kind"] == "wgrad":
        emu = {"C": (o["ref"].astype(np.float32) + o["c0"].astype(np.float32)).astype(np.float64)}
        assert max(IB.check_outputs(case, o, emu, case["id"] + " emulation").values()) <= 1.0
        return
    for rev in case["revs"]:
        for cap in {case["cap"], mix_cap(case)}:
            emu = IB.fake_launch(case, o, cap, rev)
            w = IB.check_outputs(case, o, emu, case["id"] + " emulation rev %d cap %d" % (rev, cap), colsum_start=start)
            assert all(v <= 1.0 for v in w.values()), w


@pytest.mark.parametrize("cid", ["A-fold-np2", "A-fold-np3", "A-fold32-np2"])
def test_statistics_of_another_tile_move_every_row_by_ten_limits(cid):
    """The planted per-tile offsets and scales: with the (mean, rstd) of rows r +- 256 in place of its own, some element of EVERY row
    of both tiles is at least ten limits away from its reference."""
    case = case_of(cid)
    o = IB.operands(case)
    ref, lim, bf = IB.reference_cached(case, o)["C"]
    full = lim + (IB.BF16_OUT * np.abs(ref) if bf else 0.0)
    mu, rs, _, _, share = IB.merged(o["part"])
    random_rows = ~np.isin(o["kinds"], ("const", "zero", "outlier"))        # (an outlier of 200 sigma is most of its row's M2)
    assert share[random_rows].min() >= RB.SEG_SHARE_MIN
    for ta, tb in ((0, 1), (2, 5), (6, 3)):
        perm = np.arange(case["M"])
        perm[ta * 256:(ta + 1) * 256], perm[tb * 256:(tb + 1) * 256] = np.arange(tb * 256, (tb + 1) * 256), np.arange(ta * 256, (ta + 1) * 256)
        wrong, _ = IB.fold_reference(o, case["N"], stats=(mu[perm], rs[perm]))
        moved = (np.abs(wrong - ref) / np.maximum(full, 1e-300)).max(-1)
        rows = np.r_[ta * 256:(ta + 1) * 256, tb * 256:(tb + 1) * 256]
        assert moved[rows].min() >= 10.0, (cid, ta, tb, int(rows[moved[rows].argmin()]), moved[rows].min())


# ------------------------------------------------------------------------------------------ the planted faults
@pytest.mark.parametrize("bug,cid,name,rev", BUG_ROWS)
def test_every_planted_fault_is_rejected_by_its_named_check(bug, cid, name, rev):
    case = case_of(cid)
    o = IB.operands(case)
    start = IB.colsum_start(case["N"]) if case["colsum"] else None
    for cap in {case["cap"], mix_cap(case)}:
        good = IB.fake_launch(case, o, cap, rev)
        assert max(IB.check_outputs(case, o, good, cid, colsum_start=start).values()) <= 1.0
        bad = IB.fake_launch(case, o, cap, rev, bug=bug)
        with pytest.raises(AssertionError, match=r": %s, " % name):
            IB.check_outputs(case, o, bad, cid, colsum_start=start)


def whole_tensor_metric(got, ref):
    return np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30)


def test_record_of_what_the_whole_tensor_metric_lets_through():
    """max |error| / max |reference| of C at the thresholds of tests/test_gpu_ln_fused.py (6e-3 fold kinds, 8e-3 the others): the
    planted faults it passes are exactly LETS_THROUGH (a NaN -- an element never written -- fails any comparison)."""
    passed = set()
    for bug, cid, name, rev in BUG_ROWS:
        if name in ("colsum", "part_mean", "part_m2"):
            continue                                  # (the metric is about C / aux only)
        case = case_of(cid)
        o = IB.operands(case)
        bad = IB.fake_launch(case, o, case["cap"], rev, bug=bug)
        ref = IB.reference_cached(case, o)[name][0]
        m = whole_tensor_metric(bad[name], ref)
        print(" whole-tensor metric of %s on %s: %.3g" % (bug, cid, m))
        if m < (6e-3 if case["kind"].startswith("fold") else 8e-3):
            passed.add((bug, cid))
    assert passed == LETS_THROUGH, passed
