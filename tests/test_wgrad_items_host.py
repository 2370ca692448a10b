"""The cases of tests/test_gpu_wgrad_items.py on the CPU (tables, operands, references, emulations: tests/wgrad_items_cases.py): that
every row reaches what it names -- asserted from cmp_wgrad_group_plan with the same max_wgs and flags = 2, never assumed --, that what
is correct sits inside every limit, and that each new check can fail (the manner of tests/test_gemm_items_checks_host.py): a fold fed
one K range twice, a fold that takes a slot of another launch, a fold in another order, column sums added to another problem's
vector, an item's guards taken from the next item's problem.  No device: the kernels are numpy walks of the plan's item table."""
import numpy as np
import pytest

import wgrad_items_cases as W


@pytest.fixture(scope="module")
def lib():
    from composer_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


# ------------------------------------------------------------------------------------------ what the rows reach
@pytest.mark.parametrize("K", W.DEPTHS)
def test_p8_rows_run_several_items_of_different_problems_per_workgroup(lib, K):
    for cap in W.CAPS:
        d, rows = W.plan(lib, W.P8, K, cap)
        want = W.P8_ROWS[cap]
        assert (d["tiles"], d["nitems"], d["grid"], d["wgs"], d["nk"], d["nslots"]) == (want["tiles"], 34, cap, cap, K // 32, 0), (cap, d)
        assert d["nitems"] > d["grid"]
        assert {len(w) for w in W.static_walk(d)} == want["per_wg"], cap
        assert W.ranges_histogram(rows) == {1: 34}                       # every element of C receives exactly one addition
        assert sorted(rows[:, 7].tolist()) == list(range(34)) and (rows[:, 3] == 0).all() and (rows[:, 4] == K // 32).all()
        if cap in (8, 16):
            assert W.cross_pairs(d, rows) >= W.MIN_CROSS, (cap, W.cross_pairs(d, rows))      # (6 at cap 8, 7 at cap 16)
            after, before = W.bias_switches(d, rows, W.P8_BIAS)
            assert after >= 1 and before >= 1, (cap, after, before)      # a summing item next to another problem's, on both sides
    d, rows = W.plan(lib, W.P8, K, 8)
    assert W.with_without_with(d, rows, W.P8_BIAS)
    assert len(W.P8_BIAS) == 3 and len(W.P8) == 8
    # without a cap: one item per workgroup; one K range per tile only at one k-step (the bitwise comparison includes it there)
    d, rows = W.plan(lib, W.P8, K, 0)
    assert d["grid"] == d["nitems"] and W.ranges_histogram(rows) == ({1: 34} if K == 32 else {2: 34})


@pytest.mark.parametrize("rid", W.S3_ROW_IDS)
def test_s3_rows_cut_the_tiles_as_the_table_says(lib, rid):
    r = W.row_of(rid)
    d, rows = W.plan(lib, W.S3, r["K"], r["cap"])
    assert (d["tiles"], d["nslots"]) == (r["tiles"], r["slots"]), d
    assert {len(w) for w in W.static_walk(d)} == r["per_wg"]
    assert W.ranges_histogram(rows) == r["ranges"]
    assert d["nitems"] == sum(k * v for k, v in r["ranges"].items())
    pr = W.problem_ranges(rows, len(W.S3))
    assert all(rng[-1][1] == r["K"] // 32 for rng in pr)
    if "lengths" in r:
        assert all([b - a for a, b in rng] == r["lengths"] for rng in pr)
    # the launches that produce the partials: every distinct range as a depth of its own at SUB_CAP has one range per tile
    for n in {b - a for rng in pr for a, b in rng}:
        ds, rs = W.plan(lib, W.S3, 32 * n, W.SUB_CAP)
        assert W.ranges_histogram(rs) == {1: 11} and ds["nslots"] == 0


# ------------------------------------------------------------------------------------------ what is correct is inside every limit
@pytest.mark.parametrize("K", W.DEPTHS)
def test_p8_correct_walks_sit_inside_every_limit(lib, K):
    ops, refs = W.operands("P8", K), W.references("P8", K)
    stored = [(c0 + a.t() @ b).float().numpy() for a, b, c0, _ in ops]                  # the float64 reference as stored
    assert W.check_c(stored, refs, "P8 K=%d reference as stored" % K) <= 1.0
    base = None
    for cap in W.CAPS + (0,):
        d, rows = W.plan(lib, W.P8, K, cap)
        c = W.fake_c(ops, d, rows)
        assert W.check_c(c, refs, "P8 K=%d cap %d emulation" % (K, cap)) <= 1.0
        if W.ranges_histogram(rows) == {1: 34}:                                         # one addition per element: the same bits
            base = base or c
            assert all(W.first_difference(x, y) is None for x, y in zip(c, base))
        v = W.fake_bias(ops, d, rows, W.P8_BIAS)
        assert W.check_bias(v, refs, ops, W.P8_BIAS, "P8 K=%d cap %d emulation" % (K, cap)) <= 1.0


@pytest.mark.parametrize("rid", W.S3_ROW_IDS)
def test_s3_fold_of_correct_partials_sits_inside_every_limit(lib, rid):
    r = W.row_of(rid)
    for seed, scale in ((0, 1.0), (1, 4.0)):
        ops, refs = W.operands("S3", r["K"], seed, scale), W.references("S3", r["K"], seed, scale)
        d, rows = W.plan(lib, W.S3, r["K"], r["cap"])
        parts = W.host_partials(ops, W.problem_ranges(rows, 3))
        c = [W.fold(o[2], p) for o, p in zip(ops, parts)]
        assert W.check_c(c, refs, "S3 %s fold emulation" % rid) <= 1.0
        assert W.check_c(W.fake_c(ops, d, rows), refs, "S3 %s atomic emulation" % rid) <= 1.0
        assert W.check_bias(W.fake_bias(ops, d, rows, W.S3_BIAS), refs, ops, W.S3_BIAS, "S3 %s bias emulation" % rid) <= 1.0


# ------------------------------------------------------------------------------------------ the planted faults
@pytest.mark.parametrize("rid", [r["id"] for r in W.MULTI_ROWS])
def test_a_wrong_fold_lands_outside_its_check(lib, rid):
    r = W.row_of(rid)
    X, Y = W.operands("S3", r["K"], 0, 1.0), W.operands("S3", r["K"], 1, 4.0)
    refs = {0: W.references("S3", r["K"], 0, 1.0), 1: W.references("S3", r["K"], 1, 4.0)}
    _, rows = W.plan(lib, W.S3, r["K"], r["cap"])
    pr = W.problem_ranges(rows, 3)
    px, py = W.host_partials(X, pr), W.host_partials(Y, pr)
    multi = [i for i in range(3) if len(pr[i]) > 1]
    assert multi
    for i in multi:
        good = W.fold(X[i][2], px[i])
        for what, parts, ops, which in (
                ("range 0 in place of range 1", [px[i][0]] + [px[i][0]] + px[i][2:], X, 0),
                ("the last range twice", px[i] + [px[i][-1]], X, 0),
                ("the last range missing", px[i][:-1], X, 0),
                ("slot 0 stale: the other operand set's", [py[i][0]] + px[i][1:], X, 0),
                ("slot 1 stale in the larger launch", [py[i][0]] + [px[i][1]] + py[i][2:], Y, 1)):
            bad = [W.fold(o[2], p) for o, p in zip(ops, py if which else px)]
            bad[i] = W.fold(ops[i][2], parts)
            assert W.first_difference(bad[i], W.fold(ops[i][2], (py if which else px)[i])) is not None, what
            with pytest.raises(AssertionError, match="C of problem %d" % i):
                W.check_c(bad, refs[which], "S3 %s %s" % (rid, what))
        # the order: a fold of three or more slots taken from the end differs in some element (two summands commute)
        if len(pr[i]) >= 3:
            assert W.first_difference(W.fold(X[i][2], px[i][::-1]), good) is not None
            assert W.first_difference(W.fold(np.zeros_like(good), px[i]) + X[i][2].float().numpy(), good) is None    # (the same order)
            # c0 added first instead of last: another order too
            first = W.fold(np.zeros_like(good), [X[i][2].float().numpy()] + px[i])
            assert W.first_difference(first, good) is not None
    assert any(len(pr[i]) >= 3 for i in multi) or rid == "K96-cap16"


@pytest.mark.parametrize("bug", ["next_problem", "prev_problem", "every_tile_row"])
def test_column_sums_that_reach_the_wrong_vector_land_outside_their_check(lib, bug):
    ops, refs = W.operands("P8", 96), W.references("P8", 96)
    for cap in (W.CAPS if bug == "every_tile_row" else (8, 16)):       # (at 24 no summing item has another problem's beside it)
        d, rows = W.plan(lib, W.P8, 96, cap)
        with pytest.raises(AssertionError, match="bias of problem"):
            W.check_bias(W.fake_bias(ops, d, rows, W.P8_BIAS, bug=bug), refs, ops, W.P8_BIAS, "P8 cap %d %s" % (cap, bug))
    # a vector of a problem without a bias that was added to is rejected by name, whatever the amount
    v = W.fake_bias(ops, *W.plan(lib, W.P8, 96, 8), W.P8_BIAS)
    v[1] = v[1] + np.float32(1e-6)
    with pytest.raises(AssertionError, match="which has none, was written"):
        W.check_bias(v, refs, ops, W.P8_BIAS, "P8 touched")


def test_guards_of_the_next_items_problem_land_outside_the_check(lib):
    ops, refs = W.operands("P8", 64), W.references("P8", 64)
    for cap in (8, 16):
        d, rows = W.plan(lib, W.P8, 64, cap)
        with pytest.raises(AssertionError, match="C of problem"):
            W.check_c(W.fake_c(ops, d, rows, bug="mn_next"), refs, "P8 cap %d mn_next" % cap)


def test_the_staged_launch_is_what_the_plan_was_asked_about():
    """stage() on the host: strides 8 / 16 / 8 wider or the narrowest legal ones, NaN in the padding of A and B, start values in C
    and in every bias vector, and refill() puts another operand set into the same windows."""
    ops = W.operands("P8", 32)
    for padded in (True, False):
        st = W.stage(ops, 32, padded, W.P8_BIAS, device="cpu")
        for i, (m, n) in enumerate(W.P8):
            assert st.As[i].ld == W.ld_of(m, 8 if padded else 0) and st.Bs[i].ld == W.ld_of(n, 16 if padded else 0)
            assert st.As[i].ld % 8 == 0 and st.Bs[i].ld % 8 == 0 and st.Cs[i].ld == n + (8 if padded else 0)
            if st.As[i].ld > m:
                assert bool(st.As[i].t[:, m:].float().isnan().all())
            assert st.bs[i].kind == ("acc" if i in W.P8_BIAS else "in")
        assert st.As[6].ld > W.P8[6][0]                                  # M = 300: four padding columns on the narrowest stride
        ptrs = [s.ptr() for s in st.As + st.Bs + st.Cs + st.bs]
        W.refill(st, W.operands("P8", 32, 1, 4.0), operands_too=True)
        assert ptrs == [s.ptr() for s in st.As + st.Bs + st.Cs + st.bs]
        assert bool((st.Cs[0].host().double() == W.operands("P8", 32, 1, 4.0)[0][2]).all())
        st.ar.arm()
        st.ar.check()
