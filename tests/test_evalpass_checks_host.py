"""No GPU: the assertions tests/test_gpu_evalpass_kernel.py makes about cmp_k_eval_rows (tests/evalpass_checks.py), run on NumPy fakes
of the kernel -- a correct one, summing in the kernel's order (rows dealt to 4 x blocks waves, waves folded per block, blocks folded
in 16 stripes), passes; one that breaks ties at the maximum towards the HIGHER index fails the `correct` assertion, and one that drops
the last row fails the `count` and the `nll` assertions."""
import numpy as np
import pytest

import evalpass_checks as EC

V = EC.V_DEFAULT


def fake_eval_rows(z, y, ranges, logp, bug=None):
    rows = len(y)
    if bug == "drop_last_row":
        rows -= 1
    cls = EC.class_of(y, ranges, V)
    if bug == "ties_to_higher_index":
        valid = (y >= 0) & (y < V)
        ok = valid & ((V - 1 - np.argmax(z[:, ::-1], -1)) == np.where(valid, y, 0))       # the LAST maximum wins
    else:
        ok = EC.rank0(z, y, V)
    blocks = min(-(-rows // 4), 1024)
    part = np.zeros((blocks, 4, EC.SLOTS)), np.zeros((blocks, 4, EC.SLOTS), np.int64), np.zeros((blocks, 4, EC.SLOTS), np.int64)
    for r in range(rows):                                   # wave (b, w) walks rows 4 b + w, + 4 blocks, ... in ascending order
        if cls[r] < 0:
            continue
        b, w = (r % (4 * blocks)) // 4, r % 4
        part[0][b, w, cls[r]] += -np.float64(logp[r])
        part[1][b, w, cls[r]] += 1
        part[2][b, w, cls[r]] += int(ok[r])
    out = []
    for p in part:
        per_block = np.zeros((blocks, EC.SLOTS), p.dtype)
        for w in range(4):
            per_block += p[:, w]
        stripes = np.zeros((16, EC.SLOTS), p.dtype)
        for b in range(blocks):
            stripes[b % 16] += per_block[b]
        tot = np.zeros(EC.SLOTS, p.dtype)
        for j in range(16):
            tot += stripes[j]
        out.append(tot)
    return tuple(out)


def run(rows, n, bug=None):
    z, y = EC.make_case(rows)
    logp = EC.logp_fp32(z, y, V)
    ranges = EC.CLASS_SETS[n]
    EC.check_table(fake_eval_rows(z, y, ranges, logp, bug), EC.expected_table(z, y, ranges, logp, V), n, "rows %d n %d" % (rows, n))


@pytest.mark.parametrize("rows", [1, 63, 257, 1024 + 5])
@pytest.mark.parametrize("n", [0, 6, 8])
def test_correct_fake_passes(rows, n):
    run(rows, n)


def test_case_holds_what_the_kernel_test_needs():
    z, y = EC.make_case(257)
    ok = EC.rank0(z, y, V)
    assert not ok[EC.R_TIE_HI] and not ok[EC.R_TIE_HI2] and ok[EC.R_TIE_LO] and not ok[EC.R_NEG] and not ok[EC.R_V]
    assert np.isinf(z[EC.R_INF]).sum() == 1 and np.isfinite(EC.logp_fp32(z, y, V)).all()
    assert 0.3 < ok.mean() < 0.7                                                   # `correct` is exercised
    for n, ranges in EC.CLASS_SETS.items():
        cls = EC.class_of(y, ranges, V)
        assert (cls == -1).sum() == 2 and set(cls[cls >= 0]) <= set(range(n + 1))
        _, count, _ = EC.expected_table(z, y, ranges, EC.logp_fp32(z, y, V), V)
        assert count.sum() == 255 and not count[n + 1:].any()
    assert EC.expected_table(z, y, EC.CLASS_SETS[6], EC.logp_fp32(z, y, V), V)[1][5] == 0      # a class with no row
    assert EC.expected_table(z, y, EC.CLASS_SETS[8], EC.logp_fp32(z, y, V), V)[1][8] > 0       # ids outside every class


@pytest.mark.parametrize("n", [0, 6, 8])
def test_ties_to_the_higher_index_fail_the_correct_assertion(n):
    with pytest.raises(AssertionError, match="correct"):
        run(257, n, "ties_to_higher_index")


@pytest.mark.parametrize("rows", [63, 1024 + 5])
def test_a_dropped_last_row_fails_count_and_nll(rows):
    with pytest.raises(AssertionError, match="count"):
        run(rows, 6, "drop_last_row")
    # ... and with the count forced right, the nll assertion alone catches it
    z, y = EC.make_case(rows)
    logp = EC.logp_fp32(z, y, V)
    want = EC.expected_table(z, y, EC.CLASS_SETS[6], logp, V)
    got = fake_eval_rows(z, y, EC.CLASS_SETS[6], logp, "drop_last_row")
    with pytest.raises(AssertionError, match="nll"):
        EC.check_table((got[0], want[1], want[2]), want, 6)
