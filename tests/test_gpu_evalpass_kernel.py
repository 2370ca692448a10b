"""-m gpu: cmp_k_eval_rows (composer_amd/csrc/evalpass.hip) alone, on the guard-banded arena of tests/kernel_arena.py: logits with NaN
in-row padding, the table and the workspace flush against guard bands.  Inputs, restatement and bounds: tests/evalpass_checks.py
(tests/test_evalpass_checks_host.py shows on wrong fakes that its `correct` and `nll` assertions can fail).

Shapes: rows 1, 63, 257, 1029 (one wave, one partial block, many blocks, more blocks than the fold has stripes) x V = 390 with ldz 390
(4-byte loads), 392 and 512 (16-byte loads), each with 0, 6 and 8 classes; and V = 513, ldz 576: the two-pass form of wide rows.

The table is an accumulator: the test starts its integer fields at a non-zero value per slot (count 1000 + slot, correct 100 + slot) and
nll at 0, so a slot the launch did not add into, or added into twice, shows; a second launch into the same table adds exactly the same
again; two launches into fresh tables give bitwise equal nll.  nll[c] is held to the float64 sum of the fp32 -logp values that
cmp_k_score_rows returns for the same logits, within count[c] * 2^-52 relative."""
import ctypes as C

import numpy as np
import pytest
import torch

import evalpass_checks as EC
from kernel_arena import Arena

pytestmark = pytest.mark.gpu

SHAPES = [(rows, 390, ldz) for rows in (1, 63, 257, 1024 + 5) for ldz in (390, 392, 512)] + [(63, 513, 576)]


@pytest.fixture(scope="module")
def lib():
    from composer_amd import _lib
    l = _lib.load()
    _lib.require_gpu()
    return l


def ck(lib, rc):
    assert rc == 0, lib.cmp_last_error().decode()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def classes_of(ranges):
    from composer_amd import _lib
    k = _lib.EvalClasses()
    k.n = len(ranges)
    for i, (lo, hi) in enumerate(ranges):
        k.lo[i], k.hi[i] = lo, hi
    return k


def table_init():
    t = np.zeros(27, np.int64)
    t[9:18] = 1000 + np.arange(9)
    t[18:27] = 100 + np.arange(9)
    return t


def split(words):
    """(nll float64 [9], count [9], correct [9]) of the table's 27 words, the integer fields without their start values."""
    w = np.asarray(words, np.int64)
    init = table_init()
    return w[:9].copy().view(np.float64), w[9:18] - init[9:18], w[18:27] - init[18:27]


def launch(lib, rows, V, ldz, ranges, launches=1):
    z, y = EC.make_case(rows, V)
    ar = Arena(nbytes=(rows * ldz * 4 + (512 << 10) + 255) // 256 * 256)
    zs = ar.operand(torch.from_numpy(z), torch.float32, rows, V, ldz, name="logits")
    ys = ar.vector(torch.from_numpy(y), torch.int32, name="y")
    lp = ar.output(torch.float32, 1, rows, rows, name="logp")
    tb = ar.vector(torch.from_numpy(table_init()), torch.int64, name="table", kind="acc")
    ws = ar.scratch(int(lib.cmp_k_eval_rows_ws(rows)), name="partial tables")
    P = lambda s: C.c_void_p(s.ptr())
    k = classes_of(ranges or [])
    ar.arm()
    ck(lib, lib.cmp_k_score_rows(stream(), P(zs), ldz, P(ys), P(lp), None, None, rows, V))
    tables = []
    for _ in range(launches):
        ck(lib, lib.cmp_k_eval_rows(stream(), P(zs), ldz, P(ys), rows, V, C.byref(k) if ranges is not None else None, P(tb), P(ws)))
        torch.cuda.synchronize()
        tables.append(split(tb.vec.cpu().numpy()))
    ar.check()           # guards, in-row padding and inputs bitwise unchanged; the logp window written and finite
    return z, y, lp.vec.cpu().numpy(), tables


@pytest.mark.parametrize("rows,V,ldz", SHAPES)
def test_eval_rows_against_the_restatement(lib, rows, V, ldz):
    for n, ranges in EC.CLASS_SETS.items():
        z, y, logp, (once, twice) = launch(lib, rows, V, ldz, ranges, launches=2)
        want = EC.expected_table(z, y, ranges, logp, V)
        EC.check_table(once, want, n, "rows %d V %d ldz %d n %d" % (rows, V, ldz, n))
        # a second launch into the same table: the integer fields exactly doubled, nll the first sum added to itself
        assert (twice[1] == 2 * once[1]).all() and (twice[2] == 2 * once[2]).all()
        assert (twice[0] == 2 * once[0]).all()
        # two fresh launches: the same bits
        again = launch(lib, rows, V, ldz, ranges)[3][0]
        assert once[0].tobytes() == again[0].tobytes() and (once[1] == again[1]).all() and (once[2] == again[2]).all()
        if rows >= 8:
            assert want[1].sum() == rows - 2                      # the targets -1 and V are counted nowhere
            assert 0.3 * rows < want[2].sum() < 0.7 * rows


def test_null_classes_mean_one_slot(lib):
    z, y, logp, (got,) = launch(lib, 257, 390, 392, None)
    EC.check_table(got, EC.expected_table(z, y, [], logp, 390), 0, "null classes")


def test_eval_rows_refuses_bad_arguments(lib):
    from composer_amd import _lib
    z = torch.zeros(4, 16, device="cuda"); y = torch.zeros(4, device="cuda", dtype=torch.int32)
    t = torch.zeros(27, device="cuda", dtype=torch.int64); w = torch.zeros(int(lib.cmp_k_eval_rows_ws(4)), device="cuda", dtype=torch.uint8)
    P = lambda a: C.c_void_p(a.data_ptr())
    call = lambda k, V=16, rows=4, zz=z: lib.cmp_k_eval_rows(stream(), P(zz) if zz is not None else None, 16, P(y), rows, V,
                                                            C.byref(k) if k is not None else None, P(t), P(w))
    assert call(None, V=17) == -1 and call(None, V=0) == -1 and call(None, zz=None) == -1
    for ranges, word in (([(0, 17)], "outside"), ([(-1, 4)], "outside"), ([(3, 3)], "empty"), ([(0, 8), (7, 12)], "overlaps")):
        assert call(classes_of(ranges)) == -1 and word in _lib.last_error(), ranges
    k = classes_of([])
    k.n = 9
    assert call(k) == -1 and "at most 8" in _lib.last_error()
    assert call(None, rows=0) == 0                                 # no rows: nothing to do
    torch.cuda.synchronize()
    assert not t.any()
