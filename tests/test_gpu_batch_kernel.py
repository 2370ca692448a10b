"""-m gpu: cmp_k_batch_rows (composer_amd/csrc/batch.hip) against the host restatement composer_amd.augment.build_batch, bit for bit,
on the guard-banded arena of tests/kernel_arena.py.

The id stream ends flush against a guard band (0xFF bytes: an over-read shows as the id 65535, which no layout holds), the outputs
are pre-filled with 0xFF; after the launch the guards, the stream and the plan must be bitwise unchanged and every element of x, y and
the status written.  Integers only: no tolerance anywhere.

Shapes (tests/batch_cases.py): W in {1, 7, 126, 127, 128, 1024} -- spans of 4, 16, 254, 256, 258 and 2050 tokens: under one wave,
exactly one 256-token chunk, one chunk plus two tokens, many chunks -- and B in {1, 5}, on streams built so that runs straddle tokens
63 / 64 and 255 / 256, one run is longer than a chunk, spans start and end inside runs, are all shifts or hold none, the last legal
offset occurs, pitches 0 and 127 are transposed by +-12, and f takes 512, 1000, 1024, 1100 and 1536; a second layout
(velocity_bins = 4, max_time_steps = 50) runs three of the cases."""
import ctypes as C

import numpy as np
import pytest
import torch

import batch_cases as bc
from composer_amd import augment
from kernel_arena import Arena

pytestmark = pytest.mark.gpu

CASES = [(name, W, B) for name in ("default", "small") for W, B, _ in bc.cases(name)]


@pytest.fixture(scope="module")
def lib():
    from composer_amd import _lib
    l = _lib.load()
    _lib.require_gpu()
    return l


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_refs = {}


def reference(name, W, B):
    """(ids, layout, plan, x, y, status) of a case, the host restatement computed once."""
    key = (name, W, B)
    if key not in _refs:
        ids, g = bc.stream(name)
        plan = bc.plan_for(W, B)
        _refs[key] = (ids, g, plan) + augment.build_batch(ids, g, plan, W)
    return _refs[key]


def launch(lib, ids, g, plan, W, expect_rc=0):
    B = len(plan)
    ar = Arena(nbytes=1 << 20)
    s_ids = ar.vector(torch.from_numpy(ids.astype(np.int16)), torch.int16, name="ids")       # (ids < 32768: the same 16 bits)
    s_plan = ar.vector(torch.from_numpy(plan.view(np.int32).copy()), torch.int32, name="plan")
    s_x = ar.output(torch.int32, B, W, W, name="x")
    s_y = ar.output(torch.int32, B, W, W, name="y")
    s_st = ar.output(torch.int32, B, 2, 2, name="status")
    ar.arm()
    layout = g.to_c() if g is not None else None
    rc = lib.cmp_k_batch_rows(stream(), C.c_void_p(s_ids.ptr()), len(ids), C.byref(layout) if layout is not None else None,
                              C.c_void_p(s_plan.ptr()), B, W, C.c_void_p(s_x.ptr()), C.c_void_p(s_y.ptr()), C.c_void_p(s_st.ptr()))
    assert rc == expect_rc, lib.cmp_last_error().decode()
    return ar, s_x, s_y, s_st


def test_the_cases_cover_what_they_were_built_for():
    """A condition on the inputs, checked on the host restatement: at least one row that grew, one that shrank, a vanished run, a
    fallback row, and every shape feature the streams were built for."""
    missing = set(bc.ALL_FEATURES) - bc.covered()
    assert not missing, missing


@pytest.mark.parametrize("name,W,B", CASES)
def test_batch_rows_equal_the_host_restatement(lib, name, W, B):
    ids, g, plan, x, y, st = reference(name, W, B)
    ar, s_x, s_y, s_st = launch(lib, ids, g, plan, W)
    ar.check()               # guards, stream and plan bitwise unchanged; every element of x, y, status written
    got_x, got_y, got_st = s_x.host().numpy(), s_y.host().numpy(), s_st.host().numpy()
    assert np.array_equal(got_st, st), (got_st.tolist(), st.tolist())
    assert np.array_equal(got_x, x), np.argwhere(got_x != x)[:4].tolist()
    assert np.array_equal(got_y, y), np.argwhere(got_y != y)[:4].tolist()


def test_identity_plans_need_no_layout(lib):
    ids, g = bc.stream("default")
    W = 127
    plan = augment.as_plan([(0, 0, 1024), (290, 0, 1024), (len(ids) - (W + 1), 0, 1024)])
    x, y, st = augment.build_batch(ids, None, plan, W)
    ar, s_x, s_y, s_st = launch(lib, ids, None, plan, W)
    ar.check()
    assert np.array_equal(s_x.host().numpy(), x) and np.array_equal(s_y.host().numpy(), y) and np.array_equal(s_st.host().numpy(), st)
    assert np.array_equal(x[1], ids[290:290 + W])


def test_bare_launch_refusals(lib):
    ids, g = bc.stream("default")
    plan = augment.as_plan([(0, 0, 1024)])
    launch(lib, ids[:8], g, plan, 8, expect_rc=-1)                       # n < W + 1
    bad = bc.layout("default")
    bad.time_shift_n = 0
    launch(lib, ids, bad, plan, 8, expect_rc=-1)                         # a bad layout, under the grammar's rules
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    P = C.c_void_p(z.data_ptr())
    assert lib.cmp_k_batch_rows(stream(), P, 64, None, P, 1, 0, P, P, P) == -1        # W = 0
    assert lib.cmp_k_batch_rows(stream(), None, 64, None, P, 1, 4, P, P, P) == -1
    assert lib.cmp_k_batch_rows(stream(), P, 64, None, P, 0, 4, P, P, P) == 0         # no rows: nothing to do


def test_a_bad_row_of_a_device_plan_reads_and_writes_nothing(lib):
    """The bare launch cannot see a device plan on the host: a row the host entry points refuse gets (0, CMP_BATCH_REFUSED), its x
    and y stay untouched, the stream is not read for it, and the other rows are built as usual."""
    ids, g = bc.stream("default")
    W, n = 16, len(ids)
    plan = augment.as_plan([(40, 3, 1100), (n - W, 0, 1024), (-1, 0, 1024), (0, 0, 1600), (0, 0, 511), (0, 200, 1024), (3600, -2, 700)])
    good = [0, 6]
    x, y, st = augment.build_batch(ids, g, plan[good], W)
    B = len(plan)
    ar = Arena(nbytes=1 << 20)
    s_ids = ar.vector(torch.from_numpy(ids.astype(np.int16)), torch.int16, name="ids")
    s_plan = ar.vector(torch.from_numpy(plan.view(np.int32).copy()), torch.int32, name="plan")
    fill = torch.full((B, W), -7, dtype=torch.int32)
    s_x = ar.accumulator(fill, torch.int32, B, W, W, name="x")
    s_y = ar.accumulator(fill, torch.int32, B, W, W, name="y")
    s_st = ar.output(torch.int32, B, 2, 2, name="status")
    ar.arm()
    layout = g.to_c()
    rc = lib.cmp_k_batch_rows(stream(), C.c_void_p(s_ids.ptr()), n, C.byref(layout), C.c_void_p(s_plan.ptr()), B, W,
                              C.c_void_p(s_x.ptr()), C.c_void_p(s_y.ptr()), C.c_void_p(s_st.ptr()))
    assert rc == 0, lib.cmp_last_error().decode()
    ar.check()
    got_x, got_y, got_st = s_x.host().numpy(), s_y.host().numpy(), s_st.host().numpy()
    assert np.array_equal(got_x[good], x) and np.array_equal(got_y[good], y) and np.array_equal(got_st[good], st)
    rest = [b for b in range(B) if b not in good]
    assert (got_x[rest] == -7).all() and (got_y[rest] == -7).all()
    assert got_st[rest].tolist() == [[0, 2]] * len(rest)
