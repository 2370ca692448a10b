"""-m gpu: the persistent GEMM kernels with SEVERAL items per workgroup (gemm_bf16_256_kernel in every compile-time form, its run-time
epilogue and split-K items, the two deep-pipeline kernels), each element inside its own limit.

The one-shot cmp_gemm_grid_next(cap, rev) caps the grid, so that launches of 14 to 64 items run on 6 to 24 workgroups: some
workgroup runs three items, the workgroups differ in their item counts, `has_next` is true and false in one launch -- the code
between two items (the next item's first k-slab under this item's epilogue, the fold image behind the staging areas and its counted
wait, lstat / lrow reused, EpiPre operands, one column-sum atomic per item per wave, the ItemPuller's claims and steals, ep.rev) is
what these cases run.  Tables, inputs, references and limits: tests/gemm_items_bounds.py; that each check can fail:
tests/test_gemm_items_checks_host.py.

Every case runs inside the guard-banded arena, with every leading dimension 8 or 16 elements wider than the row and exact, under
COMPOSER_GEMM_ITEMS=static and =dynamic, Table A also walked from the end (rev), at the case's cap (where that is 8 also at 6, which
changes the tile row on most item transitions), at 24 and without a cap.  "Which
workgroup runs an item never changes a result" (gemm.hip): everything that is not a float atomic must be BITWISE the same across all
of these; column sums and split-K atomics are held to their bounds.  -s prints the worst error / limit per launch form.

Measured on an MI355X (2026-10-21), worst error / limit per form over all of the above (a bf16 output stands near 1 by construction:
round-to-nearest alone uses up to 2^-8 |ref|; the fp32 figures show what the arithmetic itself leaves):
    256 kernel  generic (fp32 out, ragged dropout) 0.993   plain 0.995   GELU + aux 0.994 / aux 0.995   residual 0.995
                GELU' 0.994, column sums 0.131   split-K atomics 0.020
                fold np 2 / 3: 0.991 / 0.989   fold GELU 0.983 / 0.988, aux 0.991 / 0.989   fold fp32 out 0.033 / 0.044
                statistics out: C 0.995, mean 0.137, M2 0.125   rebuild np 2 / 3: C 0.905 / 0.970, mean 0.125 / 0.139, M2 0.125
                scale residual 0.995   scale GELU' 0.993, column sums np 2 / 3: 0.033 / 0.020
    p4-256      plain, GELU + aux, residual 0.995   split-K (slabs / atomics) 0.020
    p4-128      plain, GELU + aux, residual 0.995   split-K (slabs / atomics) 0.019
Every bitwise comparison held; a test function takes 0.1 to 0.7 s.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_items_bounds as IB

pytestmark = pytest.mark.gpu


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


_BASE = {}         # (case id, padded) -> the outputs of the first launch of that case and stride regime (float32 holds a bf16 or fp32
                   # output exactly): the bitwise reference, dropped after the case's last item mode
WORST = {}         # launch form -> {output: worst error / limit}
REPEAT_CASE = "A-fold-np2"      # launched three times in a row under `dynamic`: both counter sets, and the first one again


def exact_outputs(case, padded):
    """The outputs that no float atomic touches."""
    if case["kind"] == "wgrad" and not (case["flags"] in (16, 48) and case["mode"] == "slab" and not padded):
        return ()                                   # split-K through f32 atomics (slabs: the deep pipeline with ldc == N only)
    return ("C", "aux", "part")


def form_of(case):
    fam, kind, lnm, n = case["want"]
    return "%s kind %d lnm %d np %d%s" % ({IB.TILE256: "256", IB.P4_256: "p4-256", IB.P4_128: "p4-128"}[fam], kind, lnm, n,
                                           " split-K" if case["splitk"] > 1 else "")


@pytest.mark.parametrize("mode", IB.ITEM_MODES)
@pytest.mark.parametrize("case", IB.CASES, ids=IB.CASE_IDS)
def test_gemm_items(lib, monkeypatch, case, mode):
    monkeypatch.setenv("COMPOSER_GEMM_ITEMS", mode)
    o = IB.operands(case)
    start = IB.colsum_start(case["N"]) if case["colsum"] else None
    figures = WORST.setdefault(form_of(case), {})
    try:
        for padded in (True, False):
            for rev in case["revs"]:
                for cap in (IB.caps_of(case) if rev == 0 else IB.caps_of(case)[:2 if case["cap"] == 8 else 1]):
                    what = "%s %s %s rev %d cap %d" % (case["id"], mode, "padded" if padded else "exact", rev, cap)
                    st = IB.stage(case, o, padded)
                    st.ar.arm()
                    IB.arm(lib, case, st, cap, rev)
                    ck(lib, lib.cmp_k_gemm(stream(), *st.args))
                    if case["id"] == REPEAT_CASE and mode == "dynamic" and cap == case["cap"]:
                        first = IB.outputs_of(case, st)
                        for _ in range(2):
                            IB.arm(lib, case, st, cap, rev)
                            ck(lib, lib.cmp_k_gemm(stream(), *st.args))
                            assert np.array_equal(IB.outputs_of(case, st)["C"], first["C"]), what + ": a repeated launch differs"
                    st.ar.check()
                    outs = IB.outputs_of(case, st)
                    exact = exact_outputs(case, padded)
                    base = _BASE.get((case["id"], padded))
                    same = base is not None and bool(exact)
                    if same:
                        for name in exact:
                            if name in outs:
                                diff = np.argwhere(outs[name].astype(np.float32) != base[name])
                                assert diff.size == 0, "%s: %s differs from the first launch of this case at %s (%d elements): %r against %r" % (
                                    what, name, tuple(diff[0]), len(diff), outs[name][tuple(diff[0])], base[name][tuple(diff[0])])
                    else:
                        _BASE.setdefault((case["id"], padded), {k: v.astype(np.float32) for k, v in outs.items() if k in exact})
                    if not same or case["colsum"]:
                        w = IB.check_outputs(case, o, outs, what, colsum_start=start, sums_only=same)
                        for k, v in w.items():
                            figures[k] = max(figures.get(k, 0.0), v)
    finally:
        if case["kind"] == "wgrad":
            ck(lib, lib.cmp_gemm_set_workspace(None, 0))
        if mode == IB.ITEM_MODES[-1]:
            for padded in (True, False):
                _BASE.pop((case["id"], padded), None)
    print(" GEMM_ITEMS %s %s | %s | worst error / limit so far: %s" % (case["id"], mode, form_of(case),
                                                                        " ".join("%s %.3f" % kv for kv in sorted(figures.items()))))


def test_the_grid_hook_is_one_shot_and_refuses_what_it_cannot_mean(lib):
    assert lib.cmp_gemm_grid_next(257, 0) != 0 and b"gemm_grid_next" in lib.cmp_last_error()
    assert lib.cmp_gemm_grid_next(-1, 0) != 0
    case = next(c for c in IB.CASES if c["id"] == "A-bias-K64")
    o = IB.operands(case)
    outs = []
    for armed in (True, False, False):
        st = IB.stage(case, o, False)
        st.ar.arm()
        if armed:
            ck(lib, lib.cmp_gemm_grid_next(3, 1))
        ck(lib, lib.cmp_k_gemm(stream(), *st.args))
        st.ar.check()
        outs.append(IB.outputs_of(case, st)["C"])
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], outs[2])
