"""CPU checks of the grouped weight-gradient launch's plan (composer_amd/csrc/wgrad_plan.h) through cmp_wgrad_group_plan: the
decision and the item table for the benchmark's block shapes, every refusal, and the property the bias sums that ride on the launch
rest on -- every (tile, K range) once, and the items of a problem's first tile row cover every (column tile, k-step) of its B operand
exactly once.  Nothing here touches a GPU: pointers are made-up addresses."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x7f0000001000          # any 16-byte-aligned value: never dereferenced
FITS, R_NPROB, R_K, R_WGS, R_SLAB, R_SHAPE, R_LD, R_ALIGN, R_SPAN, R_TABLE = range(10)
SLAB, FORCE = 1, 2


@pytest.fixture(scope="module")
def lib():
    from composer_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def plan(lib, shapes, K, max_wgs=0, flags=0, lda=None, ldb=None, A=None, B=None, items=True):
    """shapes: [(M, N)].  Returns (info dict, item rows [nitems, 8] = problem, m0, n0, kt0, kt1, idx, ranges, tile)."""
    from composer_amd import _lib
    n = len(shapes)
    ip, vp = C.c_int * max(n, 1), C.c_void_p * max(n, 1)
    lda = lda or [m for m, _ in shapes]
    ldb = ldb or [nn for _, nn in shapes]
    info = _lib.WgradPlanInfo()
    cap = 4096
    rows = np.zeros((cap, 8), np.int32)
    rc = lib.cmp_wgrad_group_plan(n, vp(*(A or [PTR] * n)), ip(*lda), vp(*(B or [PTR] * n)), ip(*ldb), ip(*[m for m, _ in shapes]),
                                  ip(*[nn for _, nn in shapes]), K, max_wgs, flags, C.byref(info),
                                  rows.ctypes.data_as(C.c_void_p) if items else None, cap)
    assert rc == 0, lib.cmp_last_error().decode()
    d = {k: getattr(info, k) for k, _ in info._fields_}
    assert d["nitems"] <= cap
    return d, rows[:d["nitems"]] if d["fits"] else rows[:0]


def block(E):
    """The four problems of a decoder block: dWpr, dWfc, dWproj, dWattn."""
    return [(4 * E, E), (E, 4 * E), (E, E), (E, 3 * E)]


def check_cover(shapes, d, rows):
    """Every (tile, k-step) once; tile row 0 of every problem covers every (column tile, k-step) of B once."""
    nk = d["nk"]
    cover = {}
    for p, m0, n0, k0, k1, idx, ranges, tile in rows.tolist():
        assert 0 <= k0 < k1 <= nk and m0 % 256 == 0 and n0 % 256 == 0 and m0 < shapes[p][0] and n0 < shapes[p][1]
        c = cover.setdefault((p, m0, n0), np.zeros(nk, np.int32))
        c[k0:k1] += 1
        assert 0 <= idx < ranges <= d["max_split"]
    tiles = {(p, tm * 256, tn * 256) for p, (M, N) in enumerate(shapes) for tm in range(-(-M // 256)) for tn in range(-(-N // 256))}
    assert set(cover) == tiles and len(tiles) == d["tiles"]
    assert all((c == 1).all() for c in cover.values())
    for p, (M, N) in enumerate(shapes):
        row0 = [c for (q, m0, n0), c in cover.items() if q == p and m0 == 0]
        assert len(row0) == -(-N // 256) and all((c == 1).all() for c in row0)


def test_benchmark_block_shapes(lib):
    """C2 (E = 512, 131 072 tokens): 48 tiles x 5 K ranges, the 16 spare workgroups as a sixth range of dWproj (4 tiles) and dWattn
    (12 tiles): 256 items, one per workgroup; 18 of the 48 tiles are in tile row 0.  The same cut at B = 32;
    C4 (E = 768, 65 536 tokens): 108 tiles x 2, a third range for dWproj (9) and dWattn (27)."""
    for tokens in (131072, 32768):
        d, rows = plan(lib, block(512), tokens)
        assert d["fits"] and d["taken"] and d["refusal"] == FITS
        assert (d["tiles"], d["nitems"], d["grid"], d["wgs"], d["nk"]) == (48, 48 * 5 + 16, 256, 256, tokens // 32)
        per_prob = [sorted({r[6] for r in rows.tolist() if r[0] == p}) for p in range(4)]
        assert per_prob == [[5], [5], [6], [6]]
        assert d["max_split"] == 6 and d["longest"] == -(-d["nk"] // 5)
        assert len({(r[0], r[1], r[2]) for r in rows.tolist() if r[1] == 0}) == 18
        check_cover(block(512), d, rows)
    d, rows = plan(lib, block(768), 65536)
    assert d["fits"] and d["taken"] and (d["tiles"], d["nitems"], d["grid"]) == (108, 108 * 2 + 36, 252)
    assert [sorted({r[6] for r in rows.tolist() if r[0] == p}) for p in range(4)] == [[2], [2], [3], [3]]
    check_cover(block(768), d, rows)


def test_cost_model_declines_a_lone_problem_without_force(lib):
    """One problem alone is what a split-K launch already is: the cost model keeps it (grouped >= separate), force takes it."""
    d, _ = plan(lib, [(512, 512)], 131072)
    assert d["fits"] and not d["taken"]
    d, rows = plan(lib, [(512, 512)], 131072, flags=FORCE)
    assert d["fits"] and d["taken"]
    check_cover([(512, 512)], d, rows)


def test_refusals(lib):
    ok = block(64)
    assert plan(lib, ok, 96)[0]["fits"]
    cases = [
        (dict(shapes=[], K=96), R_NPROB),
        (dict(shapes=[(64, 64)] * 9, K=96), R_NPROB),                      # nprob > 8
        (dict(shapes=ok, K=48), R_K),                                      # K % 32
        (dict(shapes=ok, K=16), R_K),
        (dict(shapes=ok, K=96, max_wgs=7), R_WGS),
        (dict(shapes=ok, K=96, flags=SLAB), R_SLAB),                       # slab workspace
        (dict(shapes=[(0, 64)], K=96), R_SHAPE),
        (dict(shapes=[(64, 65536 - 256)], K=96), R_SHAPE),
        (dict(shapes=[(64, 64)], K=96, lda=[68]), R_LD),
        (dict(shapes=[(64, 64)], K=96, ldb=[68]), R_LD),
        (dict(shapes=[(64, 64)], K=96, A=[PTR + 8]), R_ALIGN),             # alignment
        (dict(shapes=[(64, 64)], K=96, B=[PTR + 2]), R_ALIGN),
        (dict(shapes=[(64, 64)], K=131072, lda=[8192]), R_SPAN),           # 2 GiB operand
    ]
    for kw, want in cases:
        d, rows = plan(lib, **kw)
        assert (d["fits"], d["taken"], d["refusal"]) == (0, 0, want), (kw, d)
        assert len(rows) == 0
    # a refused list stays refused under force
    assert plan(lib, ok, 48, flags=FORCE)[0]["refusal"] == R_K


@pytest.mark.parametrize("K", [32, 96, 1024, 32768])
@pytest.mark.parametrize("max_wgs", [0, 8, 104, 208])
def test_consistency_sweep(lib, K, max_wgs):
    """Every (tile, K range) exactly once and tile row 0 covering B exactly once, over ragged problem lists (those of
    tests/test_gpu_wgrad_group_bias.py among them), workgroup caps (a data-parallel job's) and depths."""
    rng = np.random.default_rng(K + max_wgs)
    lists = [[(264, 520), (8, 8), (1000, 136)], block(64), block(320), block(512)]
    dims = [8, 64, 136, 256, 264, 520, 1000, 1536, 2048]
    lists += [[(int(rng.choice(dims)), int(rng.choice(dims))) for _ in range(int(rng.integers(1, 9)))] for _ in range(12)]
    for shapes in lists:
        d, rows = plan(lib, shapes, K, max_wgs=max_wgs, flags=FORCE)
        assert d["fits"] and d["taken"] and d["grid"] == min(d["nitems"], d["wgs"]) and d["wgs"] == (min(max_wgs, 256) if max_wgs else 256) // 8 * 8
        check_cover(shapes, d, rows)
        assert d["longest"] == max(r[4] - r[3] for r in rows.tolist())


def test_wgrad_plan_header_stands_alone_under_host_sanitizers(tmp_path):
    """wgrad_plan.h compiles with the host compiler, no HIP include path, and the native sweep (tests/wgrad_plan_sweep.cpp: the same
    cover properties over 1 684 lists up to K = 131 072) runs clean under ASan + UBSan; the header is HIP-free and reads no
    environment variable."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = "clang++"
    exe = str(tmp_path / "wgrad_plan_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "wgrad_plan_sweep.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "wgrad_plan sweep ok" in r.stdout and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
    hdr = open(os.path.join(ROOT, "composer_amd", "csrc", "wgrad_plan.h")).read()
    code = "\n".join(l.split("//")[0] for l in hdr.split("\n"))
    for banned in ("hip/", "hipcc", "getenv", "malloc"):
        assert banned not in code, banned
