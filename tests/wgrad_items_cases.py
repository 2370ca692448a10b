"""Case tables, operands, references and the fold emulation of tests/test_gpu_wgrad_items.py (the grouped weight-gradient launch --
gemm.hip: gemm_wgrad_group_kernel / gemm_wgrad_group_la_kernel -- with SEVERAL items per workgroup, and its last-arriver form held to
its stated summation order); tests/test_wgrad_items_host.py asserts on the CPU, from cmp_wgrad_group_plan, what every row below says it
reaches, and that each check can fail.  Nothing here needs a device: `stage(..., device="cpu")` carves the same arena on the host.

wgrad_plan.h cuts every tile into s <= G / T K ranges (T: 256 x 256 output tiles of all problems, G: workgroups), so a workgroup runs
several items only when T > G: the one-shot cmp_gemm_grid_next(cap, 0) in front of cmp_k_wgrad_group_bias makes G = cap, as a
data-parallel job's cmp_dp_set_gemm_cus does for the model.  P8 has 34 tiles; a workgroup then walks items of DIFFERENT problems back
to back (item_coords switches A / B / C / M / N / the leading dimensions / cur_bias, both buffer descriptors are rebuilt, the next
item's stages are issued under this item's epilogue, and Ccur / Mcur / Ncur / meta keep this item's values across the switch).

    list, depth, cap                      tiles  items per workgroup  K ranges per tile
    P8, K in DEPTHS, cap 8                34     4 or 5               1       >= 5 consecutive item pairs of different problems
    P8, K in DEPTHS, cap 16               34     2 or 3               1       >= 5 such pairs
    P8, K in DEPTHS, cap 24               34     1 or 2               1       has_next true and false in one launch
    S3, K = 1024, no cap                  11     1                    5       7, 7, 7, 7, 4 k-steps; 55 slots
    S3, K = 256, cap 24                   11     1                    10 tiles x 2, 1 tile x 3; 23 slots
    S3, K = 96, cap 16                    11     1                    6 tiles x 1, 5 tiles x 2: slot and no-slot tiles; 10 slots
    S3, K = 96, cap 8                     11     1 or 2               1       no slot: the last-arriver launch gets a null workspace

The depths are 1, 2, 3, 4 and 5 k-steps against the three stages the kernel issues ahead of an item (the next item's prologue is
`if (kt0 + i < kt1) issue(...)`, its first wait `wait_younger(min(n, AHEAD) - 1)`)."""
import ctypes as C
import functools

import numpy as np
import torch

import kernel_arena as KA
from kernel_arena import Arena

F32, BF = torch.float32, torch.bfloat16
FORCE = 2                       # cmp_wgrad_group_plan flags: take the launch whatever the cost model says (as the entry point does)

P8 = [(264, 520), (8, 8), (1000, 136), (520, 776), (136, 264), (8, 520), (300, 8), (264, 264)]
S3 = [(264, 520), (8, 8), (1000, 136)]
LISTS = {"P8": P8, "S3": S3}
P8_BIAS = (0, 2, 4)             # the problems of P8 that get a bias vector; the other five have none.  At cap 8 one workgroup runs
                                # problems 0, 1, 2 in a row (with, without, with) and another goes from a summing item of 4 to 5
S3_BIAS = (0, 2)                # as tests/test_gpu_wgrad_group_bias.py: the middle problem has none
DEPTHS = (32, 64, 96, 128, 160)
CAPS = (8, 16, 24)
ITEM_MODES = ("static", "dynamic")
SUB_CAP = 8                     # the single-range launches that produce the partials of a K range
MIN_CROSS = 5                   # consecutive item pairs of one workgroup that belong to different problems (caps 8 and 16)

P8_ROWS = {8: dict(tiles=34, per_wg={4, 5}), 16: dict(tiles=34, per_wg={2, 3}), 24: dict(tiles=34, per_wg={1, 2})}
# ranges: {K ranges of a tile: tiles that have so many}
S3_ROWS = [
    dict(id="K1024-nocap", K=1024, cap=0, tiles=11, per_wg={1}, ranges={5: 11}, slots=55, lengths=[7, 7, 7, 7, 4]),
    dict(id="K256-cap24", K=256, cap=24, tiles=11, per_wg={1}, ranges={2: 10, 3: 1}, slots=23),
    dict(id="K96-cap16", K=96, cap=16, tiles=11, per_wg={1}, ranges={1: 6, 2: 5}, slots=10),
    dict(id="K96-cap8", K=96, cap=8, tiles=11, per_wg={1, 2}, ranges={1: 11}, slots=0),
]
S3_ROW_IDS = [r["id"] for r in S3_ROWS]
MULTI_ROWS = [r for r in S3_ROWS if r["slots"] > 0]


def ld_of(width, pad):
    """A leading dimension of A or B: the row, `pad` elements wider, rounded up to the multiple of 8 the launch requires (exact for
    every width here but the 300 of P8's seventh problem, whose narrowest legal stride is 304: four NaN columns)."""
    return -(-(width + pad) // 8) * 8


def row_of(rid):
    return next(r for r in S3_ROWS if r["id"] == rid)


# ------------------------------------------------------------------------------------------ the plan
def plan(lib, shapes, K, max_wgs=0, flags=FORCE):
    """cmp_wgrad_group_plan of [(M, N)] on exact strides -> (info dict, rows [nitems, 8] = problem, m0, n0, kt0, kt1, index of the
    K range among the tile's, K ranges of the tile, tile) in item-table order."""
    from composer_amd import _lib
    n = len(shapes)
    ip = C.c_int * n
    info = _lib.WgradPlanInfo()
    cap = 4096
    rows = np.zeros((cap, 8), np.int32)
    Ms, Ns = ip(*[m for m, _ in shapes]), ip(*[nn for _, nn in shapes])
    lda, ldb = ip(*[ld_of(m, 0) for m, _ in shapes]), ip(*[ld_of(nn, 0) for _, nn in shapes])
    rc = lib.cmp_wgrad_group_plan(n, None, lda, None, ldb, Ms, Ns, K, max_wgs, flags, C.byref(info), rows.ctypes.data_as(C.c_void_p), cap)
    assert rc == 0, lib.cmp_last_error().decode()
    d = {k: getattr(info, k) for k, _ in info._fields_}
    assert d["fits"] and d["taken"] and d["nitems"] <= cap, d
    return d, rows[:d["nitems"]]


def static_walk(d):
    """Item-table positions per workgroup under static striding: blockIdx.x, + gridDim.x, ..."""
    return [list(range(w, d["nitems"], d["grid"])) for w in range(d["grid"])]


def cross_pairs(d, rows):
    """Consecutive items of one workgroup that belong to different problems."""
    return sum(int(rows[a, 0] != rows[b, 0]) for w in static_walk(d) for a, b in zip(w[:-1], w[1:]))


def bias_switches(d, rows, bias_on):
    """(after, before): items that sum B's columns (tile row 0 of a problem with a bias) directly followed / preceded, in their
    workgroup, by an item of another problem -- where a cur_bias switched too early or too late would show."""
    after = before = 0
    for w in static_walk(d):
        for j, pos in enumerate(w):
            if int(rows[pos, 0]) in bias_on and int(rows[pos, 1]) == 0:
                after += int(j + 1 < len(w) and rows[w[j + 1], 0] != rows[pos, 0])
                before += int(j > 0 and rows[w[j - 1], 0] != rows[pos, 0])
    return after, before


def with_without_with(d, rows, bias_on):
    """Some workgroup runs a problem with a bias, then one without, then one with again."""
    for w in static_walk(d):
        seq = [int(rows[p, 0]) in bias_on for p in w]
        if any(a and not b and c for a, b, c in zip(seq[:-2], seq[1:-1], seq[2:])):
            return True
    return False


def ranges_histogram(rows):
    per_tile = {}
    for r in rows.tolist():
        per_tile[r[7]] = r[6]
    h = {}
    for v in per_tile.values():
        h[v] = h.get(v, 0) + 1
    return h


def problem_ranges(rows, nprob):
    """Per problem the K ranges [(kt0, kt1)] in the order of their index; every tile of a problem has the same ones (asserted)."""
    out = []
    for p in range(nprob):
        tiles = {}
        for q, m0, n0, k0, k1, idx, ranges, tile in rows.tolist():
            if q == p:
                tiles.setdefault(tile, {})[idx] = (k0, k1)
                assert 0 <= idx < ranges
        per = [[t[i] for i in range(len(t))] for t in tiles.values()]
        assert per and all(x == per[0] for x in per), (p, per)
        assert per[0][0][0] == 0 and all(a[1] == b[0] for a, b in zip(per[0][:-1], per[0][1:])), per[0]
        out.append(per[0])
    return out


# ------------------------------------------------------------------------------------------ operands and references
@functools.lru_cache(maxsize=None)
def operands(name, K, seed=0, scale=1.0):
    """Per problem (a [K, M], b [K, N] as rounded to bf16, c0 [M, N], b0 [N]) in float64; c0 and b0 are float32 values.  Draws of
    different seeds are independent; `scale` multiplies A and B (C0, the bias start and the products by its square / by it)."""
    g = torch.Generator().manual_seed(7919 * seed + K + 7)
    out = []
    for m, n in LISTS[name]:
        a = (torch.randn(K, m, generator=g) * scale).to(BF).double()
        b = (torch.randn(K, n, generator=g) * scale).to(BF).double()
        c0 = (torch.randn(m, n, generator=g) * scale * scale).double()
        b0 = ((torch.randn(n, generator=g) * 3.0 + 1.0) * scale).double()
        out.append((a, b, c0, b0))
    return out


@functools.lru_cache(maxsize=None)
def references(name, K, seed=0, scale=1.0):
    """Per problem ((ref of C, S, factor), (ref of the bias vector, S, factor)): kernel_arena's bounds, computed once and shared."""
    out = []
    for a, b, c0, b0 in operands(name, K, seed, scale):
        ref, S, f = KA.gemm_bound(a.t().contiguous(), b, c0.abs())
        out.append(((ref + c0, S, f), KA.colsum_bound(b, b0)))
    return out


def sub_operands(ops, kt0, kt1):
    """Rows 32 kt0 .. 32 kt1 of every A and B as operands of their own, C zero: the partial of one K range."""
    return [(a[32 * kt0:32 * kt1].contiguous(), b[32 * kt0:32 * kt1].contiguous(), torch.zeros_like(c0), b0) for a, b, c0, b0 in ops]


# ------------------------------------------------------------------------------------------ staging
class Staged:
    pass


def arena_bytes(shapes, K, padded):
    pa, pb, pc = (8, 16, 8) if padded else (0, 0, 0)
    n = 0
    for m, nn in shapes:
        for b in (K * ld_of(m, pa) * 2, K * ld_of(nn, pb) * 2, m * (nn + pc) * 4, nn * 4):
            n += b + KA.GUARD + 2 * KA.ALIGN
    return n + 2 * KA.GUARD


def stage(ops, K, padded, bias_on=(), device="cuda"):
    """One guard-banded arena with every operand of the launch: lda / ldb / ldc 8 / 16 / 8 elements wider than the row (NaN in the
    padding columns of A and B) or exact; C and the bias vectors of `bias_on` are accumulators with non-zero start values, the
    vectors of the other problems inputs (check() requires them bitwise unchanged)."""
    shapes = [(a.shape[1], b.shape[1]) for a, b, _, _ in ops]
    st = Staged()
    st.ar = ar = Arena(device, arena_bytes(shapes, K, padded))
    st.shapes, st.K, st.bias_on = shapes, K, tuple(bias_on)
    st.As, st.Bs, st.Cs, st.bs = [], [], [], []
    for i, (a, b, c0, b0) in enumerate(ops):
        m, n = shapes[i]
        st.As.append(ar.operand(a, BF, K, m, ld_of(m, 8 if padded else 0), name="A%d" % i))
        st.Bs.append(ar.operand(b, BF, K, n, ld_of(n, 16 if padded else 0), name="B%d" % i))
        st.Cs.append(ar.accumulator(c0, F32, m, n, n + (8 if padded else 0), name="C%d" % i))
        st.bs.append(ar.vector(b0.float(), F32, name="bias%d" % i, kind="acc" if i in st.bias_on else "in"))
    nn = len(shapes)
    vp, ip = C.c_void_p * nn, C.c_int * nn
    st.args = (nn, vp(*[s.ptr() for s in st.As]), ip(*[s.ld for s in st.As]), vp(*[s.ptr() for s in st.Bs]), ip(*[s.ld for s in st.Bs]),
               vp(*[s.ptr() for s in st.Cs]), ip(*[s.ld for s in st.Cs]), ip(*[m for m, _ in shapes]), ip(*[n for _, n in shapes]), K)
    st.bias_arg = vp(*[s.ptr() if i in st.bias_on else None for i, s in enumerate(st.bs)])
    return st


def refill(st, ops, operands_too=False):
    """The start values back into C and the bias vectors (and, for another operand set of the same shapes, A and B): the windows,
    and with them every pointer of the launch, stay where they are -- the launcher's item table and slots are reused."""
    for i, (a, b, c0, b0) in enumerate(ops):
        if operands_too:
            st.As[i].logical.copy_(a.to(BF))
            st.Bs[i].logical.copy_(b.to(BF))
        st.Cs[i].logical.copy_(c0.to(F32))
        st.bs[i].logical.copy_(b0.to(F32).reshape(1, -1))


def launch(lib, st, stream, cap=0, bias=True):
    """cmp_gemm_grid_next(cap, 0) where a cap is asked for, then the grouped launch; returns its status."""
    if cap:
        rc = lib.cmp_gemm_grid_next(cap, 0)
        assert rc == 0, lib.cmp_last_error().decode()
    return lib.cmp_k_wgrad_group_bias(stream, *st.args, st.bias_arg if bias and st.bias_on else None)


def c_of(st):
    return [c.host().numpy() for c in st.Cs]


def bias_of(st):
    return [v.host().reshape(-1).numpy() for v in st.bs]


# ------------------------------------------------------------------------------------------ the checks
def check_c(got, refs, what):
    """Every element of every problem's C inside kernel_arena's limit; -> worst error / limit."""
    return max(KA.assert_within(torch.from_numpy(np.asarray(c, np.float64)), ref, f * S, False, "%s: C of problem %d" % (what, i))
               for i, (c, ((ref, S, f), _)) in enumerate(zip(got, refs)))


def check_bias(got, refs, ops, bias_on, what):
    """The vectors of `bias_on` inside colsum_bound of their start value plus the column sums of B as stored; every other vector
    bitwise its start value.  -> worst error / limit."""
    worst = 0.0
    for i, (v, (_, (ref, S, f))) in enumerate(zip(got, refs)):
        if i in bias_on:
            worst = max(worst, KA.assert_within(torch.from_numpy(np.asarray(v, np.float64)), ref, f * S, False, "%s: bias of problem %d" % (what, i)))
        else:
            assert np.array_equal(np.asarray(v, np.float32), ops[i][3].float().numpy()), "%s: bias of problem %d, which has none, was written" % (what, i)
    return worst


def first_difference(a, b):
    """None where a and b are equal as float32 values, else a text that names the first element that differs."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    diff = np.argwhere(a != b)
    if diff.size == 0:
        return None
    at = tuple(int(x) for x in diff[0])
    return "element %s: %r against %r (%d of %d elements differ)" % (at, float(a[at]), float(b[at]), len(diff), a.size)


def fold(c0, partials):
    """The last arriver's order in float32 (gemm.hip, the WGLA epilogue): the slots of a tile summed from zero in the order of their
    K ranges, then ONE addition onto C:  fl(c0 + fl(.. fl(fl(0 + p_0) + p_1) .. + p_last))."""
    s = np.zeros_like(np.asarray(partials[0], np.float32))
    for p in partials:
        s = (s + np.asarray(p, np.float32)).astype(np.float32)
    return (np.asarray(c0, np.float32) + s).astype(np.float32)


def host_partials(ops, ranges):
    """What a perfect kernel stores for each K range: the float64 product of the range's rows, rounded to float32 once."""
    return [[(a[32 * k0:32 * k1].t() @ b[32 * k0:32 * k1]).float().numpy() for k0, k1 in ranges[i]] for i, (a, b, _, _) in enumerate(ops)]


def fake_c(ops, d, rows, bug=None):
    """Every problem's C after a launch whose workgroups walk their items in the kernel's static order, in numpy: an item adds the
    float32 image of its K range's float64 product onto its tile, inside the problem's M and N.  bug: `mn_next` -- Mcur / Ncur not
    kept across item_coords(): the row and column guards are the NEXT item's problem's (clipped to the array here: only a smaller
    problem shows)."""
    shapes = [(a.shape[1], b.shape[1]) for a, b, _, _ in ops]
    out = [c0.float().numpy().copy() for _, _, c0, _ in ops]
    for w in static_walk(d):
        for j, pos in enumerate(w):
            p, m0, n0, k0, k1 = (int(x) for x in rows[pos, :5])
            M, N = shapes[p]
            if bug == "mn_next" and j + 1 < len(w):
                M, N = (min(x, y) for x, y in zip(shapes[p], shapes[int(rows[w[j + 1], 0])]))
            r1, c1 = min(m0 + 256, M), min(n0 + 256, N)
            if r1 > m0 and c1 > n0:
                a, b = ops[p][0], ops[p][1]
                part = (a[32 * k0:32 * k1, m0:r1].t() @ b[32 * k0:32 * k1, n0:c1]).float().numpy()
                out[p][m0:r1, n0:c1] = (out[p][m0:r1, n0:c1] + part).astype(np.float32)
    return out


def fake_bias(ops, d, rows, bias_on, bug=None):
    """The bias vectors after a launch whose workgroups walk their items in the kernel's static order, in numpy: an item of tile
    row 0 of a problem with a bias adds the float32 column sums of its rows of B to that problem's vector.  bug: `next_problem` --
    cur_bias read after item_coords() moved on: the sums go to the vector of the NEXT item's problem; `prev_problem` -- cur_bias
    not switched: to the PREVIOUS item's; `every_tile_row` -- the m0 == 0 condition dropped."""
    vec = [b0.float().numpy().copy() for _, _, _, b0 in ops]
    for w in static_walk(d):
        for j, pos in enumerate(w):
            p, m0, n0, k0, k1 = (int(x) for x in rows[pos, :5])
            if p not in bias_on or (m0 != 0 and bug != "every_tile_row"):
                continue
            b = ops[p][1]
            sums = b[32 * k0:32 * k1, n0:n0 + 256].sum(0).float().numpy()
            target = p
            if bug == "next_problem" and j + 1 < len(w):
                target = int(rows[w[j + 1], 0])
            if bug == "prev_problem" and j > 0:
                target = int(rows[w[j - 1], 0])
            if target not in bias_on:
                continue                                    # (a null pointer: nothing is added)
            hi = min(n0 + len(sums), len(vec[target]))
            if hi > n0:
                vec[target][n0:hi] = (vec[target][n0:hi] + sums[:hi - n0]).astype(np.float32)
    return vec
