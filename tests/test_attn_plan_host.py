"""CPU checks of the attention launcher's decision (composer_amd/csrc/attn_plan.h) through cmp_attn_plan: which kernel form, grids,
LDS bytes, block plan, bias sums fused or a pass, timing classes a cmp_k_attn_fwd / cmp_k_attn_bwd call gets -- for the case tables
of the GPU kernel tests (the form each row's comment names IS the form it reaches), for the model's own launches, for every refusal,
and as a sweep of internal invariants.  Nothing here touches a GPU: the device's answers (workgroups per CU, key-split opt-in) are
arguments, DEVICE_CAPS holds the MI355X's and tests/test_gpu_kernels.py::test_attention_caps_are_what_the_host_tables_assume checks
them on the device."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

import test_gpu_kernel_guards as G
import test_gpu_kernels as K
import test_gpu_ln_fused as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32, BF16 = 0, 1
FWD_KS, FWD_MASK, FWD_ROWS, BWD_LN, BWD_KS1, BWD_KS2, BWD_ROWS = range(7)          # CMP_ATTN_*
K_FWD, K_DQ, K_DQ_LN = range(3)                                                    # CMP_ATTN_K_*
INVALID = -1
# cmp_attn_caps on an MI355X: resident workgroups per CU of the (forward, dQ, rstd-scaled dQ) kernel per (dtype, head size) -- the slots
# of the block plan -- as tests/test_gpu_kernels.py::test_attention_caps_are_what_the_host_tables_assume reads them off the device.  dQ holds
# Occ<T, D>::MINW_Q waves per SIMD (bf16 up to 64 wide: 3), the narrow forward kernels fit a fourth; 64 KiB and more of LDS allow 2, then 1.
DEVICE_CAPS = {(BF16, 16): (4, 3, 3), (BF16, 32): (4, 3, 3), (BF16, 64): (3, 3, 3), (BF16, 128): (2, 2, 2),
               (FP32, 16): (4, 3, None), (FP32, 32): (4, 2, None), (FP32, 64): (2, 2, None), (FP32, 128): (1, 1, None)}


def device_ks_ok(dtype, D):
    return int(dtype == BF16 and D <= 32)          # the key-split set exists there and gets its LDS opt-in


@pytest.fixture(scope="module")
def lib():
    from composer_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def plan(lib, dtype, B, T, H, D, p=0.0, amask=0, bias=0, ln=0, backward=0, wgs=None, ks_ok=None):
    """cmp_attn_plan with the MI355X's caps unless given: the plan as a dict, or (status, message) of a refusal."""
    from composer_amd import _lib
    info = _lib.AttnPlanInfo()
    if wgs is None:
        wgs = DEVICE_CAPS.get((dtype, D), (0, 0, 0))[(K_DQ_LN if ln else K_DQ) if backward else K_FWD] or 0
    ks_ok = device_ks_ok(dtype, D) if ks_ok is None else ks_ok
    rc = lib.cmp_attn_plan(dtype, B, T, H, D, p, amask, bias, ln, backward, wgs, ks_ok, C.byref(info))
    if rc != 0:
        return rc, lib.cmp_last_error().decode()
    return {n: (list(v) if hasattr(v, "__len__") else v) for n, v in ((n, getattr(info, n)) for n, _ in info._fields_)}


def both(lib, dtype, B, T, H, D, p, **kw):
    return plan(lib, dtype, B, T, H, D, p, **kw), plan(lib, dtype, B, T, H, D, p, backward=1, **kw)


def key_split_expected(dtype, B, T, H, D):
    return dtype == BF16 and D <= 32 and T >= 64 and -(-T // 128) * B * H <= 128


# ------------------------------------------------------------------------------------------ (a) the case tables, asserted
def test_fwd_bwd_and_guarded_tables_reach_both_kernel_sets(lib):
    """test_attention_fwd_bwd / test_attention_guarded: ragged T below and above one block at every head size; the small bf16 rows
    with heads up to 32 wide run the key-split kernels (the guarded table's last row by its comment), the rest the 128-row ones."""
    rows = [(dt, *s) for dt in (FP32, BF16) for s in K.ATTN_FWD_BWD_SHAPES] + list(G.ATTN_GUARDED_CASES)
    forms = set()
    for (dtype, B, T, H, D), p in itertools.product(rows, sorted(set(K.ATTN_FWD_BWD_P + G.ATTN_GUARDED_P))):
        f, b = both(lib, dtype, B, T, H, D, p, bias=1)
        ks = key_split_expected(dtype, B, T, H, D)
        assert f["form"] == (FWD_KS if ks else FWD_ROWS) and b["form"] in ((BWD_KS1, BWD_KS2) if ks else (BWD_ROWS,)), (dtype, B, T, H, D, f, b)
        assert f["drop"] == b["drop"] == int(p > 0) and f["plan_u"] == b["plan_u"] == -1, (f, b)
        forms.update((f["form"], b["form"]))
    assert forms == {FWD_KS, FWD_ROWS, BWD_KS1, BWD_ROWS}
    dtype, B, T, H, D = G.ATTN_GUARDED_CASES[-1]                     # "the last one runs the key-split kernels"
    assert both(lib, dtype, B, T, H, D, 0.2, bias=1)[1]["form"] == BWD_KS1
    assert {key_split_expected(BF16, *s) for s in K.ATTN_FWD_BWD_SHAPES} == {True, False}


def test_full_length_rows_take_single_blocks_or_a_short_plan(lib):
    """test_attention_full_length_many_groups: 64 (batch, head) rows.  T = 1024: 256 pairs are fewer than 512, so the 2-D grid of
    single blocks, 8 per row; T = 2048: 512 pairs, less than one round of 96 slots per XCD: 6 of the 8 rows per XCD as single blocks.
    25 MB and more of gradient, but nothing armed."""
    B, H, D = K.ATTN_FULL_LENGTH_BHD
    for dtype, T, p in K.ATTN_FULL_LENGTH_CASES:
        f, b = both(lib, dtype, B, T, H, D, p)
        u, gx, gy = (-1, 8, 64) if T == 1024 else (6, 8 * (2 * 8 + 6 * 16), 1)
        assert (f["form"], b["form"], f["plan_u"], b["plan_u"]) == (FWD_ROWS, BWD_ROWS, u, u), (f, b)
        assert (f["grid_x"][0], f["grid_y"][0]) == (gx, gy) and (b["grid_x"], b["grid_y"]) == ([gx, T // 256 if u > 0 else 8], [gy, 64]), (f, b)
        assert f["optin"] == b["optin"] == int(dtype == FP32) and b["bias_fused"] == b["bias_pass"] == 0, (f, b)


def test_block_plan_rows_get_the_plans_their_comments_name(lib):
    """test_attention_block_plans: rows per XCD that run as single blocks.  With 3 (bf16) and 2 (fp32) workgroups per CU: 8, 12, 8, 4, 8 --
    the dQ launch of every row and the forward launch of all but the head-size-32 row, whose forward kernel fits 4 per CU and pairs all
    16 rows in one whole round of 128 slots."""
    cases = K.ATTN_BLOCK_PLAN_CASES
    assert [plan(lib, dt, B, T, H, D, p, backward=bw, wgs=3 if dt == BF16 else 2)["plan_u"] for bw in (0, 1) for dt, B, H, D, T, p in cases] == [8, 12, 8, 4, 8] * 2
    assert [DEVICE_CAPS[(c[0], c[3])][:2] for c in cases] == [(3, 3), (3, 3), (3, 3), (4, 3), (2, 2)]
    got = []
    for dtype, B, H, D, T, p in cases:
        f, b = both(lib, dtype, B, T, H, D, p)
        assert (f["form"], b["form"]) == (FWD_ROWS, BWD_ROWS), (f, b)
        nb, rows = -(-T // 128), B * H // 8
        pairs = (nb + 1) // 2
        for q in (f, b):
            u = q["plan_u"]
            assert (q["grid_x"][0], q["grid_y"][0]) == ((8 * ((rows - u) * pairs + u * nb), 1) if u > 0 else (pairs, B * H)), q
        assert (b["grid_x"][1], b["grid_y"][1]) == (pairs, B * H), b               # dK/dV keeps the paired 2-D grid
        got.append((rows, f["plan_u"], b["plan_u"]))
    # 24 of 32 rows paired, 8 single; 12 of 16 single; 8 of 40 unpaired; head size 32 (dQ only); fp32 on 64 slots per XCD
    assert got == [(32, 8, 8), (16, 12, 12), (40, 8, 8), (16, -1, 4), (40, 8, 8)]


def test_key_split_rows_reach_the_key_split_kernels(lib):
    """test_attention_key_split_kernels: every row runs the key-split forward; the backward in one launch while 2 ceil(T/32) B H <= 512
    workgroups are resident at once, in two launches from there on."""
    want = {(1, 16, 16, 1024): BWD_KS2, (1, 16, 16, 1000): BWD_KS2, (2, 4, 32, 600): BWD_KS1, (1, 2, 16, 96): BWD_KS1}
    assert {c[:4] for c in K.ATTN_KEY_SPLIT_CASES} == set(want)
    for B, H, D, T, p in K.ATTN_KEY_SPLIT_CASES:
        f, b = both(lib, BF16, B, T, H, D, p, bias=1)
        nq = -(-T // 32)
        assert f["form"] == FWD_KS and (f["grid_x"][0], f["grid_y"][0], f["smem"][0]) == (nq, B * H, 4 * 256 * 40 * 2), f
        assert b["form"] == want[(B, H, D, T)] and (b["bias_fused"], b["bias_pass"]) == (0, 1), b
        if b["form"] == BWD_KS1:
            assert 2 * nq * B * H <= 512 and (b["nlaunch"], b["grid_x"][0], b["cls"][0]) == (1, 2 * nq, 5), b
        else:
            assert 2 * nq * B * H > 512 and (b["nlaunch"], b["grid_x"], b["cls"]) == (2, [nq, nq], [4, 5]), b
            assert b["smem"] == [81920, 40960 + 3 * 256 * 4], b
    # without the opt-in, or with a mask term, the same launches stay on the 128-row kernels
    assert plan(lib, BF16, 1, 1024, 16, 16, ks_ok=0)["form"] == FWD_ROWS and plan(lib, BF16, 1, 1024, 16, 16, backward=1, ks_ok=0)["form"] == BWD_ROWS
    assert plan(lib, BF16, 1, 1024, 16, 16, amask=1)["form"] == FWD_MASK


def test_bias_rows_take_the_path_their_comments_name(lib):
    """test_attention_bias_gradient_paths: fused / fused / pass behind the key-split kernels / pass behind the 128-row kernels."""
    got = []
    for B, H, D, T, p, fused in K.ATTN_BIAS_PATH_CASES:
        b = plan(lib, BF16, B, T, H, D, p, bias=1, backward=1)
        assert (b["bias_fused"], b["bias_pass"]) == (int(fused), int(not fused)), b
        got.append(((B, H, D, T), b["form"]))
    assert got == [((8, 8, 64, 1024), BWD_ROWS), ((5, 12, 64, 2048), BWD_ROWS), ((1, 16, 16, 1024), BWD_KS2), ((8, 16, 16, 1024), BWD_ROWS)]
    # the bound itself (3072 bytes of bf16 gradient per token at E = 512): 5461 tokens are the last pass, 5462 are fused; fp32 never a pass
    assert 5461 * 3072 <= 16 << 20 < 5462 * 3072
    assert plan(lib, BF16, 1, 5461, 8, 64, bias=1, backward=1)["bias_pass"] == 1 and plan(lib, BF16, 1, 5462, 8, 64, bias=1, backward=1)["bias_fused"] == 1
    assert plan(lib, FP32, 1, 1024, 16, 16, bias=1, backward=1)["bias_fused"] == 1


def test_ln_rows_cases_get_the_rstd_form_with_fused_sums(lib):
    """test_attention_backward_scales_its_rows_by_the_layernorm_rstd: the rstd form at every head size, its bias sums in the kernels; the
    plain call of the same test (2.7 MB of gradient; 144 blocks at head size 32: past the key split) takes the 128-row kernels and a pass."""
    B, T = L.ATTN_LN_ROWS_BT
    for (D, H), p in itertools.product(L.ATTN_LN_ROWS_HEADS, L.ATTN_LN_ROWS_P):
        b = plan(lib, BF16, B, T, H, D, p, bias=1, ln=1, backward=1)
        assert (b["form"], b["bias_fused"], b["bias_pass"], b["nlaunch"], b["plan_u"]) == (BWD_LN, 1, 0, 2, -1), b
        assert b["optin"] == int(D == 128) and b["smem"][1] == b["smem"][0] + 1536, b
        plain = plan(lib, BF16, B, T, H, D, p, bias=1, backward=1)
        assert (plain["form"], plain["bias_pass"]) == (BWD_ROWS, 1), plain


def test_attention_bound_tables_reach_the_forms_their_comments_name(lib):
    """tests/test_gpu_attention_bounds.py: every row of its tables, at both dropout rates, with the bias gradient armed."""
    import test_gpu_attention_bounds as AB
    def forms(row, **kw):
        dtype, B, T, H, D, _ = row
        return [tuple(q["form"] for q in both(lib, dtype, B, T, H, D, p, bias=1, **kw)) for p in AB.P_DROP]
    # tile-edge lengths: bf16 at head size 16 is on the key-split set from T = 64 on, in ONE launch (at most 2 * 9 * 2 = 36 workgroups);
    # every other row, head size 64 and all of fp32, on the 128-row kernels
    seen = set()
    for row in AB.TILE_EDGE_CASES:
        dtype, B, T, H, D, _ = row
        want = (FWD_KS, BWD_KS1) if (dtype == BF16 and D == 16 and T >= 64) else (FWD_ROWS, BWD_ROWS)
        assert forms(row) == [want] * 2, row
        seen.add((dtype, D, want))
    assert seen == {(FP32, 16, (FWD_ROWS, BWD_ROWS)), (FP32, 64, (FWD_ROWS, BWD_ROWS)), (BF16, 64, (FWD_ROWS, BWD_ROWS)),
                    (BF16, 16, (FWD_ROWS, BWD_ROWS)), (BF16, 16, (FWD_KS, BWD_KS1))}
    assert {r[2] for r in AB.TILE_EDGE_CASES} == {1, 2} | {e + d for e in (32, 64, 128, 256) for d in (-1, 0, 1)}
    # T = 333 on the 128-row kernels: three query blocks; the narrow bf16 heads only because 3 * 48 blocks are past the key split
    for row in AB.ROWS_333_CASES:
        dtype, B, T, H, D, _ = row
        assert forms(row) == [(FWD_ROWS, BWD_ROWS)] * 2 and T == 333 and -(-T // 128) == 3, row
        if dtype == BF16 and D <= 32:
            assert 3 * B * H > 128, row
    assert {(r[0], r[4]) for r in AB.ROWS_333_CASES} == {(FP32, 64), (BF16, 64), (FP32, 128), (BF16, 128), (BF16, 16), (BF16, 32)}
    assert {r[0] for r in AB.ROWS_333_CASES if r[5] == 0} == {FP32, BF16}                     # one row per dtype with scale = 0
    # key split: the backward in one launch while 2 * 11 * B H <= 512, in two from there on
    for row in AB.KEY_SPLIT_ONE_CASES:
        assert forms(row) == [(FWD_KS, BWD_KS1)] * 2 and 2 * 11 * row[1] * row[3] <= 512, row
    for row in AB.KEY_SPLIT_TWO_CASES:
        assert forms(row) == [(FWD_KS, BWD_KS2)] * 2 and 3 * row[1] * row[3] <= 128 and 2 * 11 * row[1] * row[3] > 512, row
    assert {r[4] for r in AB.KEY_SPLIT_ONE_CASES} == {r[4] for r in AB.KEY_SPLIT_TWO_CASES} == {16, 32}
    # the rstd-scaled backward: a row of the rstd test's own table
    for row in AB.LN_ROWS_CASES:
        dtype, B, T, H, D, _ = row
        assert (B, T) == L.ATTN_LN_ROWS_BT and (D, H) in L.ATTN_LN_ROWS_HEADS and dtype == BF16
        assert [plan(lib, dtype, B, T, H, D, p, bias=1, ln=1, backward=1)["form"] for p in AB.P_DROP] == [BWD_LN] * 2, row


# ------------------------------------------------------------------------------------------ (b) the model's own launches
def test_model_launches(lib):
    # C2 (E = 512, 8 heads of 64, T = 1024) at B = 128: 1024 (batch, head) rows, 128 per XCD; 4 pairs each over 96 slots: 5 whole rounds
    # pair 120 rows, 8 run as single blocks; 805 MB of gradient: fused sums
    f, b = both(lib, BF16, 128, 1024, 8, 64, 0.1, bias=1)
    assert (f["form"], f["plan_u"], f["grid_x"][0], f["grid_y"][0], f["smem"][0], f["optin"], f["cls"][0]) == (FWD_ROWS, 8, 8 * (120 * 4 + 8 * 8), 1, 36864, 0, 3), f
    assert (b["form"], b["plan_u"], b["grid_x"], b["grid_y"], b["smem"], b["bias_fused"], b["bias_pass"], b["cls"]) == \
        (BWD_ROWS, 8, [4352, 4], [1, 1024], [36864, 38400], 1, 0, [4, 5]), b
    flops = 128 * 8 * 1024 * 1024 * 64
    assert f["work"][0] == 2 * flops and b["work"] == [3 * flops, 4 * flops], (f, b)
    assert f["bytes"][0] == 128 * 1024 * 8 * (4 * 64 * 2 + 4) and b["bytes"] == [128 * 1024 * 8 * (6 * 64 * 2 + 8)] * 2, (f, b)
    # ... on the fused block path the backward stores rstd-scaled rows: the same grids from the rstd kernels
    r = plan(lib, BF16, 128, 1024, 8, 64, 0.1, bias=1, ln=1, backward=1)
    assert (r["form"], r["plan_u"], r["grid_x"], r["bias_fused"]) == (BWD_LN, 8, [4352, 4], 1), r
    # C2 at B = 32: 32 rows per XCD, 24 paired, 8 single (the first row of ATTN_BLOCK_PLAN_CASES); 201 MB
    f, b = both(lib, BF16, 32, 1024, 8, 64, 0.1, bias=1)
    assert (f["plan_u"], b["plan_u"], f["grid_x"][0], b["bias_fused"]) == (8, 8, 8 * (24 * 4 + 8 * 8), 1), (f, b)
    # C4 (E = 768, 12 heads of 64, T = 2048, B = 32): 48 rows per XCD, 8 pairs each: 4 whole rounds pair all 48
    f, b = both(lib, BF16, 32, 2048, 12, 64, 0.1, bias=1)
    assert (f["form"], f["plan_u"], f["grid_x"][0], f["grid_y"][0], b["plan_u"], b["bias_fused"]) == (FWD_ROWS, -1, 8, 384, -1, 1), (f, b)
    # the reference's default configuration at batch 1 (16 heads of 16, T = 1024): 128 blocks of the 128-row kind -> key split, the
    # backward in two launches (1024 workgroups on 512 slots), the bias sums a pass
    f, b = both(lib, BF16, 1, 1024, 16, 16, 0.1, bias=1)
    assert (f["form"], f["grid_x"][0], f["grid_y"][0], f["optin"]) == (FWD_KS, 32, 16, 1), f
    assert (b["form"], b["nlaunch"], b["bias_fused"], b["bias_pass"], b["plan_u"]) == (BWD_KS2, 2, 0, 1, -1), b
    # ... at batch 2 the split already loses
    assert both(lib, BF16, 2, 1024, 16, 16, 0.1, bias=1)[1]["form"] == BWD_ROWS
    # ... with rstd rows: no key split, fused sums
    r = plan(lib, BF16, 1, 1024, 16, 16, 0.1, bias=1, ln=1, backward=1)
    assert (r["form"], r["bias_fused"], r["bias_pass"], r["grid_x"], r["grid_y"]) == (BWD_LN, 1, 0, [8, 8], [16, 16]), r
    # a masked forward (Transformer.call(attention_mask=...)): never the key split, not timed
    f = plan(lib, BF16, 1, 1024, 16, 16, 0.0, amask=1)
    assert (f["form"], f["cls"][0], f["work"][0], f["bytes"][0], f["grid_x"][0], f["grid_y"][0]) == (FWD_MASK, -1, 0.0, 0.0, 8, 16), f
    # deterministic mode arms no bias pointer: neither fused nor a pass (model.hip runs its own fixed-order pass)
    b = plan(lib, BF16, 1, 1024, 16, 16, 0.1, backward=1)
    assert (b["bias_fused"], b["bias_pass"]) == (0, 0), b


# ------------------------------------------------------------------------------------------ (c) refusals
def test_every_refusal_is_reached_with_its_message(lib):
    for D in (0, 8, 24, 48, 96, 256):
        for backward in (0, 1):
            r = plan(lib, BF16, 2, 64, 2, D, backward=backward)
            assert r == (INVALID, "attention: head size %d unsupported (16/32/64/128)" % D), r
    r = plan(lib, FP32, 2, 64, 2, 64, ln=1, backward=1)
    assert r == (INVALID, "attention backward: LayerNorm row scaling exists in bf16 only"), r
    assert plan(lib, FP32, 2, 64, 2, 48, ln=1, backward=1)[1].startswith("attention: head size 48")          # the head size first
    assert isinstance(plan(lib, FP32, 2, 64, 2, 64, ln=1), dict)                                             # a forward has no such rows
    # nothing to launch comes before every refusal
    for args in ((BF16, 0, 64, 2, 48), (BF16, 2, 0, 2, 48), (FP32, 0, 64, 2, 64)):
        assert plan(lib, *args, ln=1, backward=1)["empty"] == 1


# ------------------------------------------------------------------------------------------ (d) consistency sweep
@pytest.mark.parametrize("backward", [0, 1])
def test_plan_invariants_sweep(lib, backward):
    """dtype x head size x B x H x T (ragged and tiny too) x p x mask / bias / rstd rows x caps 0-4 x key-split opt-in: whatever is
    planned is launchable and consistent with itself."""
    Bs, Hs, Ts = (1, 3, 8, 40, 128), (1, 4, 8, 12, 16), (1, 33, 63, 64, 129, 600, 1000, 1024, 2048)
    planned = 0
    for dtype, D, B, H, T, p, opt, wgs, ks_ok in itertools.product((FP32, BF16), (16, 32, 64, 128), Bs, Hs, Ts, (0.0, 0.1), range(4), range(5), (0, 1)):
        amask, bias, ln = (opt & 1, 0, 0) if not backward else (0, opt & 1, opt >> 1)
        if ln and dtype == FP32:
            continue                                  # refused by rule: test_every_refusal_is_reached_with_its_message
        q = plan(lib, dtype, B, T, H, D, p, amask=amask, bias=bias, ln=ln, backward=backward, wgs=wgs, ks_ok=ks_ok)
        what = (dtype, D, B, H, T, p, amask, bias, ln, wgs, ks_ok, q)
        assert isinstance(q, dict) and not q["empty"], what
        planned += 1
        ks = q["form"] in (FWD_KS, BWD_KS1, BWD_KS2)
        assert q["form"] in ((BWD_LN, BWD_KS1, BWD_KS2, BWD_ROWS) if backward else (FWD_KS, FWD_MASK, FWD_ROWS)), what      # exactly one form
        assert (q["form"] == BWD_LN) == bool(ln) and (q["form"] == FWD_MASK) == bool(amask), what
        assert q["nlaunch"] == (2 if q["form"] in (BWD_LN, BWD_KS2, BWD_ROWS) else 1) and q["block"] == 256 and q["drop"] == int(p > 0), what
        for i in range(q["nlaunch"]):
            assert q["grid_x"][i] > 0 and q["grid_y"][i] > 0 and 0 < q["smem"][i] <= 160 << 10, what
            assert q["cls"][i] == (-1 if amask else (3 if not backward else (5 if q["form"] == BWD_KS1 else 4 + i))), what
        assert q["optin"] == int(max(q["smem"][:q["nlaunch"]]) > 64 << 10), what
        assert q["bias_fused"] + q["bias_pass"] == bias, what
        if ks:
            assert dtype == BF16 and D <= 32 and T >= 64 and ks_ok and not amask and not ln and q["plan_u"] == -1 and q["bias_fused"] == 0, what
        nb, rows = -(-T // 128), B * H // 8
        pairs, u = (nb + 1) // 2, q["plan_u"]
        if u >= 0:
            assert wgs >= 1 and B * H % 8 == 0 and 0 < u < rows and (q["grid_x"][0], q["grid_y"][0]) == (8 * ((rows - u) * pairs + u * nb), 1), what
        elif not ks:
            assert q["grid_y"][0] == B * H and q["grid_x"][0] in (nb, pairs), what
        if wgs < 1:
            assert u == -1, what
    assert planned == (2 * 4 * 5 * 5 * 9 * 2 * 4 * 5 * 2) * (3 if backward else 4) // 4


def test_attn_plan_header_stands_alone_under_host_sanitizers(tmp_path):
    """attn_plan.h compiles with the host compiler, no HIP include path, and the sweep runs clean under ASan + UBSan: the header is
    HIP-free and the flop, byte and grid products do not overflow at B = 512, T = 4096, H = 16, D = 128."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = "clang++"
    exe = str(tmp_path / "attn_plan_sweep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "attn_plan_sweep.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "attn_plan sweep ok" in r.stdout and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
    hdr = open(os.path.join(ROOT, "composer_amd", "csrc", "attn_plan.h")).read()
    code = "\n".join(l.split("//")[0] for l in hdr.split("\n"))
    for banned in ("hip/", "hipcc", "getenv", "std::string", "std::vector", "std::map", "malloc", "new "):
        assert banned not in code, banned
