"""-m gpu: truncated sampling (top-k, nucleus / top-p) drawn on the device, against its host specification
`composer_amd.transformer.sampling_keep_set` (include/composer_hip.h, "truncated sampling").

The device draw must equal, bit for bit, the plain sampler (cmp_k_sample) on a copy of the logits row with every dropped column
set to -inf: at kernel level over 10 000 draw counters, and in both decode chains at every step, where the row is read back with
cmp_decode_logits_get / cmp_decode_batch_logits_get (tests/test_gpu_decode_logits.py ties those rows to the float64 oracle).  The
distribution of the draws is checked by chi-square against the renormalised truncated softmax.

A top-p case whose float64 cumulative mass lies within DELTA = 1e-9 of top_p is undecidable between two summation orders: the
chain tests skip such a step, count it, and fail above 1 % skipped; the kernel-level rows keep a margin of 1e-6 and skip nothing.
"""
import ctypes as C

import numpy as np
import pytest
import yaml
from click.testing import CliRunner

from test_sampling_truncation import DELTA, KERNEL_MARGIN, TEMPERATURES, brute_keep_set, kernel_rows, kp_cases, round3_row

pytestmark = pytest.mark.gpu

V0 = 390
MODES = ("literal", "kv", "kv-slide")
# per-row (temperature, top_k, top_p) of the batched chain, cycled over the rows
ROW_PARAMS = [(1.0, 0, 1.0), (0.7, 40, 1.0), (1.6, 0, 0.9), (1.0, 40, 0.9), (0.7, 0, 0.5), (0.0, 40, 0.9), (1.3, 5, 0.95)]


def chi_square_p(counts, probs, min_expected=8.0):
    """Pearson chi-square of observed counts against expected probabilities; cells with a small expectation are pooled
    (smallest first) until every cell expects >= min_expected draws.  Returns (p-value, degrees of freedom).
    (tests/test_gpu_round3.py: chi_square_p)"""
    from scipy import stats
    n = counts.sum()
    exp = probs * n
    order = np.argsort(exp)
    e_cells, o_cells = [], []
    acc_e = acc_o = 0.0
    for i in order:
        acc_e += exp[i]; acc_o += counts[i]
        if acc_e >= min_expected:
            e_cells.append(acc_e); o_cells.append(acc_o)
            acc_e = acc_o = 0.0
    if acc_e > 0:                      # leftover joins the last cell
        e_cells[-1] += acc_e; o_cells[-1] += acc_o
    e, o = np.array(e_cells), np.array(o_cells)
    stat = ((o - e) ** 2 / e).sum()
    dof = len(e) - 1
    return float(stats.chi2.sf(stat, dof)), dof


def keep_and_margin(z, temperature, top_k, top_p):
    """(sampling_keep_set, distance of the nearest cumulative mass from top_p relative to the total; inf when top_p is off or
    the draw is greedy)"""
    from composer_amd.transformer import sampling_keep_set
    keep = sampling_keep_set(z, temperature, top_k, top_p)
    margin = np.inf
    if temperature > 0 and np.float32(top_p) < 1:
        V = len(z)
        order = np.lexsort((np.arange(V), -z.astype(np.float64)))
        if 0 < top_k < V:
            order = order[:top_k]
        z64 = z[order].astype(np.float64)
        cum = np.cumsum(np.exp((z64 - z64[0]) / np.float64(np.float32(temperature))))
        margin = float(np.abs(cum / cum[-1] - np.float64(np.float32(top_p))).min())
    return keep, margin


def masked(z, keep):
    out = np.full(len(z), -np.inf, np.float32)
    out[keep] = z[keep]
    return out


def truncated_probs(z, temperature, keep):
    p = np.zeros(len(z))
    zz = z[keep].astype(np.float64) / temperature
    p[keep] = np.exp(zz - zz.max())
    return p / p.sum()


def gpu():
    import torch
    from composer_amd import _lib
    lib = _lib.load(); _lib.require_gpu()
    return torch, _lib, lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)


def k_sample(lib, _lib, stream, zd, V, temperature, seed, ctr0, n, out):
    _lib.check(lib.cmp_k_sample(stream, C.c_void_p(zd.data_ptr()), V, temperature, seed, ctr0, n, C.c_void_p(out.data_ptr())))


def k_sample_ex(lib, _lib, stream, zd, V, temperature, k, p, seed, ctr0, n, out):
    _lib.check(lib.cmp_k_sample_ex(stream, C.c_void_p(zd.data_ptr()), V, temperature, k, p, seed, ctr0, n, C.c_void_p(out.data_ptr())))


# ---------------------------------------------------------------- 1. kernel level, bitwise
@pytest.mark.parametrize("name", [n for n, _ in kernel_rows()])
def test_k_sample_ex_equals_k_sample_on_the_masked_row(name):
    torch, _lib, lib, stream = gpu()
    z = dict(kernel_rows())[name]
    V, n, seed = len(z), 10_000, 123
    zd = torch.from_numpy(z).cuda()
    got = torch.empty(n, dtype=torch.int32, device="cuda")
    want = torch.empty(n, dtype=torch.int32, device="cuda")
    for t in TEMPERATURES:
        for k, p in kp_cases(V):
            keep, margin = keep_and_margin(z, t, k, p)
            assert margin >= KERNEL_MARGIN, (name, t, k, p, margin)          # never skipped: the row is away from the boundary
            assert keep.tolist() == brute_keep_set(z, t, k, p)[0]
            md = torch.from_numpy(masked(z, keep)).cuda()
            k_sample_ex(lib, _lib, stream, zd, V, t, k, p, seed, 7, n, got)
            k_sample(lib, _lib, stream, md, V, t, seed, 7, n, want)
            torch.cuda.synchronize()
            g, w = got.cpu().numpy(), want.cpu().numpy()
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, (name, t, k, p, len(keep), bad[:5], g[bad[:5]], w[bad[:5]])
            assert np.isin(g, keep).all()
            if (k, p) in ((0, 1.0), (V, 1.0)):                                # filters off: the plain sampler on the row itself
                k_sample(lib, _lib, stream, zd, V, t, seed, 7, n, want)
                torch.cuda.synchronize()
                assert np.array_equal(g, want.cpu().numpy()), (name, t, k, p)
            if k == 1:
                assert (g == keep[0]).all()


def test_k_sample_ex_greedy_ignores_the_filters_and_bad_arguments_are_refused():
    torch, _lib, lib, stream = gpu()
    z = round3_row(V0)
    z[[40, 41, 300]] = z.max() + 1.0                         # a three-way tie at the top: the lowest index
    zd = torch.from_numpy(z).cuda()
    got = torch.empty(8, dtype=torch.int32, device="cuda")
    for k, p in ((0, 1.0), (40, 0.9), (1, 0.5)):
        k_sample_ex(lib, _lib, stream, zd, V0, 0.0, k, p, 9, 0, 8, got)
        torch.cuda.synchronize()
        assert got.cpu().tolist() == [40] * 8
    for k, p in ((-1, 1.0), (0, 0.0), (0, 1.5), (0, float("nan")), (0, -0.1)):
        assert lib.cmp_k_sample_ex(stream, C.c_void_p(zd.data_ptr()), V0, 1.0, k, p, 9, 0, 8, C.c_void_p(got.data_ptr())) == -1
        assert "top_" in _lib.last_error()
    # the truncating sampler's row limit is named, and only asked for when a filter is on
    wide = torch.zeros(5000, dtype=torch.float32, device="cuda")
    assert lib.cmp_k_sample_ex(stream, C.c_void_p(wide.data_ptr()), 5000, 1.0, 40, 1.0, 9, 0, 8, C.c_void_p(got.data_ptr())) == -1
    assert "4096" in _lib.last_error()
    for t, k, p in ((1.0, 0, 1.0), (1.0, 5000, 1.0), (0.0, 40, 0.9)):
        _lib.check(lib.cmp_k_sample_ex(stream, C.c_void_p(wide.data_ptr()), 5000, t, k, p, 9, 0, 8, C.c_void_p(got.data_ptr())))
    torch.cuda.synchronize()


def test_k_sample_ex_at_the_row_limit():
    """V = 4096, sixteen columns per thread, the largest LDS image"""
    torch, _lib, lib, stream = gpu()
    V, n = 4096, 2000
    z = np.random.default_rng(4096).standard_normal(V).astype(np.float32) * 2.0
    z[[100, 4000, 2048]] = 1.0                               # an exact tie
    zd = torch.from_numpy(z).cuda()
    got = torch.empty(n, dtype=torch.int32, device="cuda")
    want = torch.empty(n, dtype=torch.int32, device="cuda")
    for t, k, p in ((1.0, 40, 1.0), (0.7, 0, 0.9), (1.6, 1000, 0.5), (1.0, 4095, 1.0)):
        keep, margin = keep_and_margin(z, t, k, p)
        assert margin >= KERNEL_MARGIN, (t, k, p, margin)
        k_sample_ex(lib, _lib, stream, zd, V, t, k, p, 5, 0, n, got)
        k_sample(lib, _lib, stream, torch.from_numpy(masked(z, keep)).cuda(), V, t, 5, 0, n, want)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want.cpu().numpy()), (t, k, p)


@pytest.mark.parametrize("V", [390, 1384])
def test_sample_rows_ex_equals_the_per_row_calls(V):
    torch, _lib, lib, stream = gpu()
    B, ldz, seed, ctr = 37, V + 6, 99, 5
    z = np.random.default_rng(V).standard_normal((B, ldz)).astype(np.float32) * 3
    zd = torch.from_numpy(z).cuda()
    prm = [ROW_PARAMS[b % len(ROW_PARAMS)] for b in range(B)]
    ta = np.array([q[0] for q in prm], np.float32)
    ka = np.array([q[1] for q in prm], np.int32)
    pa = np.array([q[2] for q in prm], np.float32)
    got = torch.empty(B, dtype=torch.int32, device="cuda")
    _lib.check(lib.cmp_k_sample_rows_ex(stream, C.c_void_p(zd.data_ptr()), ldz, B, V, ta.ctypes.data_as(C.c_void_p),
                                        ka.ctypes.data_as(C.c_void_p), pa.ctypes.data_as(C.c_void_p), seed, ctr,
                                        C.c_void_p(got.data_ptr())))
    want = torch.empty(B, dtype=torch.int32, device="cuda")
    plain = torch.empty(B, dtype=torch.int32, device="cuda")
    for b in range(B):
        k_sample_ex(lib, _lib, stream, zd[b], V, float(ta[b]), int(ka[b]), float(pa[b]), seed + b, ctr, 1, want[b:])
    # null arrays: the defaults (temperature 1, filters off) = cmp_k_sample_rows
    _lib.check(lib.cmp_k_sample_rows_ex(stream, C.c_void_p(zd.data_ptr()), ldz, B, V, None, None, None, seed, ctr,
                                        C.c_void_p(plain.data_ptr())))
    ref = torch.empty(B, dtype=torch.int32, device="cuda")
    _lib.check(lib.cmp_k_sample_rows(stream, C.c_void_p(zd.data_ptr()), ldz, B, V, 1.0, seed, ctr, C.c_void_p(ref.data_ptr())))
    torch.cuda.synchronize()
    assert got.cpu().tolist() == want.cpu().tolist()
    assert plain.cpu().tolist() == ref.cpu().tolist()
    for b in range(B):
        keep, margin = keep_and_margin(z[b, :V], *prm[b])
        assert margin < DELTA or int(got[b]) in keep, b


# ---------------------------------------------------------------- 2. distribution
@pytest.mark.parametrize("temperature", [0.7, 1.6])
@pytest.mark.parametrize("k,p", [(40, 1.0), (0, 0.9), (40, 0.9)])
def test_truncated_draws_follow_the_renormalised_softmax(temperature, k, p):
    torch, _lib, lib, stream = gpu()
    n = 200_000
    z = round3_row(V0)
    keep, margin = keep_and_margin(z, temperature, k, p)
    assert margin >= KERNEL_MARGIN
    zd = torch.from_numpy(z).cuda()
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    k_sample_ex(lib, _lib, stream, zd, V0, temperature, k, p, 123, 0, n, ids)
    torch.cuda.synchronize()
    got = ids.cpu().numpy()
    counts = np.bincount(got, minlength=V0).astype(np.float64)
    outside = np.setdiff1d(np.arange(V0), keep)
    assert counts[outside].sum() == 0                                    # zero draws outside the kept set
    pv, dof = chi_square_p(counts[keep], truncated_probs(z, temperature, keep)[keep])
    print("chi-square: p-value %.4g, dof %d, kept %d" % (pv, dof, len(keep)))
    assert dof >= 3 and pv > 1e-3, (pv, dof)
    # resolution: the same counts against the neighbouring set (top_k + 8, resp. top_p + 0.03) are far outside
    k2, p2 = (k + 8, p) if p == 1.0 else (k, min(p + 0.03, 1.0))
    keep2 = keep_and_margin(z, temperature, k2, p2)[0]
    assert len(keep2) > len(keep)
    pv2 = chi_square_p(counts[keep2], truncated_probs(z, temperature, keep2)[keep2])[0]
    print("against (%d, %.2f): p-value %.4g, kept %d" % (k2, p2, pv2, len(keep2)))
    assert pv2 < 1e-6, pv2


# ---------------------------------------------------------------- 3. both chains, every mode
W_SMALL, KEEP_SMALL = 32, 12


def small_model(W=W_SMALL, seed=4):
    from composer_amd.transformer import Transformer
    return Transformer(V0, 64, W, 2, 4, attention_dropout_rate=0.0, residual_dropout_rate=0.0, dtype="fp32", seed=seed,
                       max_batch=1, max_seq=W)


def steps_for(mode):
    return {"literal": 24, "kv": 20, "kv-slide": 3 * W_SMALL}[mode]          # kv-slide: slides at 32, 53, 74, 95 tokens


def prompts_for(B, rng):
    return [rng.integers(0, V0, int(k)).astype(np.int32) for k in rng.integers(1, 13, B)]


def begin_one(m, _lib, p, mode, t, k, q, seed):
    mm = _lib.DECODE_LITERAL if mode == "literal" else _lib.DECODE_KV
    _lib.check(m._lib.cmp_decode_begin_ex(m._h, p.ctypes.data_as(C.c_void_p), len(p), mm, KEEP_SMALL if mode == "kv-slide" else 0,
                                          t, k, q, seed), "begin_ex")


def begin_batch(m, _lib, prompts, mode, prm, seed):
    B, ld = len(prompts), max(len(p) for p in prompts)
    buf = np.zeros((B, ld), np.int32)
    for b, p in enumerate(prompts):
        buf[b, :len(p)] = p
    lens = np.array([len(p) for p in prompts], np.int32)
    ta = np.array([q[0] for q in prm], np.float32)
    ka = np.array([q[1] for q in prm], np.int32)
    pa = np.array([q[2] for q in prm], np.float32)
    mm = _lib.DECODE_LITERAL if mode == "literal" else _lib.DECODE_KV
    _lib.check(m._lib.cmp_decode_batch_begin_ex(m._h, buf.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), B, ld, mm,
                                                KEEP_SMALL if mode == "kv-slide" else 0, ta.ctypes.data_as(C.c_void_p),
                                                ka.ctypes.data_as(C.c_void_p), pa.ctypes.data_as(C.c_void_p), seed), "batch_begin_ex")


def first_rows(m, prompts):
    """the logits every row's first id is drawn from: the forward pass on the prompt, last position"""
    return np.stack([m(p.reshape(1, -1))[0][0, -1] for p in prompts])


def check_ids_against_the_masked_rows(ids, Z, prm, seed, what):
    """ids [B][n], Z [B][n][V] (the row each id was drawn from): every id equals cmp_k_sample on the host-masked row with
    (seed + b, counter i).  Undecidable top-p steps are skipped and counted."""
    torch, _lib, lib, stream = gpu()
    B, n, V = Z.shape
    M = np.empty_like(Z)
    skip = np.zeros((B, n), bool)
    for b in range(B):
        t, k, q = prm[b]
        for i in range(n):
            keep, margin = keep_and_margin(Z[b, i], t, k, q)
            skip[b, i] = margin < DELTA
            M[b, i] = masked(Z[b, i], keep)
    md = torch.from_numpy(M).cuda()
    want = torch.empty((B, n), dtype=torch.int32, device="cuda")
    for b in range(B):
        for i in range(n):
            k_sample(lib, _lib, stream, md[b, i], V, float(prm[b][0]), seed + b, i, 1, want[b, i:])
    torch.cuda.synchronize()
    w = want.cpu().numpy()
    bad = (w != ids) & ~skip
    assert not bad.any(), (what, np.argwhere(bad)[:5].tolist(), ids[bad][:5], w[bad][:5])
    return int(skip.sum()), B * n


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_batch1_chain_draws_from_the_kept_set_of_its_logits(mode, graph, monkeypatch):
    from composer_amd import _lib
    monkeypatch.setenv("COMPOSER_NO_GRAPH", "0" if graph else "1")
    m = small_model()
    rng = np.random.default_rng(21)
    n, seed = steps_for(mode), 31
    skipped = cases = 0
    for j, (t, k, q) in enumerate(ROW_PARAMS[1:5]):
        p = prompts_for(1, rng)[0]
        z0 = first_rows(m, [p])
        begin_one(m, _lib, p, mode, t, k, q, seed + j)
        ids = np.zeros((1, n), np.int32)
        Z = np.zeros((1, n, V0), np.float32)
        Z[0, 0] = z0[0]
        one = np.zeros(1, np.int32)
        for i in range(n):
            _lib.check(m._lib.cmp_decode_steps(m._h, 1, one.ctypes.data_as(C.c_void_p)), "steps")
            ids[0, i] = one[0]
            if i >= 1:
                _lib.check(m._lib.cmp_decode_logits_get(m._h, Z[0, i].ctypes.data_as(C.c_void_p)), "logits")
        s, c = check_ids_against_the_masked_rows(ids, Z, [(t, k, q)], seed + j, (mode, graph, t, k, q))
        skipped += s; cases += c
        # steps(n) equals n steps of one, and the Python wrapper is the same call
        out = m.generate(p, n, temperature=t, mode=mode, seed=seed + j, top_k=k, top_p=q,
                         **({"slide_keep": KEEP_SMALL} if mode == "kv-slide" else {}))
        assert out.tolist() == ids[0].tolist(), (mode, graph, t, k, q)
        if mode == "kv-slide":
            assert m.decode_slide_stats()[0] >= 3                        # several slides happened
    assert skipped <= 0.01 * cases, (skipped, cases)
    m.close()


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("B", [3, 37])
@pytest.mark.parametrize("mode", MODES)
def test_batched_chain_draws_from_each_rows_own_kept_set(mode, B, graph, monkeypatch):
    from composer_amd import _lib
    monkeypatch.setenv("COMPOSER_NO_GRAPH", "0" if graph else "1")
    m = small_model()
    rng = np.random.default_rng(100 + B)
    n, seed = steps_for(mode), 57
    prompts = prompts_for(B, rng)
    prm = [ROW_PARAMS[(b + 3) % len(ROW_PARAMS)] for b in range(B)]       # B = 3: the greedy row included
    Z = np.zeros((B, n, V0), np.float32)
    Z[:, 0] = first_rows(m, prompts)
    begin_batch(m, _lib, prompts, mode, prm, seed)
    ids = np.zeros((B, n), np.int32)
    one = np.zeros((B, 1), np.int32)
    zb = np.zeros((B, V0), np.float32)
    for i in range(n):
        _lib.check(m._lib.cmp_decode_batch_steps(m._h, 1, one.ctypes.data_as(C.c_void_p)), "batch_steps")
        ids[:, i] = one[:, 0]
        if i >= 1:
            _lib.check(m._lib.cmp_decode_batch_logits_get(m._h, zb.ctypes.data_as(C.c_void_p)), "batch_logits")
            Z[:, i] = zb
    skipped, cases = check_ids_against_the_masked_rows(ids, Z, prm, seed, (mode, B, graph))
    assert skipped <= 0.01 * cases, (skipped, cases)
    sk = {"slide_keep": KEEP_SMALL} if mode == "kv-slide" else {}
    # steps(n) equals n steps of one (through the Python wrapper, per-row sequences of parameters)
    out = m.generate_batch(prompts, n, temperature=[q[0] for q in prm], top_k=[q[1] for q in prm], top_p=[q[2] for q in prm],
                           mode=mode, seed=seed, **sk)
    assert out.tolist() == ids.tolist()
    if mode == "kv-slide":
        assert m.decode_slide_stats(batched=True)[0] >= 3 * B
    # a row of the batch equals `generate` on its prompt with seed + b and its own parameters
    for b in sorted({0, 1, B // 2, B - 1}):
        t, k, q = prm[b]
        alone = m.generate(prompts[b], n, temperature=t, top_k=k, top_p=q, mode=mode, seed=seed + b, **sk)
        assert alone.tolist() == ids[b].tolist(), (mode, B, graph, b)
    # changing the other rows' parameters does not change this row's ids
    other = [prm[b] if b == 1 else (0.9, 7, 0.8) for b in range(B)]
    out2 = m.generate_batch(prompts, n, temperature=[q[0] for q in other], top_k=[q[1] for q in other],
                            top_p=[q[2] for q in other], mode=mode, seed=seed, **sk)
    assert out2[1].tolist() == ids[1].tolist()
    assert out2[0].tolist() != ids[0].tolist()
    # greedy with the filters on equals greedy (the row whose temperature is 0, and a whole greedy batch)
    g0 = m.generate_batch(prompts, n, temperature=0.0, mode=mode, seed=seed, **sk)
    g1 = m.generate_batch(prompts, n, temperature=0.0, top_k=40, top_p=0.9, mode=mode, seed=seed, **sk)
    assert g0.tolist() == g1.tolist()
    bz = [b for b in range(B) if prm[b][0] == 0.0]
    assert bz and all(ids[b].tolist() == g0[b].tolist() for b in bz)
    m.close()


def test_begin_ex_refuses_bad_arguments_before_any_device_work():
    from composer_amd import _lib
    m = small_model()
    p = np.array([5, 6, 7], np.int32)
    lib, h = m._lib, m._h
    for k, q in ((-1, 1.0), (0, 0.0), (0, 1.5), (0, float("nan"))):
        assert lib.cmp_decode_begin_ex(h, p.ctypes.data_as(C.c_void_p), 3, _lib.DECODE_KV, 0, 1.0, k, q, 3) == -1
        assert "top_" in _lib.last_error()
    one = np.zeros(1, np.int32)
    assert lib.cmp_decode_steps(h, 1, one.ctypes.data_as(C.c_void_p)) == -4          # nothing was begun
    assert lib.cmp_decode_begin_ex(h, p.ctypes.data_as(C.c_void_p), 3, _lib.DECODE_LITERAL, 8, 1.0, 0, 1.0, 3) == -1   # keep: kv only
    assert lib.cmp_decode_begin_ex(h, p.ctypes.data_as(C.c_void_p), 3, _lib.DECODE_KV, W_SMALL, 1.0, 0, 1.0, 3) == -1
    for kw in ({"top_k": -1}, {"top_p": 0.0}, {"top_p": 1.5}, {"top_p": float("nan")}, {"top_k": 2.5}):
        with pytest.raises(ValueError, match="top_k|top_p"):
            m.generate(p, 4, **kw)
        with pytest.raises(ValueError, match="top_k|top_p"):
            m.generate_batch([p, p], 4, **kw)
    with pytest.raises(ValueError, match="top_k"):
        m.generate_batch([p, p], 4, top_k=[1, 2, 3])
    with pytest.raises(ValueError, match="top_p"):
        m.generate_batch([p, p], 4, top_p=[0.5, 1.5])
    m.close()


# ---------------------------------------------------------------- 4. filters off is the plain sampler
@pytest.mark.parametrize("mode", MODES)
def test_filters_off_is_the_call_without_the_keywords(mode):
    m = small_model()
    rng = np.random.default_rng(8)
    n, seed = steps_for(mode), 11
    sk = {"slide_keep": KEEP_SMALL} if mode == "kv-slide" else {}
    prompts = prompts_for(5, rng)
    for t in (1.0, 0.7):
        base = m.generate(prompts[0], n, temperature=t, mode=mode, seed=seed, **sk)
        assert m.generate(prompts[0], n, temperature=t, mode=mode, seed=seed, top_k=0, top_p=1.0, **sk).tolist() == base.tolist()
        assert m.generate(prompts[0], n, temperature=t, mode=mode, seed=seed, top_k=V0, **sk).tolist() == base.tolist()
        assert m.generate(prompts[0], n, temperature=t, mode=mode, seed=seed, top_k=40, **sk).tolist() != base.tolist()
        bb = m.generate_batch(prompts, n, temperature=t, mode=mode, seed=seed, **sk)
        assert m.generate_batch(prompts, n, temperature=t, mode=mode, seed=seed, top_k=0, top_p=1.0, **sk).tolist() == bb.tolist()
        assert m.generate_batch(prompts, n, temperature=t, mode=mode, seed=seed, top_k=V0, **sk).tolist() == bb.tolist()
        assert m.generate_batch(prompts, n, temperature=[t] * 5, top_k=[0] * 5, top_p=[1.0] * 5, mode=mode, seed=seed,
                                **sk).tolist() == bb.tolist()
        assert bb[0].tolist() == base.tolist()
    m.close()


# ---------------------------------------------------------------- 5. CLI
def test_cli_top_k_top_p_num_samples(tmp_path):
    from composer_amd import cli, checkpoint as ckpt, dataset as D
    cfg = yaml.safe_load(open(cli.get_default_config()))
    mc = cfg["transformer"]["model"]
    mc.update({"window_size": 64, "embedding_size": 64, "decoder_layers_count": 2, "attention_head_count": 4,
               "attention_dropout_rate": 0.0, "residual_dropout_rate": 0.0})
    cfg["transformer"]["runtime"] = {"dtype": "fp32", "seed": 3}
    run = tmp_path / "run"
    run.mkdir()
    (run / "config.yml").write_text(yaml.safe_dump(cfg))
    model, _ = cli.create_model(cli.ModelType.TRANSFORMER, cli.get_config_from_restoredir(run), dtype="fp32")
    ckpt.CheckpointManager(str(run)).save(model.state_dict(), {"step": 1})
    prompt = [5, 6, 7, 8]
    want = model.generate_batch([prompt] * 3, 16, temperature=1.0, mode="kv", top_k=40, top_p=0.9)
    plain = model.generate_batch([prompt] * 3, 16, temperature=1.0, mode="kv")
    one = model.generate(prompt, 16, temperature=1.0, mode="kv", top_k=40, top_p=0.9)
    model.close()
    assert want.tolist() != plain.tolist() and len({tuple(r) for r in want.tolist()}) == 3
    r = CliRunner()
    base = ["generate", "transformer", str(run)]
    opts = ["--prompt-ids", "5,6,7,8", "--length", "16", "--decode-mode", "kv-cache", "--top-k", "40", "--top-p", "0.9"]
    res = r.invoke(cli.cli, base + [str(tmp_path / "many.data")] + opts + ["--num-samples", "3"], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    assert "decode-mode: kv-cache" in res.stderr and "top-k 40" in res.stderr and "top-p 0.9" in res.stderr
    lines = res.stdout.strip().split("\n")[-3:]
    for i in range(3):
        assert [int(t) for t in lines[i].split(",")] == want[i].tolist(), i
        got, _ = D.read_data_file(tmp_path / ("many-%d.data" % i))
        assert got.tolist() == prompt + want[i].tolist()
    res = r.invoke(cli.cli, base + [str(tmp_path / "one.data")] + opts, catch_exceptions=False)
    assert res.exit_code == 0, res.output
    assert [int(t) for t in res.stdout.strip().split("\n")[-1].split(",")] == one.tolist() == want[0].tolist()
