"""-m gpu: cmp_k_novelty (composer_amd/csrc/novelty.hip) against the host restatement composer_amd.novelty.match_table, bit for bit, on
the guard-banded arena of tests/kernel_arena.py.

The corpus ends flush against a guard band (0xFF bytes: an over-read shows as the id 65535, which no query may hold), and so do the
start bits, the queries and the lengths.  len is pre-filled with 0xFF like every arena output; pos and k are pre-filled with a poison
of their own (novelty_cases.POISON_POS / POISON_K), because -1 -- the 0xFF pattern -- is a legal value of both.  After the launch the
guards, the corpus, the start bits, the queries and the lengths must be bitwise unchanged, every element of the three outputs
written, and all three equal to the restatement.  The query rows' padding behind lens[b] holds -1.  Integers only: no tolerance.

Shapes (tests/novelty_cases.py): n in {1, 255, 256, 257, 5000, 70000}, L in {1, 2, 63, 64, 65, 300, 1025}, B in {1, 3} ragged, N in
{0, 2} (one and seven counters per lane), velocity folding on and off.  Also cmp_novelty through a cmp_dataset on two cases, and
every refusal the library decides."""
import ctypes as C

import numpy as np
import pytest
import torch

import novelty_cases as nc
from composer_amd import novelty
from kernel_arena import Arena

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from composer_amd import _lib
    l = _lib.load()
    _lib.require_gpu()
    return l


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def start_words(starts, n):
    w = np.zeros(-(-n // 32), np.uint32)
    for s in starts:
        w[int(s) >> 5] |= np.uint32(1 << (int(s) & 31))
    return w.view(np.int32)


def opts_of(c):
    from composer_amd import _lib
    v = c.velocity or (0, 0)
    return _lib.NoveltyOpts(c.min_match, c.N, v[0], v[1])


@pytest.mark.parametrize("name", nc.NAMES)
def test_novelty_kernel_equals_the_host_restatement(lib, name):
    c = nc.case(name)
    ar = Arena(nbytes=1 << 20)
    s_ids = ar.vector(torch.from_numpy(c.corpus.astype(np.int16)), torch.int16, name="corpus")     # (ids < 32768: the same 16 bits)
    s_bits = ar.vector(torch.from_numpy(start_words(c.starts, c.n).copy()), torch.int32, name="start bits")
    x = np.full((c.B, c.ld), -1, np.int32)
    for b, r in enumerate(c.rows):
        x[b, :len(r)] = r
    s_x = ar.operand(torch.from_numpy(x), torch.int32, c.B, c.ld, c.ld, name="x")
    s_lens = ar.vector(torch.tensor(c.lens, dtype=torch.int32), torch.int32, name="lens")
    s_len = ar.output(torch.int32, c.B, c.ld, c.ld, name="len")
    s_pos = ar.accumulator(torch.full((c.B, c.ld), nc.POISON_POS, dtype=torch.int64), torch.int64, c.B, c.ld, c.ld, name="pos")
    s_k = ar.accumulator(torch.full((c.B, c.ld), nc.POISON_K, dtype=torch.int32), torch.int32, c.B, c.ld, c.ld, name="k")
    ar.arm()
    layout, o = c.layout.to_c(), opts_of(c)
    rc = lib.cmp_k_novelty(stream(), C.c_void_p(s_ids.ptr()), c.n, C.c_void_p(s_bits.ptr()), C.byref(layout), C.c_void_p(s_x.ptr()),
                           C.c_void_p(s_lens.ptr()), c.B, c.ld, C.byref(o), C.c_void_p(s_len.ptr()), C.c_void_p(s_pos.ptr()),
                           C.c_void_p(s_k.ptr()))
    assert rc == 0, lib.cmp_last_error().decode()
    ar.check()                   # guards, corpus, start bits, queries, lengths bitwise unchanged; every element of len written
    got_len, got_pos, got_k = s_len.host().numpy(), s_pos.host().numpy(), s_k.host().numpy()
    assert not (got_pos == nc.POISON_POS).any(), "pos: element %s was never written" % np.argwhere(got_pos == nc.POISON_POS)[0].tolist()
    assert not (got_k == nc.POISON_K).any(), "k: element %s was never written" % np.argwhere(got_k == nc.POISON_K)[0].tolist()
    nc.compare(name, got_len, got_pos, got_k)


def test_one_piece_needs_no_start_bits_and_no_layout(lib):
    """start_bits_dev = null is one piece; layout = null is enough while N = 0."""
    c = nc.case("n257b")
    ids = torch.from_numpy(c.corpus.astype(np.int16)).cuda()
    row = c.rows[0]
    x = torch.from_numpy(row.copy()).cuda()
    lens = torch.tensor([len(row)], dtype=torch.int32, device="cuda")
    ln = torch.empty(len(row), dtype=torch.int32, device="cuda")
    ps = torch.empty(len(row), dtype=torch.int64, device="cuda")
    ks = torch.empty(len(row), dtype=torch.int32, device="cuda")
    from composer_amd import _lib
    o = _lib.NoveltyOpts(2, 0, 0, 0)
    P = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.cmp_k_novelty(stream(), P(ids), c.n, None, None, P(x), P(lens), 1, len(row), C.byref(o), P(ln), P(ps), P(ks))
    assert rc == 0, lib.cmp_last_error().decode()
    torch.cuda.synchronize()
    want = novelty.match_table(c.corpus, None, row, None, 2, 0, None)
    for got, ref in zip((ln, ps, ks), want):
        assert np.array_equal(got.cpu().numpy(), ref)


@pytest.mark.parametrize("name", ["n5000_fold", "n257b"])
def test_cmp_novelty_through_a_dataset(name):
    c = nc.case(name)
    corpus = novelty.Corpus(c.corpus, c.starts, None, c.layout, nc.VELOCITY)
    try:
        ln, ps, ks, lens = corpus.match_arrays(c.rows, c.min_match, c.N, ignore_velocity=c.velocity is not None)
        assert lens.tolist() == c.lens
        nc.compare(name, ln, ps, ks)
        reports = corpus.match(c.rows, c.min_match, c.N, ignore_velocity=c.velocity is not None)
        ref = nc.reference(name)
        for b, r in enumerate(reports):
            assert np.array_equal(r.len, ref[0][b, :c.lens[b]]) and np.array_equal(r.pos, ref[1][b, :c.lens[b]])
            assert r.coverage == novelty.coverage_of(ref[0][b, :c.lens[b]])
    finally:
        corpus.close()


def test_the_library_refuses_what_the_contract_refuses(lib):
    from composer_amd import _lib
    z = torch.zeros(4096, dtype=torch.int32, device="cuda")
    P = C.c_void_p(z.data_ptr())
    outs = tuple(C.c_void_p(z.data_ptr() + 4096 * i) for i in (1, 2, 3))        # three disjoint windows of the same buffer
    g = nc.LAYOUT.to_c()

    def k_novelty(n=64, layout=g, B=1, ld=8, o=(1, 0, 0, 0), ids=P, x=P, lens=P, out=outs):
        oo = _lib.NoveltyOpts(*o)
        return lib.cmp_k_novelty(stream(), ids, n, None, C.byref(layout) if layout is not None else None, x, lens, B, ld, C.byref(oo), *out)
    bad_notes = nc.LAYOUT.to_c()
    bad_notes.note_off0 = 100
    far = nc.LAYOUT.to_c()
    far.note_on0 = 65500
    for kw in (dict(n=0), dict(n=1 << 40), dict(B=0), dict(B=257), dict(ld=0), dict(ld=32769), dict(o=(0, 0, 0, 0)), dict(o=(1, -1, 0, 0)),
               dict(o=(1, 25, 0, 0)), dict(o=(1, 1, 0, 0), layout=None), dict(o=(1, 0, -1, 4)), dict(o=(1, 0, 65530, 10)),
               dict(o=(1, 0, 0, -1)), dict(o=(1, 0, 100, 40)), dict(o=(1, 0, 250, 10)), dict(layout=bad_notes), dict(layout=far),
               dict(ids=None), dict(x=None), dict(lens=None), dict(out=(None, P, P)), dict(out=(P, None, P)), dict(out=(P, P, None))):
        assert k_novelty(**kw) == -1, kw
        assert lib.cmp_last_error().decode()
    assert k_novelty() == 0, lib.cmp_last_error().decode()          # the same arguments, nothing wrong: runs
    torch.cuda.synchronize()
    # through a dataset: lengths, query ids, the layout rule, the piece list
    ctx, h = C.c_void_p(), C.c_void_p()
    assert lib.cmp_ctx_create(0, C.byref(ctx)) == 0
    ids = np.arange(100, dtype=np.uint16)
    assert lib.cmp_dataset_create(ctx, ids.ctypes.data_as(C.c_void_p), 100, None, C.byref(h)) == 0
    try:
        def pieces(st):
            a = np.asarray(st, np.int64)
            return lib.cmp_dataset_set_pieces(h, a.ctypes.data_as(C.c_void_p), len(a))
        for st in ([1, 5], [0, 7, 3], [0, 100], [0, -1], []):
            assert pieces(st) == -1, st
        assert lib.cmp_dataset_set_pieces(h, None, 1) == -1
        assert pieces([0, 50]) == 0 and pieces([0, 10, 10, 60]) == 0          # replaced; an empty piece is allowed

        def run(x, lens, ld, o=(1, 0, 0, 0)):
            x, lens = np.asarray(x, np.int32), np.asarray(lens, np.int32)
            B = len(lens)
            ln, ps, ks = np.empty((B, ld), np.int32), np.empty((B, ld), np.int64), np.empty((B, ld), np.int32)
            oo = _lib.NoveltyOpts(*o)
            A = lambda a: a.ctypes.data_as(C.c_void_p)
            return lib.cmp_novelty(h, A(x), A(lens), B, ld, C.byref(oo), A(ln), A(ps), A(ks)), ln, ps, ks
        assert run([[1, 2, 3, 4]], [0], 4)[0] == -1
        assert run([[1, 2, 3, 4]], [5], 4)[0] == -1
        assert run([[1, 2, -1, 4]], [4], 4)[0] == -1
        assert run([[1, 2, 65535, 4]], [4], 4)[0] == -1
        assert run([[1, 2, 3, 4]], [4], 4, (1, 1, 0, 0))[0] == -1               # N > 0, a dataset without a layout
        rc, ln, ps, ks = run([[8, 9, 10, 11], [58, 59, 60, 61]], [4, 3], 4, (2, 0, 0, 0))
        assert rc == 0, lib.cmp_last_error().decode()
        assert ln.tolist() == [[2, 0, 2, 0], [2, 0, 0, 0]]                    # the starts at 10 and 60 cut the runs
        assert ps.tolist() == [[8, -1, 10, -1], [58, -1, -1, -1]] and not ks.any()
        rc, _, _, _ = run([[1, 2, -1, 70000]], [2], 4)                         # ids behind the length are not looked at
        assert rc == 0
    finally:
        lib.cmp_dataset_destroy(h)
        lib.cmp_ctx_destroy(ctx)
