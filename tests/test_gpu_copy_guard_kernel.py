"""-m gpu: cmp_k_copy_bans (composer_amd/csrc/copyguard.hip) against the host restatement composer_amd.novelty.copy_bans, bit for
bit, words and counts, on the guard-banded arena of tests/kernel_arena.py.

The corpus ends flush against a guard band (0xFF bytes: an over-read shows as the id 65535, which no history may hold), and so do the
start bits, the histories (leading dimension 71), the lengths and the static words.  Both outputs are pre-filled with a poison of
their own, not the arena's 0xFF: a ban word of 32 set bits is a legal value (velocity folding bans the 32 ids 256 .. 287 at once).  After the launch the guards and every input must be bitwise unchanged,
every word of both outputs written, and both equal to the restatement.  Integers only: no tolerance.

Shapes (tests/copy_guard_cases.py): n in {1, 7, 257, 4099}, M in {1, 2, 16, 64}, B in {1, 3, 16}, N in {0, 2}, velocity folding on
and off; rows with lens < M and lens == 0; a static vector whose bits the scan must keep; planted copies that start at 0 and whose
continuation is c[n - 1]; a corpus pointer that is not 16-byte aligned; and the refusals the library decides."""
import ctypes as C

import numpy as np
import pytest
import torch

import copy_guard_cases as cg
from kernel_arena import Arena

pytestmark = pytest.mark.gpu
POISON = -(1 << 61)
POISON_W = 0x5A5AA5A5                      # no ban word of the cases: the static bits of a case are a dozen, the bans a few ranges


def start_words(starts, n):
    w = np.zeros(-(-n // 32), np.uint32)
    for s in starts:
        w[int(s) >> 5] |= np.uint32(1 << (int(s) & 31))
    return w.view(np.int32)


@pytest.fixture(scope="module")
def lib():
    from composer_amd import _lib
    l = _lib.load()
    _lib.require_gpu()
    return l


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def opts_of(c):
    from composer_amd import _lib
    v = c.velocity or (0, 0)
    return _lib.CopyGuardOpts(c.M, c.N, v[0], v[1])


def run_case(lib, c, skew=0, with_static=True, with_bits=True):
    """One launch on a fresh arena -> (words [B, nw] uint32, counts [B] int64).  skew: the corpus is handed over `skew` ids behind the
    start of its window (the stream is then that much shorter), so the pointer is not 16-byte aligned."""
    nw = (cg.V + 31) // 32
    ar = Arena(nbytes=1 << 20)
    s_ids = ar.vector(torch.from_numpy(c.corpus.astype(np.int16)), torch.int16, name="corpus")
    s_bits = ar.vector(torch.from_numpy(start_words(c.starts, c.n).copy()), torch.int32, name="start bits")
    s_h = ar.operand(torch.from_numpy(c.hist), torch.int32, c.B, c.ld, c.ld, name="history")
    s_lens = ar.vector(torch.tensor(c.lens, dtype=torch.int32), torch.int32, name="lens")
    s_static = ar.vector(torch.from_numpy(c.static.view(np.int32).copy()), torch.int32, name="static words")
    s_words = ar.accumulator(torch.full((c.B, nw), POISON_W, dtype=torch.int32), torch.int32, c.B, nw, nw, name="ban words")
    s_count = ar.accumulator(torch.full((c.B,), POISON, dtype=torch.int64), torch.int64, 1, c.B, c.B, name="counts")
    ar.arm()
    layout, o = c.layout.to_c(), opts_of(c)
    rc = lib.cmp_k_copy_bans(stream(), C.c_void_p(s_ids.ptr() + 2 * skew), c.n - skew, C.c_void_p(s_bits.ptr()) if with_bits else None,
                             C.byref(layout), C.byref(o), C.c_void_p(s_h.ptr()), C.c_void_p(s_lens.ptr()), c.B, c.ld, cg.V,
                             C.c_void_p(s_static.ptr()) if with_static else None, C.c_void_p(s_words.ptr()), C.c_void_p(s_count.ptr()))
    assert rc == 0, lib.cmp_last_error().decode()
    ar.check()                   # guards and inputs bitwise unchanged
    got = s_words.host().numpy().view(np.uint32)
    assert not (got == POISON_W).any(), "ban words: element %s was never written" % np.argwhere(got == POISON_W)[0].tolist()
    counts = s_count.host().numpy().reshape(-1)
    assert not (counts == POISON).any(), "counts: row %d was never written" % int(np.argmax(counts == POISON))
    return got, counts


@pytest.mark.parametrize("name", cg.NAMES)
def test_copy_bans_kernel_equals_the_host_restatement(lib, name):
    c = cg.case(name)
    _, want_words, want_counts = cg.reference(name)
    words, counts = run_case(lib, c)
    bad = np.argwhere(words != want_words)
    assert bad.size == 0, "%s: ban words differ at (row, word) %s: got %08x, reference %08x (row lengths %s)" % (
        name, bad[0].tolist(), words[tuple(bad[0])], want_words[tuple(bad[0])], c.lens)
    assert np.array_equal(counts, want_counts), (name, counts.tolist(), want_counts.tolist())
    assert (words & c.static == c.static).all()              # the static bits, those at or above V included, are kept
    for b in range(c.B):
        if c.lens[b] < c.M:
            assert np.array_equal(words[b], c.static) and counts[b] == 0


@pytest.mark.parametrize("name,skew", [("n4099_m16", 3), ("n257_m2", 5), ("n4099_m64", 1)])
def test_a_corpus_that_is_not_16_byte_aligned(lib, name, skew):
    """The scan loads 16 bytes at a time where it can: a stream that starts `skew` ids behind an aligned address, with no start bits
    and no static words (both null)."""
    from composer_amd import novelty
    c = cg.case(name)
    words, counts = run_case(lib, c, skew=skew, with_static=False, with_bits=False)
    for b in range(c.B):
        want = novelty.copy_bans(c.corpus[skew:], None, c.hist[b, :c.lens[b]], cg.V, c.layout, c.M, c.N, c.velocity)
        assert np.array_equal(words[b], cg.to_words(want)), (name, b)
        assert counts[b] == want.sum()


def test_the_library_refuses_what_the_contract_refuses(lib):
    from composer_amd import _lib
    z = torch.zeros(8192, dtype=torch.int32, device="cuda")
    P = C.c_void_p(z.data_ptr())
    W, Cn = C.c_void_p(z.data_ptr() + 4096), C.c_void_p(z.data_ptr() + 16384)
    g = cg.LAYOUT.to_c()

    def k(n=64, layout=g, o=(2, 0, 0, 0), B=1, ld=8, V=cg.V, ids=P, hist=P, lens=P, words=W, count=Cn):
        oo = _lib.CopyGuardOpts(*o)
        return lib.cmp_k_copy_bans(stream(), ids, n, None, C.byref(layout) if layout is not None else None, C.byref(oo), hist, lens, B,
                                   ld, V, None, words, count)
    bad_notes = cg.LAYOUT.to_c()
    bad_notes.note_off0 = 100
    for kw in (dict(o=(0, 0, 0, 0)), dict(o=(65, 0, 0, 0)), dict(o=(2, -1, 0, 0)), dict(o=(2, 25, 0, 0)), dict(layout=None),
               dict(o=(2, 0, 100, 40)), dict(o=(2, 0, 250, 10)), dict(o=(2, 0, 65530, 10)), dict(o=(2, 0, 0, -1)), dict(layout=bad_notes),
               dict(n=0), dict(n=1 << 40), dict(B=0), dict(B=257), dict(ld=0), dict(V=0), dict(ids=None), dict(hist=None), dict(lens=None),
               dict(words=None), dict(count=None)):
        assert k(**kw) == -1, kw
        assert lib.cmp_last_error().decode()
    assert k() == 0, lib.cmp_last_error().decode()          # the same arguments, nothing wrong: runs
    torch.cuda.synchronize()
