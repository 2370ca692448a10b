"""Corpora, queries and case features shared by the novelty tests (tests/test_novelty_host.py and tests/test_novelty_checks_host.py on
the CPU, tests/test_gpu_novelty_kernel.py on the device), and the comparison all of them use.

Streams are drawn from a six-id alphabet (two TIME_SHIFTs, two VELOCITYs, the pedal pair) plus a few notes of the real layout, so chance
matches and ties are plentiful; on top, copies of query segments are PLANTED in the corpus at positions chosen for what the kernel
(composer_amd/csrc/novelty.hip: NOV_BLOCK = 256 diagonals per workgroup, NOV_SCHUNK = 512 query positions per LDS chunk) can get
wrong.  Every plant records what the host restatement must report at its query position; `covered()` returns the features whose
recorded expectations the restatement really meets, so a change of the streams cannot silently stop covering one.

A plant is PLANT tokens long (8 in the small cases) and is followed in the corpus by a token that differs from the query's next
one, so its run has exactly that length.  Generic plants take query positions 4 apart: at its own position a plant is 4 tokens
longer than its predecessor's remainder, hence the unique winner.  The special segments at the front of row 0 use TIME_SHIFT ids that
occur nowhere else, so nothing matches them by chance."""
import numpy as np

from composer_amd import novelty
from composer_amd.grammar import EventGrammar

KERNEL_BLOCK, KERNEL_SCHUNK = 256, 512
LAYOUT = EventGrammar.from_dataset_params(10, 100, 32, rules=0)          # notes 0 / 128, velocities 256..287, shifts 288..387, pedal 388 / 389
VELOCITY = (256, 32)
ALPHABET = (288, 297, 259, 263, 388, 389)
PITCHES = (0, 1, 2, 60, 62, 64, 125, 126, 127)
SPECIAL_ROOM = 92              # query positions of row 0 the special segments take (7 x 13 + 1)

ALL_FEATURES = ("every_block_edge", "block_edge_last", "block_edge_first", "s_chunk_512", "s_chunk_1024", "copy_at_p0",
                "copy_ends_at_n_minus_1", "copy_to_query_end", "piece_start_inside", "diag_p_below_s", "equal_copies_lower_p",
                "k0_beats_plus2", "minus2_beats_plus2", "no_clip_126", "fold_on", "fold_off", "run_min_match_minus_1",
                "run_exactly_min_match", "pad_tail", "n_1", "one_chunk_rows_share", "many_chunks")

#        name            n      L    B  N  fold   min_match
GRID = (("n1",           1,     1,   1, 0, False, 1),
        ("n255",         255,   2,   1, 0, False, 1),
        ("n256",         256,   63,  3, 0, False, 3),
        ("n257a",        257,   64,  1, 2, True,  3),
        ("n257b",        257,   65,  3, 2, False, 2),
        ("n5000_fold",   5000,  300, 3, 2, True,  4),
        ("n5000_exact",  5000,  300, 3, 2, False, 4),
        ("n5000_long",   5000,  1025, 1, 0, False, 6),
        ("n70000",       70000, 1025, 3, 2, True,  5))
NAMES = tuple(g[0] for g in GRID)
SMALL = ("n1", "n255", "n256", "n257a", "n257b")             # cheap enough for the triple loop

_cases, _refs = {}, {}


class Case:
    pass


def _lens(L, B):
    return [L, max(1, (2 * L) // 3), max(1, L - 1)][:B]


def build(name, n, L, B, N, fold, min_match):
    rng = np.random.default_rng(sum(map(ord, name)) + 7)
    c = Case()
    c.name, c.n, c.ld, c.B, c.N, c.min_match = name, n, L, B, N, min_match
    c.layout, c.velocity = LAYOUT, (VELOCITY if fold else None)
    notes = [LAYOUT.note_on0 + p for p in PITCHES] + [LAYOUT.note_off0 + p for p in PITCHES]

    def draw(k):
        return np.where(rng.random(k) < 0.7, rng.choice(ALPHABET, size=k), rng.choice(notes, size=k)).astype(np.int64)
    corpus = draw(n)
    c.lens = _lens(L, B)
    rows = [draw(l) for l in c.lens]
    starts = {0}
    if n >= 255:
        starts |= {int(v) for v in rng.integers(1, n, size=max(2, n // 700))}
    c.expect = []                                  # (feature, b, s, kind, value): kind "pos_k" -> (pos, k), "len" -> len, "not_pos" -> pos
    c.features = set()
    M = 12 if L >= 300 else 8
    c.plant = M
    used = np.zeros(n, bool)
    pool = iter(range(300, 388))                   # TIME_SHIFT ids that occur nowhere else
    u = lambda: next(pool)

    def free(p0, m):
        return 0 <= p0 and p0 + m <= n and not used[max(0, p0 - 1):min(n, p0 + m + 1)].any()

    def put(p0, tokens, next_query=None):
        m = len(tokens)
        corpus[p0:p0 + m] = tokens
        used[max(0, p0 - 1):min(n, p0 + m + 1)] = True
        if p0 + m < n:                                 # the run ends here: a breaker that no query token equals by chance
            corpus[p0 + m] = 298 if next_query != 298 else 299

    def find(m, lo=1):
        for p0 in range(lo, n - m):
            if free(p0, m):
                return p0
        raise AssertionError("%s: no room for a plant" % name)

    def moved(tokens, k):
        return novelty.map_query(np.asarray(tokens, np.int64), k, LAYOUT, (0, 0))
    special = L >= 300 and n >= 5000
    if special:
        on, off = LAYOUT.note_on0, LAYOUT.note_off0
        seg = lambda i: 13 * i
        x0 = rows[0]
        # k = 0 against k = +2, the transposed copy at the LOWER position
        A = [on + 60, u(), on + 62, off + 60, u(), on + 64, off + 62, u(), off + 64, on + 60, u(), off + 60]
        B2 = [on + 62, u(), on + 60, off + 62, u(), on + 64, off + 60, u(), off + 64, on + 62, u(), off + 62]
        Cq = [on + 60, u(), off + 60, u(), on + 62, on + 126, u(), off + 62, on + 64, u(), off + 64, off + 126]
        D = [on + 60, 256 + 3, u(), off + 60, u(), on + 62, u(), 256 + 20, off + 62, u(), on + 64, off + 64]
        E = [u() for _ in range(min_match)] + [u()]
        F = [u() for _ in range(min_match)] + [u()]
        for i, t in enumerate((A, B2, Cq, D, E, F)):
            x0[seg(i):seg(i) + len(t)] = t
            x0[seg(i) + len(t):seg(i + 1)] = 298 + (i & 1)            # filler that occurs nowhere in the corpus but as a breaker
        if N >= 2:
            lo = find(12)
            put(lo, moved(A, 2))
            hi = find(12, lo)
            put(hi, A)
            c.expect.append(("k0_beats_plus2", 0, seg(0), "pos_k", (hi, 0)))
            lo = find(12)
            put(lo, moved(B2, 2))
            hi = find(12, lo)
            put(hi, moved(B2, -2))
            c.expect.append(("minus2_beats_plus2", 0, seg(1), "pos_k", (hi, -2)))
            # pitch 126 + 2: the corpus holds pitch 127 there -- a clipping kernel matches all 12, the contract the first 5
            t = moved(Cq, 2)
            t[5], t[11] = on + 127, off + 127
            p0 = find(12)
            put(p0, t)
            c.expect.append(("no_clip_126", 0, seg(2), "len_pos_k", (5, p0, 2)))
        t = list(D)
        t[1], t[7] = 256 + 9, 256 + 1
        p0 = find(12)
        put(p0, t)
        if fold:
            c.expect.append(("fold_on", 0, seg(3), "pos_k", (p0, 0)))
        else:
            c.expect.append(("fold_off", 0, seg(3), "len", 0))         # on + 60 alone, then a velocity that differs
        p0 = find(min_match)
        put(p0, E[:min_match])
        c.expect.append(("run_exactly_min_match", 0, seg(4), "len_pos_k", (min_match, p0, 0)))
        p0 = find(min_match)
        put(p0, F[:min_match - 1])
        c.expect.append(("run_min_match_minus_1", 0, seg(5), "len", 0))
    # query slots of the generic plants, 4 apart
    slots = [(b, s) for b in range(B) for s in range(SPECIAL_ROOM if (special and b == 0) else 0, c.lens[b] - M + 1, 4)]
    taken = set()

    def plant_on(feature, d=None, p0=None, want=None, slot_ok=lambda b, s: True, solo=False):
        """One generic plant on diagonal d (or at p0, or anywhere): the first free slot that fits.  solo: the neighbouring slots stay
        empty (a plant cut in two must not lose to a neighbour's remainder).  -> (b, s, p0) or None."""
        for b, s in slots:
            if (b, s) in taken or not slot_ok(b, s):
                continue
            if solo and ((b, s - 4) in taken or (b, s + 4) in taken):
                continue
            q = d + s if d is not None else (p0 if p0 is not None else None)
            if q is None:
                q = find(M)
            if not free(q, M):
                continue
            taken.add((b, s))
            if solo:
                taken.update({(b, s - 4), (b, s + 4)})
            nxt = int(rows[b][s + M]) if s + M < c.lens[b] else None
            put(q, rows[b][s:s + M], nxt)
            c.expect.append((feature, b, s, "pos_k", (q, 0)) if want is None else (feature, b, s) + want(q))
            return b, s, q
        return None
    if L >= M and n >= 2 * M + 4:
        # copies across the s-chunk boundaries of row 0
        for mult in range(KERNEL_SCHUNK, c.lens[0], KERNEL_SCHUNK):
            plant_on("s_chunk_%d" % mult, slot_ok=lambda b, s: b == 0 and s < mult < s + M)
        got = plant_on("copy_at_p0", p0=0, slot_ok=lambda b, s: s > 0)
        if got:
            c.expect.append(("diag_p_below_s",) + got[:2] + ("pos_k", (0, 0)))
        plant_on("copy_ends_at_n_minus_1", p0=n - M)
        for b in range(B):                                             # a copy that runs to the end of the query (its slot is its own)
            s = c.lens[b] - M
            if s >= 0 and all(abs(s - t) >= 4 or bb != b for bb, t in taken) and not (special and b == 0 and s < SPECIAL_ROOM):
                q = find(M)
                put(q, rows[b][s:s + M])
                taken.add((b, s))
                c.expect.append(("copy_to_query_end", b, s, "len_pos_k", (M, q, 0)))
                for mult in range(KERNEL_SCHUNK, c.lens[b], KERNEL_SCHUNK):
                    if b == 0 and s < mult < s + M:
                        c.expect.append(("s_chunk_%d" % mult, b, s, "len_pos_k", (M, q, 0)))
                break
        # a piece start in the middle of a copy: two runs of M / 2
        got = plant_on("piece_start_inside", want=lambda q: ("len_pos_k", (M // 2, q, 0)), solo=True)
        if got:
            starts.add(got[2] + M // 2)
            c.expect.append(("piece_start_inside", got[0], got[1] + M // 2, "len_pos_k", (M // 2, got[2] + M // 2, 0)))
        # two equal copies: the lower position wins
        got = plant_on("equal_copies_lower_p")
        if got:
            b, s, q = got
            q2 = find(M, q + M + 2)
            put(q2, rows[b][s:s + M], int(rows[b][s + M]) if s + M < c.lens[b] else None)
        # the edges of every diagonal block: last diagonal of block j - 1, first of block j
        nblocks = -(-(n + L - 1) // KERNEL_BLOCK)
        missed = 0
        for j in range(1, nblocks):
            d0 = j * KERNEL_BLOCK - (L - 1)
            for feature, d in (("block_edge_last", d0 - 1), ("block_edge_first", d0)):
                if plant_on(feature, d=d) is None:
                    missed += 1
        c.edges_missed, c.nblocks = missed, nblocks
    # a start may not fall inside a plant it was not meant for
    keep = [s for s in sorted(starts) if s == 0 or not used[s] or any(e[0] == "piece_start_inside" and e[4][1] == s for e in c.expect)]
    c.starts = np.asarray(keep, np.int64)
    c.corpus = corpus.astype(np.uint16)
    c.rows = [r.astype(np.int32) for r in rows]
    if any(l < L for l in c.lens):
        c.features.add("pad_tail")
    if n == 1:
        c.features.add("n_1")
    if B > 1 and L <= KERNEL_SCHUNK:
        c.features.add("one_chunk_rows_share")
    if L > KERNEL_SCHUNK:
        c.features.add("many_chunks")
    return c


def case(name):
    if name not in _cases:
        if name == "n1":                     # one id against itself
            c = build(*GRID[0])
            c.corpus = np.asarray([288], np.uint16)
            c.rows = [np.asarray([288], np.int32)]
            c.expect.append(("copy_at_p0", 0, 0, "len_pos_k", (1, 0, 0)))
            _cases[name] = c
        else:
            _cases[name] = build(*[g for g in GRID if g[0] == name][0])
    return _cases[name]


def reference(name):
    """(len, pos, k) [B, ld] of a case by the host restatement, computed once and shared; read-only."""
    if name not in _refs:
        c = case(name)
        ref = novelty.match_rows(c.corpus, c.starts, c.rows, c.layout, c.min_match, c.N, c.velocity, ld=c.ld)
        for a in ref:
            a.setflags(write=False)
        _refs[name] = ref
    return _refs[name]


def met(c, ref, e):
    """Does the table `ref` meet the recorded expectation e of case c?"""
    ln, ps, ks = ref
    _, b, s, kind, v = e
    got = (int(ln[b, s]), int(ps[b, s]), int(ks[b, s]))
    if kind == "pos_k":
        return got[0] >= c.plant and got[1:] == tuple(v)
    if kind == "len":
        return got[0] == v
    return got == tuple(v)


def covered(names=NAMES):
    """The features of ALL_FEATURES that the cases hold: a planted feature counts when EVERY expectation recorded under its name, in
    every case that planted it, is what the host restatement reports."""
    ok, bad = set(), set()
    for name in names:
        c, ref = case(name), reference(name)
        ok |= c.features
        for e in c.expect:
            (ok if met(c, ref, e) else bad).add(e[0])
        if getattr(c, "nblocks", 0) > 1 and c.edges_missed <= 2 and name in ("n5000_fold", "n70000"):
            ok.add("every_block_edge")             # (the last block's edges may lie past n - PLANT)
    if {"block_edge_last", "block_edge_first"} & bad:
        bad.add("every_block_edge")
    return ok - bad


# ------------------------------------------------------------------------------------------------ the comparison
POISON_POS, POISON_K = -(1 << 62), 0x7A7A7A7A             # what the tests pre-fill pos and k with: -1 (0xFF..) is a legal value of both


def compare(name, got_len, got_pos, got_k):
    """Raises AssertionError unless the three [B, ld] arrays are the host restatement's, padded tail included."""
    c = case(name)
    ln, ps, ks = reference(name)
    for what, got, ref in (("len", got_len, ln), ("pos", got_pos, ps), ("k", got_k, ks)):
        got = np.asarray(got)
        assert got.shape == ref.shape, (name, what, got.shape, ref.shape)
        bad = np.argwhere(got != ref)
        assert bad.size == 0, "%s: %s differs at (row, s) %s: got %s, reference %s (%d of %d elements; row lengths %s)" % (
            name, what, bad[0].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])], len(bad), ref.size, c.lens)
