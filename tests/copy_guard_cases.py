"""Corpora, histories and the slow reference shared by the copy-guard tests (tests/test_copy_guard_host.py on the CPU,
tests/test_gpu_copy_guard_kernel.py on the device).

`brute_bans` is the contract of include/composer_hip.h ("copy guard") as a triple loop over (p, k, j) and a loop over the columns, one
token comparison at a time; its flags switch on the mistakes the tests must be able to see.  The cases draw corpus and histories from
novelty_cases' small alphabet, so chance matches are plentiful at M = 1 and 2, and PLANT windows of the corpus into the histories --
transposed and with other velocities where the case allows it -- at the positions a scan can get wrong: the window that starts at 0,
the one whose continuation is c[n - 1], a piece start exactly at p - M (still a ban) and one inside the window (no ban)."""
import numpy as np

import novelty_cases as nc
from composer_amd import novelty

LAYOUT, VELOCITY, V = nc.LAYOUT, nc.VELOCITY, 390
LD = 71                                                    # a leading dimension that is no multiple of anything

#        name          n     M   B   N  fold
GRID = (("n1",         1,    1,  1,  0, False),
        ("n7_m1",      7,    1,  3,  2, True),
        ("n7_m2",      7,    2,  1,  0, True),
        ("n7_m16",     7,    16, 3,  0, False),
        ("n257_m1",    257,  1,  16, 0, False),
        ("n257_m2",    257,  2,  3,  2, True),
        ("n257_m16",   257,  16, 16, 2, False),
        ("n257_m64",   257,  64, 3,  0, True),
        ("n4099_m1",   4099, 1,  3,  2, False),
        ("n4099_m2",   4099, 2,  16, 0, True),
        ("n4099_m16",  4099, 16, 3,  0, False),
        ("n4099_m16t", 4099, 16, 1,  2, True),
        ("n4099_m64",  4099, 64, 16, 2, True))
NAMES = tuple(g[0] for g in GRID)
SMALL = tuple(g[0] for g in GRID if g[1] <= 257) + ("n4099_m16",)      # cheap enough for the triple loop

_cases, _refs = {}, {}


def tok_under(x, k, layout, vel, clip=False):
    """A history token (or a column) under transposition k -> the corpus code it equals, or None (equals nothing)."""
    x = int(x)
    if x < 0 or x >= 65535:
        return None
    if vel and vel[0] <= x < vel[0] + vel[1]:
        return vel[0]
    for base in (int(layout.note_on0), int(layout.note_off0)):
        if base <= x < base + 128:
            q = x - base + k
            if clip:
                q = min(max(q, 0), 127)
            return base + q if 0 <= q <= 127 else None
    return x


def brute_bans(corpus, starts, history, V, layout, M, N=0, vel=None, ignore_starts=False, ts_exempt=True, clip=False, wrap=False):
    """The contract, one comparison at a time.  The flags are MISTAKES: ignore_starts forgets the piece starts, ts_exempt=False bans
    TIME_SHIFT continuations too, clip clips a moved pitch instead of "equals nothing", wrap lets the window start before position 0."""
    c = [int(v) for v in corpus]
    n, t = len(c), len(history)
    st = {0} if starts is None else {int(s) for s in starts}
    cf = [vel[0] if vel and vel[0] <= v < vel[0] + vel[1] else v for v in c]
    bans = np.zeros(V, bool)
    if t < M:
        return bans
    ts0, tsn = int(layout.time_shift0), int(layout.time_shift_n)
    for p in range(0 if wrap else M, n):
        if not ignore_starts and any(q in st for q in range(p - M + 1, p + 1)):
            continue
        for k in range(-N, N + 1):
            if all(tok_under(history[t - M + j], k, layout, vel, clip) == cf[p - M + j] for j in range(M)):
                for v in range(V):
                    if ts_exempt and ts0 <= v < ts0 + tsn:
                        continue
                    if tok_under(v, k, layout, vel, clip) == cf[p]:
                        bans[v] = True
    return bans


class Case:
    pass


def build(name, n, M, B, N, fold):
    rng = np.random.default_rng(sum(map(ord, name)) + 11)
    c = Case()
    c.name, c.n, c.M, c.B, c.N, c.ld = name, n, M, B, N, LD
    c.layout, c.velocity = LAYOUT, (VELOCITY if fold else None)
    notes = [LAYOUT.note_on0 + p for p in nc.PITCHES] + [LAYOUT.note_off0 + p for p in nc.PITCHES]
    alphabet = nc.ALPHABET + (256 + 5, 256 + 30)

    def draw(k):
        return np.where(rng.random(k) < 0.7, rng.choice(alphabet, size=k), rng.choice(notes, size=k)).astype(np.int64)
    corpus = draw(n)
    if n > M + 8:                                              # a stretch without a note token, followed by one: 2 N + 1 pitches
        q = int(rng.integers(M, n - M - 1)) if n > 2 * M + 2 else M
        corpus[q - M:q] = rng.choice(nc.ALPHABET, size=M)
        corpus[q] = LAYOUT.note_on0 + 60
        c.no_note_p = q
    starts = {0}
    if n >= 257:
        starts |= {int(v) for v in rng.integers(1, n, size=3) if v > M}       # (not inside the first row's plant)
    if n > M and LAYOUT.time_shift0 <= corpus[M] < LAYOUT.time_shift0 + LAYOUT.time_shift_n:
        corpus[M] = 389                                        # ... whose continuation is no TIME_SHIFT: every case bans something
    # row lengths: the first row full, then one shorter than M, an empty one, the rest anything that holds a window
    lens = [LD]
    if B >= 3:
        lens += [M - 1, 0]
    while len(lens) < B:
        lens.append(int(rng.integers(M, LD + 1)) if M <= LD else LD)
    c.lens = lens[:B]
    hist = np.full((B, LD), -1, np.int64)
    c.plants = []                                              # (row, p, k)
    live = [b for b in range(B) if c.lens[b] >= M]
    for i, b in enumerate(live):
        L = c.lens[b]
        hist[b, :L] = draw(L)
        if n <= M:
            continue
        if i == 0:
            p = M                                              # the window that starts at 0
        elif i == 1:
            p = n - 1                                          # the continuation is the last id of the stream
        elif i == 2 and getattr(c, "no_note_p", None):
            p = c.no_note_p
        elif i == 5 and N >= 1 and M >= 2 and n > 3 * M:
            # a trap for clipping: the history under k = +1 is pitch 127, then "128" -- equals nothing; clipped, it is the corpus
            p = int(rng.integers(M, n - 1))
            corpus[p - M:p] = LAYOUT.note_on0 + 127
            corpus[p] = LAYOUT.note_on0 + 60
            hist[b, L - M:L] = [LAYOUT.note_on0 + 126 + (j & 1) for j in range(M)]
            starts -= set(range(p - M + 1, p + 1))
            continue
        elif rng.random() < 0.25:
            continue                                           # a row with chance matches only
        else:
            p = int(rng.integers(M, n))
        k = int(rng.integers(-N, N + 1))
        w = corpus[p - M:p].copy()
        moved = novelty.map_query(w, -k, LAYOUT, (0, 0))       # the history holds pitch - k, so that under k it is the corpus
        if (moved < 0).any():
            k, moved = 0, w
        if fold:
            vel = (moved >= VELOCITY[0]) & (moved < VELOCITY[0] + VELOCITY[1])
            moved = np.where(vel, rng.integers(VELOCITY[0], VELOCITY[0] + VELOCITY[1], size=M), moved)
        hist[b, L - M:L] = moved
        c.plants.append((b, p, k))
        if i == 3 and p - M >= 1:
            starts.add(p - M)                                  # a start exactly in front of the window: still a ban
        if i == 4 and M >= 2:
            starts.add(p - M + 1 + int(rng.integers(0, M)))    # a start inside p - M + 1 .. p: no ban from this position
    c.hist = hist.astype(np.int32)
    c.corpus = corpus.astype(np.uint16)
    c.starts = np.asarray(sorted(s for s in starts if s < n), np.int64)
    # a static vector with bits the scan must keep: a few columns, a TIME_SHIFT among them, and a bit at or above V
    words = np.zeros((V + 31) // 32, np.uint32)
    for v in list(rng.integers(0, V, size=12)) + [int(LAYOUT.time_shift0) + 3, V + 5]:
        words[int(v) >> 5] |= np.uint32(1 << (int(v) & 31))
    c.static = words
    return c


def case(name):
    if name not in _cases:
        _cases[name] = build(*[g for g in GRID if g[0] == name][0])
    return _cases[name]


def to_words(bans, static=None):
    w = np.zeros((len(bans) + 31) // 32, np.uint32)
    for v in np.flatnonzero(bans):
        w[v >> 5] |= np.uint32(1 << (int(v) & 31))
    return w if static is None else w | static


def reference(name):
    """(bans bool [B, V], words uint32 [B, nw] = static | bans, counts int64 [B]) of a case by the host restatement, computed once and
    shared; read-only."""
    if name not in _refs:
        c = case(name)
        bans = np.stack([novelty.copy_bans(c.corpus, c.starts, c.hist[b, :c.lens[b]], V, c.layout, c.M, c.N, c.velocity)
                         for b in range(c.B)])
        words = np.stack([to_words(bans[b], c.static) for b in range(c.B)])
        sbits = np.array([(c.static[v >> 5] >> np.uint32(v & 31)) & 1 for v in range(V)], bool)
        counts = (bans & ~sbits).sum(1).astype(np.int64)
        for a in (bans, words, counts):
            a.setflags(write=False)
        _refs[name] = (bans, words, counts)
    return _refs[name]
