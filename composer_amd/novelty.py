"""Novelty check: the longest training-set match of every event of a sample (include/composer_hip.h, "novelty check").

`match_table` restates the contract on the host, vectorised over the corpus position p with one numpy pass per (s, k); the device
(composer_amd/csrc/novelty.hip) computes the same three integer arrays bit for bit.  `Corpus` owns a context and a cmp_dataset (it
needs no model) and turns the arrays into `NoveltyReport`s: the longest match and where it lies, the share of the query covered by
reported matches, the longest match's duration.

Known limit: a time-stretched copy re-chunks its TIME_SHIFT runs and is not found.

Copy guard (include/composer_hip.h, "copy guard"; the scan: composer_amd/csrc/copyguard.hip).  With a guard attached to a decode
chain no draw extends a verbatim match of the row's history h = prompt ++ ids so far (t = len(h)) with the corpus past max_copy = M
events.  `copy_bans` restates the ban set of one draw: column v is banned iff v is not a TIME_SHIFT id, t >= M, and there are a corpus
position p, M <= p < n, and a k in [-N, N] such that h[t - M + j] under k equals c[p - M + j] for j = 0 .. M - 1, v under k equals
c[p], and none of p - M + 1 .. p is a piece start.  Token equality under k is `map_query`'s (a moved pitch that leaves 0 .. 127
equals nothing, folded velocities equal each other, corpus tokens are never transposed).  TIME_SHIFT ids are exempt: no dynamic rule
of the decode ever bans one, the time budget relies on it.  The bans are ORed with the chain's static vector and the grammar's and
budget's bans in PLAY and ignored in ENDING and DONE.  So in prompt ++ ids every drawn event that is the (M + 1)-th or a later event
of a match is a TIME_SHIFT; with a prompt of at most M events every match of more than M events consists of TIME_SHIFT events only
from its (M + 1)-th event on."""
import ctypes as C

import numpy as np

MAX_B, MAX_LD, MAX_TRANSPOSE = 256, 32768, 24
MAX_N = 1 << 40
MAX_COPY = 64


def rank_order(transpose):
    """The transpositions in the order of the contract: 0, -1, +1, -2, +2 ... (smaller |k| first, negative before positive)."""
    out = [0]
    for a in range(1, int(transpose) + 1):
        out += [-a, a]
    return out


def check_options(min_match, transpose, velocity_range, layout):
    """Every refusal of the options that the library states, as a ValueError -> (min_match, N, (velocity0, velocity_n))."""
    min_match, transpose = int(min_match), int(transpose)
    if min_match < 1:
        raise ValueError('min_match=%d must be >= 1' % min_match)
    if not 0 <= transpose <= MAX_TRANSPOSE:
        raise ValueError('transpose=%d outside [0, %d]' % (transpose, MAX_TRANSPOSE))
    if transpose and layout is None:
        raise ValueError('transpose=%d needs the event layout (which ids are notes)' % transpose)
    v0, vn = (0, 0) if velocity_range is None else (int(velocity_range[0]), int(velocity_range[1]))
    if vn < 0 or v0 < 0 or v0 + vn > 65536:
        raise ValueError('velocity ids [%d, %d) outside [0, 65536)' % (v0, v0 + vn))
    if layout is not None:
        on0, off0 = int(layout.note_on0), int(layout.note_off0)
        for name, lo in (('note_on', on0), ('note_off', off0)):
            if lo < 0 or lo + 128 > 65536:
                raise ValueError('%s ids [%d, %d) outside [0, 65536)' % (name, lo, lo + 128))
            if vn and not (v0 + vn <= lo or lo + 128 <= v0):
                raise ValueError('the velocity ids [%d, %d) overlap the %s ids [%d, %d)' % (v0, v0 + vn, name, lo, lo + 128))
        if not (on0 + 128 <= off0 or off0 + 128 <= on0):
            raise ValueError('the note_on ids [%d, %d) overlap the note_off ids [%d, %d)' % (on0, on0 + 128, off0, off0 + 128))
    return min_match, transpose, (v0, vn)


def check_starts(starts, n):
    """None: one piece.  Sorted (non-decreasing), inside [0, n), the first of them 0 -> int64 array."""
    if n >= MAX_N:
        raise ValueError('n=%d ids: the corpus must hold fewer than 2^40' % n)
    if starts is None:
        return np.zeros(1, np.int64)
    st = np.asarray(starts, np.int64).reshape(-1)
    if len(st) == 0 or st[0] != 0:
        raise ValueError('piece starts must begin with 0')
    if (st < 0).any() or (st >= n).any():
        raise ValueError('a piece start lies outside [0, %d)' % n)
    if (np.diff(st) < 0).any():
        raise ValueError('piece starts are not sorted')
    return st


def check_query(x):
    x = np.asarray(x, np.int64).reshape(-1)
    if len(x) < 1 or len(x) > MAX_LD:
        raise ValueError('a query holds %d ids: 1 .. %d are allowed' % (len(x), MAX_LD))
    if (x < 0).any() or (x >= 65535).any():
        raise ValueError('a query id lies outside [0, 65535)')
    return x


def map_query(x, k, layout, velocity):
    """The query under transposition k: velocity ids folded to the first of the range, a note of pitch p moved to p + k, or -1 (equals
    nothing) when that leaves 0 .. 127 -- never clipped."""
    v0, vn = velocity
    x = np.where((x >= v0) & (x < v0 + vn), v0, x)
    if layout is None or k == 0:
        return x
    out = x.copy()
    for base in (int(layout.note_on0), int(layout.note_off0)):
        note = (x >= base) & (x < base + 128)
        moved = x + k
        out[note] = np.where((moved[note] >= base) & (moved[note] < base + 128), moved[note], -1)
    return out


def match_table(corpus, starts, x, layout=None, min_match=1, transpose=0, velocity_range=None):
    """(len int32 [L], pos int64 [L], k int32 [L]) of ONE query x against the corpus: the contract of include/composer_hip.h restated.
    m(s, ., k) is built from m(s + 1, ., k) for s = L - 1 down to 0, all p at once; k runs in rank order and a later k replaces the
    best only with a strictly longer run, argmax takes the smallest p: the total order of the contract."""
    min_match, N, vel = check_options(min_match, transpose, velocity_range, layout)
    c = np.asarray(corpus).astype(np.int64).reshape(-1)
    n = len(c)
    if n < 1:
        raise ValueError('the corpus is empty')
    st = check_starts(starts, n)
    x = check_query(x)
    L = len(x)
    cf = np.where((c >= vel[0]) & (c < vel[0] + vel[1]), vel[0], c).astype(np.int32)
    # go_on[p]: a run at p may continue into p + 1 (inside the stream, not a piece start)
    go_on = np.ones(n, np.int32)
    go_on[n - 1] = 0
    nxt = st[st >= 1] - 1
    go_on[nxt] = 0
    best_len, best_pos, best_k = np.zeros(L, np.int32), np.full(L, -1, np.int64), np.zeros(L, np.int32)
    prev, cur = np.zeros(n + 1, np.int32), np.zeros(n, np.int32)
    for k in rank_order(N):
        xk = map_query(x, k, layout, vel).astype(np.int32)
        prev[:] = 0
        for s in range(L - 1, -1, -1):
            np.multiply(prev[1:], go_on, out=cur)
            cur += 1
            cur *= (cf == xk[s])
            m = int(cur.max())
            if m > best_len[s]:
                best_len[s], best_pos[s], best_k[s] = m, int(cur.argmax()), k
            prev[:n] = cur
    low = best_len < min_match
    best_len[low], best_pos[low], best_k[low] = 0, -1, 0
    return best_len, best_pos, best_k


def match_rows(corpus, starts, rows, layout=None, min_match=1, transpose=0, velocity_range=None, ld=None):
    """match_table on ragged rows -> padded [B, ld] arrays as cmp_novelty writes them: (0, -1, 0) behind a row's length."""
    B = len(rows)
    ld = max(len(r) for r in rows) if ld is None else int(ld)
    ln, ps, ks = np.zeros((B, ld), np.int32), np.full((B, ld), -1, np.int64), np.zeros((B, ld), np.int32)
    for b, r in enumerate(rows):
        ln[b, :len(r)], ps[b, :len(r)], ks[b, :len(r)] = match_table(corpus, starts, r, layout, min_match, transpose, velocity_range)
    return ln, ps, ks


def coverage_of(length):
    """The share of query positions inside some reported interval [s, s + len(s))."""
    length = np.asarray(length, np.int64)
    L = len(length)
    if L == 0:
        return 0.0
    edge = np.zeros(L + 1, np.int64)
    s = np.flatnonzero(length > 0)
    np.add.at(edge, s, 1)
    np.add.at(edge, np.minimum(s + length[s], L), -1)
    return float((np.cumsum(edge[:L]) > 0).sum()) / L


def check_guard_options(max_copy, transpose, velocity_range, layout):
    """Every refusal of a copy guard's options that the library states, as a ValueError -> (M, N, (velocity0, velocity_n))."""
    max_copy, transpose = int(max_copy), int(transpose)
    if not 1 <= max_copy <= MAX_COPY:
        raise ValueError('max_copy=%d outside [1, %d]' % (max_copy, MAX_COPY))
    if not 0 <= transpose <= MAX_TRANSPOSE:
        raise ValueError('transpose=%d outside [0, %d]' % (transpose, MAX_TRANSPOSE))
    if layout is None:
        raise ValueError('a copy guard needs the event layout (which ids are TIME_SHIFT and notes)')
    _, N, vel = check_options(1, transpose, velocity_range, layout)
    return max_copy, N, vel


def copy_bans(corpus, starts, history, V, layout, max_copy, transpose=0, velocity_range=None):
    """bool [V]: the columns the copy rule bans for a row whose history is `history` (the contract at the top of this file), all
    corpus positions at once per k."""
    M, N, vel = check_guard_options(max_copy, transpose, velocity_range, layout)
    c = np.asarray(corpus).astype(np.int64).reshape(-1)
    n = len(c)
    if n < 1:
        raise ValueError('the corpus is empty')
    st = check_starts(starts, n)
    h = np.asarray(history, np.int64).reshape(-1)
    V = int(V)
    bans = np.zeros(V, bool)
    if len(h) < M or n <= M:
        return bans
    w = h[len(h) - M:]
    w = np.where((w < 0) | (w >= 65535), -1, w)                   # such an id equals nothing
    cols = np.arange(V, dtype=np.int64)
    cols = np.where(cols >= 65535, -1, cols)
    cf = np.where((c >= vel[0]) & (c < vel[0] + vel[1]), vel[0], c)
    is_start = np.zeros(n + 1, np.int64)
    is_start[st] = 1
    cs = np.cumsum(is_start)
    p = np.arange(M, n)
    free = (cs[p] - cs[p - M]) == 0                               # no start among p - M + 1 .. p
    for k in range(-N, N + 1):
        wk = map_query(w, k, layout, vel)
        hit = free.copy()
        for j in range(M):
            hit &= cf[j:j + n - M] == wk[j]                      # c[p - M + j] for p = M .. n - 1
        if not hit.any():
            continue
        targets = np.unique(cf[M:][hit])
        vk = map_query(cols, k, layout, vel)
        bans |= np.isin(vk, targets) & (vk >= 0)
    ts0, tsn = int(layout.time_shift0), int(layout.time_shift_n)
    bans[max(ts0, 0):max(ts0 + tsn, 0)] = False
    return bans


class CopyGuard:
    """What `Transformer.generate(..., copy_guard=)` takes: a corpus and the options of the rule (`Corpus.guard` builds it)."""

    def __init__(self, corpus, max_copy, transpose=0, ignore_velocity=False):
        if ignore_velocity and corpus.velocity_range is None:
            raise ValueError('ignore_velocity needs the corpus\'s velocity_range')
        self.corpus = corpus
        self.velocity_range = corpus.velocity_range if ignore_velocity else None
        self.max_copy, self.transpose, self._vel = check_guard_options(max_copy, transpose, self.velocity_range, corpus.layout)

    def attach_args(self):
        """(cmp_dataset handle, cmp_copy_guard_opts) for cmp_decode_copy_guard; opens the corpus's dataset."""
        from . import _lib
        self.corpus._open()
        return self.corpus._ds, _lib.CopyGuardOpts(self.max_copy, self.transpose, self._vel[0], self._vel[1])

    def bans(self, history, V):
        """`copy_bans` of one history under this guard (host)."""
        return copy_bans(self.corpus.ids, self.corpus.starts, history, V, self.corpus.layout, self.max_copy, self.transpose,
                         self.velocity_range)


class NoveltyReport:
    """The arrays of one query and what they say.  longest: (length, query position, file name, offset in that file, k) of the longest
    match (the first of equals; (0, -1, None, -1, 0) when nothing reached min_match); coverage: `coverage_of`; longest_seconds: the
    duration of the longest match, from the TIME_SHIFT ids of the query inside it."""

    def __init__(self, length, pos, k, ids=None, starts=None, names=None, layout=None, time_step_ms=10):
        self.len = np.asarray(length, np.int32)
        self.pos = np.asarray(pos, np.int64)
        self.k = np.asarray(k, np.int32)
        self.events = len(self.len)
        self.coverage = coverage_of(self.len)
        self.longest = (0, -1, None, -1, 0)
        self.longest_seconds = 0.0
        if self.events and int(self.len.max()) > 0:
            s = int(self.len.argmax())
            m, p = int(self.len[s]), int(self.pos[s])
            st = np.zeros(1, np.int64) if starts is None else np.asarray(starts, np.int64)
            piece = int(np.searchsorted(st, p, side='right')) - 1
            name = names[piece] if names is not None else None
            self.longest = (m, s, name, p - int(st[piece]), int(self.k[s]))
            if ids is not None and layout is not None:
                seg = np.asarray(ids, np.int64)[s:s + m] - int(layout.time_shift0)
                steps = int((seg[(seg >= 0) & (seg < int(layout.time_shift_n))] + 1).sum())
                self.longest_seconds = steps * time_step_ms / 1000.0

    def to_dict(self):
        m, s, name, off, k = self.longest
        return {'events': self.events, 'coverage': self.coverage, 'longest_seconds': self.longest_seconds,
                'longest': {'length': m, 'position': s, 'file': name, 'offset': off, 'transpose': k},
                'len': self.len.tolist(), 'pos': self.pos.tolist(), 'k': self.k.tolist()}

    def line(self):
        """What the CLI prints behind the query's name."""
        m, s, name, off, k = self.longest
        if m == 0:
            return 'events {} longest 0 (0.000 s) coverage {:.6f}'.format(self.events, self.coverage)
        return 'events {} longest {} ({:.3f} s) at {} in {} offset {} transpose {:+d} coverage {:.6f}'.format(
            self.events, m, self.longest_seconds, s, name, off, k, self.coverage)


class Corpus:
    """A training id stream in HBM to match samples against.  ids: uint16 event ids; starts: piece offsets (None: one piece); names:
    one per start; layout: composer_amd.grammar.EventGrammar (needed to transpose and for durations); velocity_range: (first id, count)
    of the VELOCITY ids (needed for ignore_velocity).  Everything that can be refused is refused on the host; the context and the
    cmp_dataset are created at the first `match` that passes."""

    def __init__(self, ids, starts=None, names=None, layout=None, velocity_range=None, time_step_ms=10, device=0):
        ids = np.asarray(ids)
        if ids.ndim != 1 or len(ids) < 2:
            raise ValueError('the corpus needs at least 2 ids')
        if ids.min() < 0 or ids.max() > 65535:
            raise ValueError('event ids must fit uint16')
        self.ids = np.ascontiguousarray(ids, dtype=np.uint16)
        self.starts = check_starts(starts, len(self.ids))
        self.names = list(names) if names is not None else ['piece %d' % i for i in range(len(self.starts))]
        if len(self.names) != len(self.starts):
            raise ValueError('%d names for %d piece starts' % (len(self.names), len(self.starts)))
        self.layout, self.velocity_range, self.time_step_ms, self.device = layout, velocity_range, time_step_ms, int(device)
        check_options(1, 0, velocity_range, layout)
        self._lib = self._ctx = self._ds = None
        self.generation = 0                      # counts the datasets opened: a model re-attaches a guard whose corpus was reopened

    def _open(self):
        if self._ds is not None:
            return
        from . import _lib
        self._lib = _lib.load()
        _lib.require_gpu()
        ctx, h = C.c_void_p(), C.c_void_p()
        _lib.check(self._lib.cmp_ctx_create(self.device, C.byref(ctx)), 'cmp_ctx_create')
        self._ctx = ctx
        layout = self.layout
        if layout is not None and not isinstance(layout, _lib.EventGrammar):
            layout = layout.to_c()
        _lib.check(self._lib.cmp_dataset_create(ctx, self.ids.ctypes.data_as(C.c_void_p), len(self.ids),
                                                C.byref(layout) if layout is not None else None, C.byref(h)), 'cmp_dataset_create')
        self._ds = h
        self.generation += 1
        _lib.check(self._lib.cmp_dataset_set_pieces(h, self.starts.ctypes.data_as(C.c_void_p), len(self.starts)), 'cmp_dataset_set_pieces')

    def close(self):
        if self._ds is not None:
            self._lib.cmp_dataset_destroy(self._ds)
            self._ds = None
        if self._ctx is not None:
            self._lib.cmp_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def options(self, min_match=16, transpose=0, ignore_velocity=False):
        """-> (min_match, N, (velocity0, velocity_n)) as the library gets them; a ValueError for what it would refuse."""
        if ignore_velocity and self.velocity_range is None:
            raise ValueError('ignore_velocity needs the corpus\'s velocity_range')
        return check_options(min_match, transpose, self.velocity_range if ignore_velocity else None, self.layout)

    def guard(self, max_copy, transpose=0, ignore_velocity=False):
        """The `CopyGuard` to pass as `Transformer.generate(..., copy_guard=)` / `generate_batch(..., copy_guard=)`: decode never
        extends a match with this corpus past max_copy events.  Keep the corpus open while a model holds the guard."""
        return CopyGuard(self, max_copy, transpose, ignore_velocity)

    def match_arrays(self, sequences, min_match=16, transpose=0, ignore_velocity=False):
        """The padded [B, ld] arrays of cmp_novelty for up to 256 ragged sequences, one call."""
        from . import _lib
        min_match, N, vel = self.options(min_match, transpose, ignore_velocity)
        rows = [check_query(s) for s in sequences]
        if not 1 <= len(rows) <= MAX_B:
            raise ValueError('%d sequences in one call: 1 .. %d are allowed' % (len(rows), MAX_B))
        self._open()
        B, ld = len(rows), max(len(r) for r in rows)
        x, lens = np.zeros((B, ld), np.int32), np.asarray([len(r) for r in rows], np.int32)
        for b, r in enumerate(rows):
            x[b, :len(r)] = r
        ln, ps, ks = np.empty((B, ld), np.int32), np.empty((B, ld), np.int64), np.empty((B, ld), np.int32)
        opts = _lib.NoveltyOpts(min_match, N, vel[0], vel[1])
        P = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.cmp_novelty(self._ds, P(x), P(lens), B, ld, C.byref(opts), P(ln), P(ps), P(ks)), 'cmp_novelty')
        return ln, ps, ks, lens

    def report(self, ids, length, pos, k):
        return NoveltyReport(length, pos, k, ids, self.starts, self.names, self.layout, self.time_step_ms)

    def match(self, sequences, min_match=16, transpose=0, ignore_velocity=False):
        """One NoveltyReport per sequence (ragged lists of event ids); 256 sequences per device call."""
        self.options(min_match, transpose, ignore_velocity)
        seqs = [check_query(s) for s in sequences]
        out = []
        for i in range(0, len(seqs), MAX_B):
            part = seqs[i:i + MAX_B]
            ln, ps, ks, lens = self.match_arrays(part, min_match, transpose, ignore_velocity)
            out += [self.report(s, ln[b, :lens[b]], ps[b, :lens[b]], ks[b, :lens[b]]) for b, s in enumerate(part)]
        return out

    def match_host(self, sequences, min_match=16, transpose=0, ignore_velocity=False):
        """`match` by the host restatement (small inputs: tests, machines without a device)."""
        min_match, N, vel = self.options(min_match, transpose, ignore_velocity)
        return [self.report(s, *match_table(self.ids, self.starts, s, self.layout, min_match, N, vel if vel[1] else None))
                for s in sequences]
