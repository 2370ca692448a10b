"""Train-time augmentation of event-id rows, restated on the host: transpose, time stretch, crop.

This is the contract of the device path (include/composer_hip.h, "device dataset"; composer_amd/csrc/batch.hip) in plain integer
code, and the oracle of its tests: every comparison with the device is bitwise equality.

  Layout   any object with note_on0, note_off0 (128 consecutive ids each, id - base = pitch), time_shift0 and time_shift_n = M
           (id time_shift0 + j counts j + 1 steps) -- composer_amd.grammar.EventGrammar is one.  Never hard-coded.
  Row plan (offset, transpose k, stretch f), f in 1/1024ths: 1024 is the identity, 512 <= f <= 1536.
  Span     src = ids[offset : offset + S], S = min(2 (W + 1), n - offset), 0 <= offset <= n - (W + 1).
  Transpose a NOTE_ON / NOTE_OFF id of pitch p becomes pitch clip(p + k, 0, 127) (the reference's rule, sequence.py:379, per token).
  Stretch  R(t) = (t f + 512) >> 10.  Every maximal run of consecutive TIME_SHIFT ids, r steps in all, starting at unstretched time
           t, becomes d = R(t + r) - R(t) steps: d // M ids of M steps, then one of d % M steps if that is not zero (notes.py:116-120).
           Cumulative rounding: the emitted steps of a span sum to R(its total).
  Output   out = the first W + 1 emitted ids, x = out[:W], y = out[1:].  f = 1024 copies src[:W + 1] (transposed) without walking:
           re-chunking is not the identity on a non-canonical run ([30, 50] would become [80]).  A span that emits fewer than
           W + 1 ids falls back to the f = 1024 row, still transposed, with the fallback bit in its status.
  Status   (emitted ids clipped to W + 1, flags).

The stretch works on tokens: it is not bit-equal to the reference's note-level `time_stretch` followed by re-encoding (which
re-quantises every note's start and end on its own), only the same musical operation on the time axis."""
import numpy as np

STRETCH_ONE = 1024
STRETCH_MIN, STRETCH_MAX = 512, 1536
TRANSPOSE_MAX = 127
FALLBACK = 1
PLAN_DTYPE = np.dtype([('offset', '<i8'), ('transpose', '<i4'), ('stretch_q10', '<i4')])      # cmp_batch_row


def R(t, f):
    """Stretched time of the unstretched time t (Python integers: 64-bit and beyond)."""
    return (int(t) * int(f) + 512) >> 10


def _check_f(f):
    f = int(f)
    if not STRETCH_MIN <= f <= STRETCH_MAX:
        raise ValueError('stretch %d/1024 outside [%d, %d]' % (f, STRETCH_MIN, STRETCH_MAX))
    return f


def transpose_tokens(ids, layout, k):
    """ids (any integer array) with every NOTE_ON / NOTE_OFF pitch moved by k and clipped to [0, 127]; int64."""
    out = np.asarray(ids).astype(np.int64)
    k = int(k)
    if abs(k) > TRANSPOSE_MAX:
        raise ValueError('transpose %d outside [-%d, %d]' % (k, TRANSPOSE_MAX, TRANSPOSE_MAX))
    if k == 0:
        return out
    for base in (int(layout.note_on0), int(layout.note_off0)):
        sel = (out >= base) & (out < base + 128)
        out[sel] = base + np.clip(out[sel] - base + k, 0, 127)
    return out


def stretch_tokens(src, layout, f):
    """The whole span re-timed by f / 1024: every id the walk emits, int64.  (f = 1024 walks too: the bypass is build_row's.)"""
    f = _check_f(f)
    ts0, M = int(layout.time_shift0), int(layout.time_shift_n)
    out, t, i = [], 0, 0
    src = [int(v) for v in np.asarray(src).reshape(-1)]
    n = len(src)
    while i < n:
        v = src[i]
        if not ts0 <= v < ts0 + M:
            out.append(v)
            i += 1
            continue
        r = 0
        while i < n and ts0 <= src[i] < ts0 + M:
            r += src[i] - ts0 + 1
            i += 1
        d = R(t + r, f) - R(t, f)
        out += [ts0 + M - 1] * (d // M)
        if d % M:
            out.append(ts0 + d % M - 1)
        t += r
    return np.asarray(out, np.int64)


def build_row(ids, layout, offset, k, f, W):
    """-> (x int32 [W], y int32 [W], (emitted ids clipped to W + 1, flags))."""
    n, W, offset, f = len(ids), int(W), int(offset), _check_f(f)
    if W < 1 or n < W + 1:
        raise ValueError('a row of W=%d needs %d ids, the stream holds %d' % (W, W + 1, n))
    if not 0 <= offset <= n - (W + 1):
        raise ValueError('offset %d outside [0, %d]' % (offset, n - (W + 1)))
    if layout is None and (int(k) != 0 or f != STRETCH_ONE):
        raise ValueError('a plan that transposes or stretches needs a layout')
    src = np.asarray(ids[offset:offset + min(2 * (W + 1), n - offset)]).astype(np.int64)
    count, flags, out = W + 1, 0, None
    if f != STRETCH_ONE:
        em = stretch_tokens(src, layout, f)
        count = min(len(em), W + 1)
        if len(em) >= W + 1:
            out = em[:W + 1]
        else:
            flags = FALLBACK
    if out is None:
        out = src[:W + 1]
    out = transpose_tokens(out, layout, k).astype(np.int32)
    return out[:W].copy(), out[1:].copy(), (count, flags)


def as_plan(plan):
    """A batch plan as a PLAN_DTYPE array (cmp_batch_row [B]) from such an array or from (offset, k, f) triples."""
    if isinstance(plan, np.ndarray) and plan.dtype == PLAN_DTYPE:
        return np.ascontiguousarray(plan)
    out = np.zeros(len(plan), PLAN_DTYPE)
    for i, (o, k, f) in enumerate(plan):
        out[i] = (int(o), int(k), int(f))
    return out


def build_batch(ids, layout, plan, W):
    """-> (x int32 [B, W], y int32 [B, W], status int32 [B, 2])."""
    plan = as_plan(plan)
    B = len(plan)
    x, y, st = np.zeros((B, W), np.int32), np.zeros((B, W), np.int32), np.zeros((B, 2), np.int32)
    for b in range(B):
        x[b], y[b], st[b] = build_row(ids, layout, plan['offset'][b], plan['transpose'][b], plan['stretch_q10'][b], W)
    return x, y, st


def stretch_bounds(stretch):
    """The integer range f is drawn from for a stretch fraction: [round(1024 (1 - stretch)), round(1024 (1 + stretch))]."""
    return int(round(STRETCH_ONE * (1.0 - stretch))), int(round(STRETCH_ONE * (1.0 + stretch)))


def check_augment_options(transpose=0, stretch=0.0, random_crop=False):
    """-> (transpose int in 0..12, stretch float in 0..0.5, random_crop bool); ValueError / TypeError otherwise."""
    if isinstance(transpose, bool) or not isinstance(transpose, (int, np.integer)):
        raise TypeError('augment_transpose=%r must be an integer number of semitones' % (transpose,))
    if not 0 <= int(transpose) <= 12:
        raise ValueError('augment_transpose=%d must be in 0..12 semitones' % transpose)
    if isinstance(stretch, bool) or not isinstance(stretch, (int, float, np.integer, np.floating)):
        raise TypeError('augment_stretch=%r must be a number' % (stretch,))
    stretch = float(stretch)
    if not 0.0 <= stretch <= 0.5:                                  # (a NaN fails both comparisons)
        raise ValueError('augment_stretch=%r must be a fraction in 0..0.5' % stretch)
    if not isinstance(random_crop, (bool, np.bool_)):
        raise TypeError('random_crop=%r must be true or false' % (random_crop,))
    return int(transpose), stretch, bool(random_crop)
