"""Streams, plans and case features shared by the augmentation tests (tests/test_augment_host.py on the CPU,
tests/test_gpu_batch_kernel.py and tests/test_gpu_train_dataset.py on the device).

One stream per layout, built in segments so that the shapes the block scans of batch_rows_kernel can get wrong all occur at known
positions (token positions of the stream; a plan row at offset 0 sees them as positions of its span):

    [0, 300)      non-shift events with runs at 60..69 (straddles lanes 63 / 64) and 250..259 (straddles chunk tokens 255 / 256);
                  pitches 0 and 127, NOTE_ON and NOTE_OFF, in the first four tokens
    [300, 600)    ONE run of 300 shift tokens with random, non-canonical values: longer than a 256-token chunk
    [600, 1300)   no shift token at all (pitches 0 and 127 first)
    [1300, 3500)  shift tokens of ONE step each: at f = 512 a span of them emits far fewer than W + 1 ids -- the fallback
    [3500, n)     a random mix, 30 % shift tokens: 40 % of one step (runs that vanish at f < 1024), 40 % of M steps (two ids at
                  f > 1024: the row grows), the rest random; ends inside a run

`features` states on the host restatement what a case row contains; the tests assert that the union over their cases holds every
feature they were built for, so a change of the streams cannot silently stop covering one."""
import numpy as np

from composer_amd import augment
from composer_amd.grammar import EventGrammar

LAYOUTS = {"default": (10, 100, 32), "small": (10, 50, 4)}       # (time_step_increment, max_time_steps, velocity_bins)
WS = (1, 7, 126, 127, 128, 1024)
BS = (1, 5)
N_STREAM = 6200
ALL_FEATURES = ("straddle_63_64", "straddle_255_256", "run_over_chunk", "starts_in_run", "ends_in_run", "all_shift", "no_shift",
                "grew", "shrank", "vanished_run", "fallback", "last_offset", "clamp_low", "clamp_high", "identity",
                "f512", "f1000", "f1024", "f1100", "f1536")

_cache = {}


def layout(name):
    return EventGrammar.from_dataset_params(*LAYOUTS[name], rules=0)


def stream(name):
    """(ids uint16 [N_STREAM], layout)."""
    if name in _cache:
        return _cache[name]
    g = layout(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    M, ts0 = g.time_shift_n, g.time_shift0
    others = [i for i in range(g.vocab_size) if not ts0 <= i < ts0 + M]          # notes, velocities, pedal

    def plain(n):
        return rng.choice(others, size=n)
    corners = [g.note_on0, g.note_on0 + 127, g.note_off0, g.note_off0 + 127]
    seg0 = plain(300)
    seg0[:4] = corners
    seg0[60:70] = ts0 + rng.integers(0, M, size=10)
    seg0[250:260] = ts0 + rng.integers(0, M, size=10)
    seg1 = ts0 + rng.integers(0, M, size=300)
    seg2 = plain(700)
    seg2[:4] = corners
    seg3 = np.full(2200, ts0)
    n4 = N_STREAM - 3500
    seg4 = plain(n4)
    sh = rng.random(n4) < 0.3
    u = rng.random(int(sh.sum()))
    seg4[sh] = np.where(u < 0.4, ts0, np.where(u < 0.8, ts0 + M - 1, ts0 + rng.integers(0, M, size=int(sh.sum()))))
    seg4[-3:] = ts0 + 4
    ids = np.concatenate([seg0, seg1, seg2, seg3, seg4]).astype(np.uint16)
    assert len(ids) == N_STREAM
    _cache[name] = (ids, g)
    return _cache[name]


def rows_for(W):
    """The seven plan rows (offset, transpose, stretch) the cases of a window size draw from."""
    return [(0, 12, 1100), (305, -12, 512), (1303, 0, 512), (N_STREAM - (W + 1), 5, 1536), (3600, -3, 512), (290, 12, 1024),
            (600, -12, 1000)]


def plan_for(W, B):
    """B = 5: five of the seven rows, B = 1: a sixth, rotating with the window size so that every row meets several sizes."""
    wi = WS.index(W)
    rows = rows_for(W)
    pick = [(wi + i) % 7 for i in range(5)] if B == 5 else [(wi + 5) % 7]
    return augment.as_plan([rows[i] for i in pick])


def cases(name):
    """[(W, B, plan)]: the whole grid on the default layout, three of its cases on the second one."""
    grid = [(W, B) for W in WS for B in BS] if name == "default" else [(7, 5), (128, 5), (1024, 1)]
    return [(W, B, plan_for(W, B)) for W, B in grid]


def features(ids, g, row, W):
    """The set of ALL_FEATURES names one plan row shows (host restatement only)."""
    off, k, f = int(row["offset"]), int(row["transpose"]), int(row["stretch_q10"])
    n = len(ids)
    S = min(2 * (W + 1), n - off)
    src = ids[off:off + S].astype(np.int64)
    ts0, M = g.time_shift0, g.time_shift_n
    sh = (src >= ts0) & (src < ts0 + M)
    out = {"f%d" % f}
    runs, i = [], 0
    while i < S:
        if sh[i]:
            j = i
            while j + 1 < S and sh[j + 1]:
                j += 1
            runs.append((i, j))
            i = j + 1
        else:
            i += 1
    for a, b in runs:
        if a <= 63 and b >= 64:
            out.add("straddle_63_64")
        if a <= 255 and b >= 256:
            out.add("straddle_255_256")
        if b - a + 1 > 256:
            out.add("run_over_chunk")
    is_shift = lambda v: ts0 <= int(v) < ts0 + M
    if off > 0 and sh[0] and is_shift(ids[off - 1]):
        out.add("starts_in_run")
    if off + S < n and sh[-1] and is_shift(ids[off + S]):
        out.add("ends_in_run")
    if sh.all():
        out.add("all_shift")
    if not sh.any():
        out.add("no_shift")
    if off == n - (W + 1):
        out.add("last_offset")
    _, _, (count, flags) = augment.build_row(ids, g, off, k, f, W)
    if flags & augment.FALLBACK:
        out.add("fallback")
    if f == augment.STRETCH_ONE:
        out.add("identity")
    else:
        em = augment.stretch_tokens(src, g, f)
        if not flags and len(em) > S:
            out.add("grew")
        if not flags and len(em) < S:
            out.add("shrank")
        t = 0
        for a, b in runs:
            r = int((src[a:b + 1] - ts0 + 1).sum())
            if augment.R(t + r, f) == augment.R(t, f):
                out.add("vanished_run")
            t += r
    used = src[:W + 1] if (flags or f == augment.STRETCH_ONE) else augment.stretch_tokens(src, g, f)[:W + 1]
    for base in (g.note_on0, g.note_off0):
        p = used[(used >= base) & (used < base + 128)] - base
        if (p + k < 0).any():
            out.add("clamp_low")
        if (p + k > 127).any():
            out.add("clamp_high")
    return out


def covered(names=("default", "small")):
    """Union of the features over every row of every case of the named layouts."""
    got = set()
    for name in names:
        ids, g = stream(name)
        for W, B, plan in cases(name):
            for row in plan:
                got |= features(ids, g, row, W)
    return got
