"""Event-grammar decoding: the host restatement of the contract in include/composer_hip.h ("event-grammar decoding").

`NoteSequence.from_events` silently drops a NOTE_OFF of a silent pitch, a NOTE_ON of a sounding one, a SUSTAIN_ON while the pedal
is down and a SUSTAIN_OFF while it is up.  An `EventGrammar` names the id layout of a vocabulary, folds an id sequence into the
state those four cases depend on (which pitches sound, where the pedal is, plus the summed time shifts) and says which ids are
banned in a state.  The decode chains keep the same state per row on the device and draw from the allowed ids only
(`Transformer.generate(..., grammar=...)`); this module is what the tests compare them with.  Pure numpy / Python.

`TimedRules` restates the second contract of that header ("timed generation") over an `EventGrammar`: a time budget the draws land
on exactly, an ending phase that only releases what sounds, and a polyphony cap (`Transformer.generate(..., duration_steps=,
max_polyphony=)`).
"""
import numpy as np

from composer_amd import dataset as ds

NOTE_OFF_SOUNDING = 1      # bans NOTE_OFF p while p is silent
NOTE_ON_SILENT = 2         # bans NOTE_ON p while p sounds
PEDAL = 4                  # bans SUSTAIN_ON while the pedal is down, SUSTAIN_OFF while it is up
ALL = NOTE_OFF_SOUNDING | NOTE_ON_SILENT | PEDAL
PITCHES = 128


def words_for(vocab_size):
    return (int(vocab_size) + 31) // 32


class GrammarState:
    """sounding: bool [128]; pedal: bool; time_steps: the summed shifts of the TIME_SHIFT events seen."""
    __slots__ = ('sounding', 'pedal', 'time_steps')

    def __init__(self, sounding=None, pedal=False, time_steps=0):
        self.sounding = np.zeros(PITCHES, bool) if sounding is None else np.array(sounding, bool)
        self.pedal = bool(pedal)
        self.time_steps = int(time_steps)

    def copy(self):
        return GrammarState(self.sounding, self.pedal, self.time_steps)

    def sounding_words(self):
        """uint32 [4]: bit p % 32 of word p // 32 = pitch p sounds (cmp_decode_grammar_state's layout)"""
        return np.packbits(self.sounding, bitorder='little').view('<u4').astype(np.uint32)

    def __eq__(self, other):
        return (isinstance(other, GrammarState) and np.array_equal(self.sounding, other.sounding) and self.pedal == other.pedal
                and self.time_steps == other.time_steps)

    def __repr__(self):
        return 'GrammarState(sounding=%s, pedal=%s, time_steps=%d)' % (np.flatnonzero(self.sounding).tolist(), self.pedal,
                                                                      self.time_steps)


def ban_words(vocab_size, banned):
    """The static ban vector, uint32 [ceil(V / 32)] (bit c % 32 of word c // 32: id c is never drawn), from a sequence of ids, a
    bool mask of V entries or such a vector itself."""
    V, nw = int(vocab_size), words_for(vocab_size)
    a = np.asarray(banned)
    if a.dtype == np.uint32 and a.shape == (nw,):
        w = a.copy()
    else:
        if a.dtype == bool:
            if a.shape != (V,):
                raise ValueError('banned_ids: a mask of %d entries for a vocabulary of %d' % (a.size, V))
            mask = a
        else:
            idx = a.astype(np.int64).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= V):
                raise ValueError('banned_ids: an id outside [0, %d)' % V)
            mask = np.zeros(V, bool)
            mask[idx] = True
        bits = np.zeros(nw * 32, bool)
        bits[:V] = mask
        w = np.packbits(bits, bitorder='little').view('<u4').astype(np.uint32)
    if V & 31:
        w[-1] &= np.uint32((1 << (V & 31)) - 1)
    return np.ascontiguousarray(w)


def words_to_mask(vocab_size, words):
    return np.unpackbits(np.ascontiguousarray(words, '<u4').view(np.uint8), bitorder='little')[:int(vocab_size)].astype(bool)


def check_static_bans(vocab_size, words, grammar=None):
    """The rule cmp_decode_grammar enforces: with a layout at least one TIME_SHIFT id stays drawable, without one at least one id."""
    mask = words_to_mask(vocab_size, words)
    if grammar is not None:
        ts = mask[grammar.time_shift0:grammar.time_shift0 + grammar.time_shift_n]
        if ts.all():
            raise ValueError('the static ban vector bans every TIME_SHIFT id [%d, %d): at least one must stay drawable'
                             % (grammar.time_shift0, grammar.time_shift0 + grammar.time_shift_n))
    elif mask.all():
        raise ValueError('the static ban vector bans all %d ids: at least one must stay drawable' % int(vocab_size))
    return words


class EventGrammar:
    """The id layout of an event vocabulary and the rules in force.  note_on0 / note_off0: the first of 128 consecutive ids each
    (id - base = pitch); time_shift0, time_shift_n: the TIME_SHIFT ids; sustain_on / sustain_off: single ids, or -1 for both."""

    def __init__(self, vocab_size, note_on0, note_off0, time_shift0, time_shift_n, sustain_on=-1, sustain_off=-1, rules=ALL):
        self.vocab_size = V = int(vocab_size)
        self.note_on0, self.note_off0 = int(note_on0), int(note_off0)
        self.time_shift0, self.time_shift_n = int(time_shift0), int(time_shift_n)
        self.sustain_on, self.sustain_off = int(sustain_on), int(sustain_off)
        self.rules = int(rules)
        if self.rules & ~ALL:
            raise ValueError('rules=0x%x: unknown rule bits (known: 0x%x)' % (self.rules, ALL))
        if self.time_shift_n < 1:
            raise ValueError('time_shift_n=%d must be >= 1' % self.time_shift_n)
        if (self.sustain_on < 0) != (self.sustain_off < 0):
            raise ValueError('sustain_on=%d without sustain_off=%d (or the reverse): both ids, or -1 for both'
                             % (self.sustain_on, self.sustain_off))
        if self.sustain_on < -1 or self.sustain_off < -1:
            raise ValueError('sustain ids %d / %d: an id, or -1 for both' % (self.sustain_on, self.sustain_off))
        ranges = [('note_on', self.note_on0, PITCHES), ('note_off', self.note_off0, PITCHES),
                  ('time_shift', self.time_shift0, self.time_shift_n)]
        if self.sustain_on >= 0:
            ranges += [('sustain_on', self.sustain_on, 1), ('sustain_off', self.sustain_off, 1)]
        for name, lo, n in ranges:
            if lo < 0 or lo + n > V:
                raise ValueError('%s ids [%d, %d) outside the vocabulary [0, %d)' % (name, lo, lo + n, V))
        for i, (na, la, ca) in enumerate(ranges):
            for nb, lb, cb in ranges[i + 1:]:
                if not (la + ca <= lb or lb + cb <= la):
                    raise ValueError('the %s ids [%d, %d) overlap the %s ids [%d, %d)' % (na, la, la + ca, nb, lb, lb + cb))

    @classmethod
    def from_dataset_params(cls, time_step_increment, max_time_steps, velocity_bins, rules=ALL):
        """The layout `composer_amd.dataset.event_ranges` gives for a dataset configuration (the default one: 0 / 128 / 288, 100 /
        388 / 389 with 390 ids)."""
        rg = ds.event_ranges(ds.event_value_ranges(time_step_increment, max_time_steps, velocity_bins))
        return cls(rg[ds.SUSTAIN_OFF].stop, rg[ds.NOTE_ON].start, rg[ds.NOTE_OFF].start, rg[ds.TIME_SHIFT].start,
                   len(rg[ds.TIME_SHIFT]), rg[ds.SUSTAIN_ON].start, rg[ds.SUSTAIN_OFF].start, rules)

    def to_c(self):
        from composer_amd import _lib
        return _lib.EventGrammar(self.note_on0, self.note_off0, self.time_shift0, self.time_shift_n, self.sustain_on,
                                 self.sustain_off, self.rules)

    # ------------------------------------------------------------------ the state
    def step(self, state, event_id):
        """Applies one id to `state` in place; True when from_events would ignore the event (the state did not move and the id is
        one of the four no-op cases)."""
        i = int(event_id)
        p = i - self.note_on0
        if 0 <= p < PITCHES:
            if state.sounding[p]:
                return True
            state.sounding[p] = True
            return False
        p = i - self.note_off0
        if 0 <= p < PITCHES:
            if not state.sounding[p]:
                return True
            state.sounding[p] = False
            return False
        j = i - self.time_shift0
        if 0 <= j < self.time_shift_n:
            state.time_steps += j + 1
            return False
        if self.sustain_on >= 0 and i == self.sustain_on:
            if state.pedal:
                return True
            state.pedal = True
            return False
        if self.sustain_on >= 0 and i == self.sustain_off:
            if not state.pedal:
                return True
            state.pedal = False
            return False
        return False

    def fold(self, ids, state=None):
        """The state after `ids`, from `state` (default: nothing sounds, pedal up): the left fold of `step`."""
        st = GrammarState() if state is None else state.copy()
        for i in np.asarray(ids).reshape(-1):
            self.step(st, i)
        return st

    def ignored_events(self, ids):
        """Indices of the events of `ids` that NoteSequence.from_events drops (whatever `rules` says)."""
        st, out = GrammarState(), []
        for k, i in enumerate(np.asarray(ids).reshape(-1)):
            if self.step(st, i):
                out.append(k)
        return out

    def banned(self, state, static=None):
        """bool [V]: the ids that cannot be drawn in `state` under `rules`, ORed with the static ban vector when given."""
        b = np.zeros(self.vocab_size, bool)
        if self.rules & NOTE_OFF_SOUNDING:
            b[self.note_off0:self.note_off0 + PITCHES] |= ~state.sounding
        if self.rules & NOTE_ON_SILENT:
            b[self.note_on0:self.note_on0 + PITCHES] |= state.sounding
        if self.rules & PEDAL and self.sustain_on >= 0:
            b[self.sustain_on if state.pedal else self.sustain_off] = True
        if static is not None:
            b |= words_to_mask(self.vocab_size, static)
        return b

    def pitch_range_bans(self, lo, hi):
        """The static ban vector (uint32 words) that bans NOTE_ON of every pitch outside [lo, hi]."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo <= hi < PITCHES:
            raise ValueError('pitch range %d:%d: 0 <= LO <= HI <= 127' % (lo, hi))
        mask = np.zeros(self.vocab_size, bool)
        mask[self.note_on0:self.note_on0 + lo] = True
        mask[self.note_on0 + hi + 1:self.note_on0 + PITCHES] = True
        return ban_words(self.vocab_size, mask)


# ---------------------------------------------------------------------- timed generation (composer_hip.h, "timed generation")
PLAY, ENDING, DONE = 0, 1, 2


class TimedState:
    """The state of a row under a budget: the grammar's state `g`, the step count `t_end` at which the generated part ends (0: no
    time budget), the ids produced so far and `done_at` (-1 until the state first becomes DONE, then the ids produced by then)."""
    __slots__ = ('g', 't_end', 'produced', 'done_at')

    def __init__(self, g=None, t_end=0, produced=0, done_at=-1):
        self.g = GrammarState() if g is None else g
        self.t_end, self.produced, self.done_at = int(t_end), int(produced), int(done_at)

    def copy(self):
        return TimedState(self.g.copy(), self.t_end, self.produced, self.done_at)

    @property
    def steps_left(self):
        return self.t_end - self.g.time_steps if self.t_end else 0

    def __repr__(self):
        return 'TimedState(%r, t_end=%d, produced=%d, done_at=%d)' % (self.g, self.t_end, self.produced, self.done_at)


class TimedRules:
    """The budget of cmp_decode_budget over an `EventGrammar`: `time_steps` >= 0 steps of generated time (0: none) that the draw
    lands on exactly, an ending phase that only releases what sounds, and at most `max_polyphony` >= 0 sounding pitches (0: no
    cap).  Phases, ban sets and the frozen DONE state as the decode chains keep them per row on the device."""

    def __init__(self, grammar, time_steps=0, max_polyphony=0):
        self.grammar = grammar
        self.time_steps, self.max_polyphony = int(time_steps), int(max_polyphony)
        if self.time_steps < 0:
            raise ValueError('time_steps=%d must be >= 0 (0: no time budget)' % self.time_steps)
        if self.max_polyphony < 0:
            raise ValueError('max_polyphony=%d must be >= 0 (0: no cap)' % self.max_polyphony)

    def check_static_bans(self, static):
        """The rule the begin calls enforce: a time budget needs the one-step shift drawable, or a row one step short of t_end
        could never land on it."""
        if self.time_steps and static is not None and words_to_mask(self.grammar.vocab_size, static)[self.grammar.time_shift0]:
            raise ValueError('the static ban vector bans the one-step TIME_SHIFT id %d: a time budget needs it drawable'
                             % self.grammar.time_shift0)
        return static

    def t_end(self, prompt):
        """time_steps(prompt) + the budget: the prompt's own duration is not charged to it.  0 without a time budget."""
        return self.grammar.fold(prompt).time_steps + self.time_steps if self.time_steps else 0

    def begin(self, prompt):
        """The state of a row whose sequence so far is its prompt."""
        return TimedState(self.grammar.fold(prompt), self.t_end(prompt))

    def phase(self, state):
        if state.t_end == 0 or state.g.time_steps < state.t_end:
            return PLAY
        return ENDING if state.g.sounding.any() or state.g.pedal else DONE

    def banned(self, state, static=None):
        """bool [V]: the ban set of the next draw in `state`."""
        g, ph = self.grammar, self.phase(state)
        if ph == PLAY:
            b = g.banned(state.g, static)
            if state.t_end:
                b[g.time_shift0 + min(g.time_shift_n, state.t_end - state.g.time_steps):g.time_shift0 + g.time_shift_n] = True
            if self.max_polyphony and int(state.g.sounding.sum()) >= self.max_polyphony:
                b[g.note_on0:g.note_on0 + PITCHES] = True
            return b
        b = np.ones(g.vocab_size, bool)
        if ph == ENDING:                 # the static vector and the rule bits are ignored: the ending must be able to finish
            b[g.note_off0:g.note_off0 + PITCHES] = ~state.g.sounding
            if state.g.pedal:
                b[g.sustain_off] = False
        else:
            b[g.time_shift0] = False     # the filler
        return b

    def step(self, state, event_id):
        """Applies one drawn id to `state` in place.  In DONE the id is a filler: only `produced` moves.  Returns `done_at`."""
        if self.phase(state) != DONE:
            self.grammar.step(state.g, event_id)
            state.produced += 1
            if self.phase(state) == DONE:
                state.done_at = state.produced
        else:
            state.produced += 1
        return state.done_at

    def fold(self, prompt, ids):
        """The state after `ids` drawn behind `prompt`."""
        st = self.begin(prompt)
        for i in np.asarray(ids).reshape(-1):
            self.step(st, i)
        return st
