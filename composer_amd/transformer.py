"""Host-side mirror of the reference's `composer.models.Transformer` (reference
composer/models/transformer.py:599-960) over libcomposer_hip.so.

Same constructor arguments (transformer.py:610-614), same call / train / evaluate / load_from_checkpoint
surface (cli.py:579-589, 606-615, 635-676).  All arithmetic happens in hand-written HIP kernels on an
MI355X; this file only moves integers in and numbers out.  There is no CPU path.
"""
import collections
import ctypes as C
import enum
import logging
import math
import os
import shutil
import time
from pathlib import Path

import numpy as np

from . import _lib
from . import augment
from . import checkpoint as ckpt
from .dataset import DeviceBatch


def slide_context_length(n, window, keep):
    """c(n): the number of tokens the sliding-window decode ('kv-slide') draws the next id from, when prompt ++ generated ids
    holds n tokens.  The context grows to `window`; the draw after that re-encodes the last `keep` tokens (1 <= keep <= window - 1)
    from position 0, then the context grows to `window` again: a period of window - keep + 1 draws."""
    n, window, keep = int(n), int(window), int(keep)
    if not 1 <= keep <= window - 1:
        raise ValueError('slide keep = %d outside [1, window_size - 1 = %d]' % (keep, window - 1))
    if n < 1:
        raise ValueError('n = %d: the sequence holds at least one token' % n)
    if n <= window:
        return n
    return keep + (n - window - 1) % (window - keep + 1)


def score_windows(n, window, keep):
    """The forward passes that score a sequence of n ids under the scoring contract (include/composer_hip.h, "scoring"): a list
    of (start, length, first_scored_row).  A window feeds s[start : start + length] at positions 0 .. length - 1; its row r holds
    the logits of position start + r + 1, drawn from the context s[start : start + r + 1], and the rows first_scored_row ..
    length - 1 are the ones that count.  Every position 1 .. n - 1 is scored by exactly one (window, row), and the context that
    row gives it has length slide_context_length(position, window, keep): for positions up to `window` the plain causal pass,
    past it the conditioning of 'kv-slide' generation.  Window 0 is s[0 : min(n - 1, W)] and scores every row; window j >= 1
    starts at W + 1 + (j - 1)(W - keep + 1) - keep, holds up to W inputs and scores rows keep - 1 ...  n = 1: no window."""
    n, W, keep = int(n), int(window), int(keep)
    if not 1 <= keep <= W - 1:
        raise ValueError('slide keep = %d outside [1, window_size - 1 = %d]' % (keep, W - 1))
    if n < 1:
        raise ValueError('n = %d: the sequence holds at least one token' % n)
    out = []
    if n >= 2:
        out.append((0, min(n - 1, W), 0))
    period = W - keep + 1
    first = W + 1                                   # the first position window j scores
    while first <= n - 1:
        start = first - keep
        out.append((start, min(W, n - 1 - start), keep - 1))
        first += period
    return out


class SequenceScore:
    """What `Transformer.score` returns for one sequence s of N ids: `logp` (nats), `rank` (0 = the model's first choice) and
    `entropy` (nats) of the positions 1 .. N-1, aligned with `targets` = s[1:]; and the figures derived from them.  An empty
    result (N = 1) has NaN figures."""

    def __init__(self, targets, logp, rank, entropy):
        self.targets = np.asarray(targets, np.int32)
        self.logp = np.asarray(logp, np.float32)
        self.rank = np.asarray(rank, np.int32)
        self.entropy = np.asarray(entropy, np.float32)
        if not (self.targets.shape == self.logp.shape == self.rank.shape == self.entropy.shape and self.targets.ndim == 1):
            raise ValueError('SequenceScore: the four arrays must be 1-D of one length')

    def __len__(self):
        return int(self.logp.size)

    @property
    def events(self):
        return len(self)

    @property
    def log_likelihood(self):
        """Sum of the log-probabilities (float64), nats."""
        return float(self.logp.astype(np.float64).sum())

    @property
    def nll_per_event(self):
        return -self.log_likelihood / len(self) if len(self) else float('nan')

    @property
    def bits_per_event(self):
        return self.nll_per_event / math.log(2.0)

    @property
    def perplexity(self):
        nll = self.nll_per_event
        if nll != nll:
            return float('nan')
        return math.exp(nll) if nll < 709.0 else float('inf')

    @property
    def top1_accuracy(self):
        return float((self.rank == 0).mean()) if len(self) else float('nan')

    def by_event_type(self, event_ranges):
        """{event type: (count, mean NLL or NaN)} over the scored events, `event_ranges` = composer_amd.dataset.event_ranges(...)
        (event type -> range of ids)."""
        out = collections.OrderedDict()
        nll = -self.logp.astype(np.float64)
        for t, interval in event_ranges.items():
            sel = (self.targets >= interval.start) & (self.targets < interval.stop)
            k = int(sel.sum())
            out[t] = (k, float(nll[sel].sum() / k) if k else float('nan'))
        return out

    def to_dict(self, arrays=True):
        d = {'events': len(self), 'nll_per_event': self.nll_per_event, 'bits_per_event': self.bits_per_event,
             'perplexity': self.perplexity, 'top1_accuracy': self.top1_accuracy}
        if arrays:
            d.update(logp=[float(v) for v in self.logp], rank=[int(v) for v in self.rank], entropy=[float(v) for v in self.entropy])
        return d


def score_sequences(score_call, sequences, window, keep, max_tokens):
    """The host side of `Transformer.score`, no GPU: plans `score_windows` for every sequence, packs the windows into as few
    `score_call(x, y) -> (logp, rank, entropy)` calls as `max_tokens` (= B * T of a call) allows and scatters the rows that count
    into one `SequenceScore` per sequence.  x, y: int32 [B, T]; the windows of a call are right-padded with id 0 to the call's T
    and pad targets are -1, so are the targets of the rows before a window's first scored row.  A window is never split (its rows
    need the whole context): one that is longer than `max_tokens` goes out alone in a call of its own length, and it is
    `score_call`'s business to refuse it (cmp_score does, by name, when the model's workspace was sized smaller)."""
    seqs = [np.ascontiguousarray(np.asarray(s, dtype=np.int64).reshape(-1)) for s in sequences]
    jobs = []                                                       # (length, sequence, start, first scored row)
    for k, s in enumerate(seqs):
        if s.size == 0:
            raise ValueError('score: sequence %d is empty' % k)
        jobs += [(length, k, start, first) for start, length, first in score_windows(s.size, window, keep)]
    jobs.sort(key=lambda j: (-j[0], j[1], j[2]))                    # longest first: a call's T is its first window's length
    res = [(np.zeros(s.size - 1, np.float32), np.full(s.size - 1, -1, np.int32), np.zeros(s.size - 1, np.float32)) for s in seqs]
    i = 0
    while i < len(jobs):
        T = jobs[i][0]
        B = max(1, min(len(jobs) - i, int(max_tokens) // T))
        x = np.zeros((B, T), np.int32)
        y = np.full((B, T), -1, np.int32)
        for b, (length, k, start, first) in enumerate(jobs[i:i + B]):
            x[b, :length] = seqs[k][start:start + length]
            y[b, first:length] = seqs[k][start + first + 1:start + length + 1]
        outs = score_call(x, y)
        for b, (length, k, start, first) in enumerate(jobs[i:i + B]):
            for dst, src in zip(res[k], outs):
                dst[start + first:start + length] = src[b, first:length]
        i += B
    return [SequenceScore(s[1:], *r) for s, r in zip(seqs, res)]


class EvalReport:
    """What `Transformer.evaluate_dataset` returns: the table of one validation pass (cmp_eval_dataset) and the figures derived from it.
    `names`: the event classes in `event_ranges` order; the table's slot len(names) holds every id outside them.  `nll` are float64
    sums in nats, `count` / `correct` integers, one per slot.  An empty total has NaN figures."""

    def __init__(self, names, nll, count, correct, windows=0):
        self.names = list(names)
        k = len(self.names) + 1
        self.nll = [float(v) for v in list(nll)[:k]]
        self.count = [int(v) for v in list(count)[:k]]
        self.correct = [int(v) for v in list(correct)[:k]]
        if not len(self.nll) == len(self.count) == len(self.correct) == k:
            raise ValueError('EvalReport: the table needs %d slots (the classes and one for every other id)' % k)
        self.windows = int(windows)

    @property
    def events(self):
        return sum(self.count)

    @property
    def loss(self):
        """Mean NLL per event, nats: the slots' sums added in slot order, over the events."""
        return math.fsum(self.nll) / self.events if self.events else float('nan')

    @property
    def accuracy(self):
        return sum(self.correct) / self.events if self.events else float('nan')

    @property
    def bits_per_event(self):
        return self.loss / math.log(2.0)

    @property
    def perplexity(self):
        nll = self.loss
        if nll != nll:
            return float('nan')
        return math.exp(nll) if nll < 709.0 else float('inf')

    @property
    def other(self):
        """(count, mean NLL or NaN, accuracy or NaN) of the ids outside every class."""
        return self._slot(len(self.names))

    def _slot(self, i):
        k = self.count[i]
        return (k, self.nll[i] / k if k else float('nan'), self.correct[i] / k if k else float('nan'))

    @property
    def by_event_type(self):
        """{event type: (count, mean NLL or NaN, accuracy or NaN)} in `event_ranges` order."""
        return collections.OrderedDict((t, self._slot(i)) for i, t in enumerate(self.names))

    def to_dict(self):
        d = {'events': self.events, 'windows': self.windows, 'loss': self.loss, 'accuracy': self.accuracy,
             'bits_per_event': self.bits_per_event, 'perplexity': self.perplexity,
             'by_event_type': {str(t): {'count': c, 'nll_per_event': n, 'accuracy': a} for t, (c, n, a) in self.by_event_type.items()}}
        if self.count[len(self.names)]:
            d['other'] = dict(zip(('count', 'nll_per_event', 'accuracy'), self.other))
        return d


class ValidationTracker:
    """The decision after every validation pass, no GPU: `update(step, loss) -> (is_best, stop)`.  A loss improves when
    loss < best - min_delta (strictly; the first finite loss always does, a NaN never); `stop` turns true once `patience`
    consecutive passes have not improved (patience 0: never).  `state()` / `from_state()` carry it through a checkpoint's meta."""

    def __init__(self, patience=0, min_delta=0.0):
        patience, min_delta = int(patience), float(min_delta)
        if patience < 0 or not min_delta >= 0.0:
            raise ValueError('early_stop_patience = %d and min_delta = %g must not be negative' % (patience, min_delta))
        self.patience, self.min_delta = patience, min_delta
        self.best, self.best_step, self.bad_passes = None, None, 0

    def update(self, step, loss):
        loss = float(loss)
        is_best = loss == loss and (self.best is None or loss < self.best - self.min_delta)
        if is_best:
            self.best, self.best_step, self.bad_passes = loss, int(step), 0
        else:
            self.bad_passes += 1
        return is_best, self.patience > 0 and self.bad_passes >= self.patience

    def state(self):
        return {'best': self.best, 'best_step': self.best_step, 'bad_passes': self.bad_passes}

    def load_state(self, state):
        """Takes over the counts of an earlier run (patience and min_delta stay this run's)."""
        if state:
            best = state.get('best')
            self.best = None if best is None else float(best)
            self.best_step = state.get('best_step')
            self.bad_passes = int(state.get('bad_passes', 0))
        return self

    @classmethod
    def from_state(cls, state, patience=0, min_delta=0.0):
        return cls(patience, min_delta).load_state(state)


def exchange_verdict(all_reduce_sum, rank, is_best, stop):
    """Rank 0's verdict on every rank: a two-element vector through `all_reduce_sum`, to which rank 0 contributes (is_best, stop) and
    every other rank zeros -- so no rank leaves the train loop alone while its peers wait in a gradient all-reduce.  Collective."""
    mine = [float(bool(is_best)), float(bool(stop))] if rank == 0 else [0.0, 0.0]
    got = all_reduce_sum(mine)
    return bool(got[0] > 0.5), bool(got[1] > 0.5)


def check_eval_options(eval_freq=0, eval_max_windows=None, early_stop_patience=0, keep_best=False):
    """The argument rule of validation during training: eval_freq >= 0 optimiser steps (0 off), eval_max_windows None or >= 1,
    early_stop_patience >= 0 passes (0 off); patience and keep_best need eval_freq > 0.  Returns them as (int, int | None, int, bool)."""
    eval_freq, early_stop_patience, keep_best = int(eval_freq), int(early_stop_patience), bool(keep_best)
    if eval_freq < 0:
        raise ValueError('eval_freq = %d must not be negative (0: off)' % eval_freq)
    if eval_max_windows is not None:
        eval_max_windows = int(eval_max_windows)
        if eval_max_windows < 1:
            raise ValueError('eval_max_windows = %d must be at least 1' % eval_max_windows)
    if early_stop_patience < 0:
        raise ValueError('early_stop_patience = %d must not be negative (0: off)' % early_stop_patience)
    if (early_stop_patience or keep_best) and not eval_freq:
        raise ValueError('early_stop_patience / keep_best need eval_freq > 0: there is no validation pass to act on')
    return eval_freq, eval_max_windows, early_stop_patience, keep_best


def check_sampling(top_k, top_p):
    """The argument rule of truncated sampling: top_k an integer >= 0 (0: off), top_p in (0, 1] (1: off).  Returns (int, float)."""
    if isinstance(top_k, (bool, np.bool_)) or int(top_k) != top_k:
        raise ValueError('top_k = %r: an integer >= 0 (0: off)' % (top_k,))
    if int(top_k) < 0:
        raise ValueError('top_k = %d must be >= 0 (0: off)' % int(top_k))
    tp = float(top_p)
    if not 0.0 < tp <= 1.0:                                     # a NaN fails both comparisons
        raise ValueError('top_p = %r outside (0, 1] (1: off)' % (top_p,))
    return int(top_k), tp


def sampling_keep_set(z, temperature, top_k=0, top_p=1.0):
    """The columns truncated sampling (top-k, then nucleus / top-p) may draw from: a sorted int array.  This is the specification
    the device sampler is held to (include/composer_hip.h, "truncated sampling"), restated in numpy float64 -- no GPU.

    z: one row of logits, taken as float32.  Columns are ranked by (z descending, index ascending).  top_k = 0 or >= V: off,
    otherwise the first top_k columns of the order are the candidates.  top_p = 1: off, otherwise with
    q = exp((z - z_max) / temperature) over the candidates, in float64 from the float32 values of z, temperature and top_p, the
    kept set is the shortest prefix with sum(q[:n]) >= top_p * sum(q), n >= 1.  temperature <= 0 is the greedy argmax: the
    filters change nothing and the set is the argmax column alone."""
    z = np.asarray(z, dtype=np.float32).reshape(-1)
    V = z.size
    if V == 0:
        raise ValueError('sampling_keep_set: an empty row')
    if np.isnan(z).any():
        raise ValueError('sampling_keep_set: the row holds a NaN')
    top_k, top_p = check_sampling(top_k, top_p)
    order = np.lexsort((np.arange(V), -z.astype(np.float64)))   # last key first: z descending, then index ascending
    if not float(temperature) > 0.0:
        return order[:1].astype(np.int64)
    if 0 < top_k < V:
        order = order[:top_k]
    tp = np.float32(top_p)
    if tp < np.float32(1.0):
        z64 = z[order].astype(np.float64)
        q = np.exp((z64 - z64[0]) / np.float64(np.float32(temperature)))
        cum = np.cumsum(q)
        n = int(np.searchsorted(cum, np.float64(tp) * cum[-1], side='left')) + 1     # the first n with cum[n - 1] >= top_p * total
        order = order[:max(1, min(n, order.size))]
    return np.sort(order).astype(np.int64)


class ModelSaveFrequencyMode(enum.Enum):
    """reference composer/models/__init__.py:92-107"""
    EPOCH = 'epoch'
    GLOBAL_STEP = 'global_step'


def _truncated_normal(rng, shape, mean, stddev):
    """tf.keras.initializers.TruncatedNormal: resample outside +-2 sigma (transformer.py:115,188,670-673)."""
    a = rng.standard_normal(shape)
    bad = np.abs(a) > 2.0
    while bad.any():
        a[bad] = rng.standard_normal(int(bad.sum()))
        bad = np.abs(a) > 2.0
    return (mean + stddev * a).astype(np.float32)


class Presents:
    """Lazy `presents` tuple (transformer.py:797-806,820-821): L tensors [2,B,H,T,D] fetched from the saved
    c_attn activations only when indexed (the CLI never reads them)."""

    def __init__(self, model, B, T, generation):
        self._m, self._B, self._T, self._gen = model, B, T, generation

    def __len__(self):
        return self._m.decoder_layers_count

    def __getitem__(self, i):
        if not 0 <= i < len(self):
            raise IndexError(i)
        return self._m._fetch_present(i, self._B, self._T, self._gen)

    def __iter__(self):
        return (self[i] for i in range(len(self)))


def clip_scale(norm, clip_norm):
    """The factor global-norm clipping multiplies the gradient by (tf.clip_by_global_norm): 1 if norm <= clip_norm, else
    clip_norm / norm.  clip_norm 0 means off (1), +inf measures only (1); a NaN norm gives NaN -- no special case."""
    norm, clip_norm = float(norm), float(clip_norm)
    if clip_norm == 0.0:
        return 1.0
    if norm != norm:
        return float('nan')
    return 1.0 if norm <= clip_norm else clip_norm / norm


def warmup_lr(learning_rate, step, warmup_steps):
    """lr(step) = learning_rate * min(1, step / warmup_steps), step = the optimiser step counted from 1; warmup_steps 0: off."""
    if not warmup_steps:
        return float(learning_rate)
    return float(learning_rate) * min(1.0, float(step) / float(warmup_steps))


def check_train_options(clip_norm, accumulate_steps, warmup_steps=0):
    """Range checks shared by Transformer.set_train_options, Transformer.train and the CLI (ValueError names the option)."""
    clip_norm = float(clip_norm)
    if not clip_norm >= 0.0:
        raise ValueError('clip_norm {}: must be 0 (off), positive, or inf (measure only).'.format(clip_norm))
    if int(accumulate_steps) != accumulate_steps or int(accumulate_steps) < 1:
        raise ValueError('accumulate_steps {}: must be an integer >= 1.'.format(accumulate_steps))
    if int(warmup_steps) != warmup_steps or int(warmup_steps) < 0:
        raise ValueError('warmup_steps {}: must be an integer >= 0 (0 = off).'.format(warmup_steps))
    return clip_norm, int(accumulate_steps), int(warmup_steps)


class Transformer:
    def __init__(self, vocab_size, embedding_size, window_size, decoder_layers_count,
                 attention_head_count, use_relative_attention=False, initializer_mean=0,
                 initializer_stddev=0.02, attention_dropout_rate=0.1, residual_dropout_rate=0.1,
                 layer_normalization_epsilon=1e-5, scale=True, use_layer_normalization=True,
                 output_hidden_states=False, output_attention_weights=False, *,
                 dtype='bf16', seed=0, max_batch=1, max_seq=None, device=None, ctx=None):
        if embedding_size % attention_head_count != 0:
            raise AssertionError('hidden size must be a multiple of the attention head count')   # transformer.py:255
        if use_relative_attention:
            # the reference path is broken (Attention.build reads an undefined self.depth, transformer.py:285)
            raise NotImplementedError('use_relative_attention is not supported (broken in the reference too)')
        self.output_hidden_states = bool(output_hidden_states)
        self.output_attention_weights = bool(output_attention_weights)
        self.vocab_size = vocab_size
        self.embedding_size = embedding_size
        self.window_size = window_size
        self.decoder_layers_count = decoder_layers_count
        self.attention_head_count = attention_head_count
        self.use_layer_normalization = use_layer_normalization
        self.initializer_mean = initializer_mean
        self.initializer_stddev = initializer_stddev
        self.dtype = {'fp32': _lib.CMP_FP32, 'float32': _lib.CMP_FP32, 'bf16': _lib.CMP_BF16,
                      'bfloat16': _lib.CMP_BF16}[str(dtype)]
        self.seed = int(seed)
        self._lib = _lib.load()
        _lib.require_gpu()
        if device is None:
            device = int(os.environ.get('LOCAL_RANK', '0'))
        self._own_ctx = ctx is None
        if ctx is None:
            h = C.c_void_p()
            _lib.check(self._lib.cmp_ctx_create(int(device), C.byref(h)), 'cmp_ctx_create')
            ctx = h
        self._ctx = ctx
        cfg = _lib.ModelCfg(vocab_size, embedding_size, window_size, decoder_layers_count, attention_head_count,
                            float(layer_normalization_epsilon), int(bool(scale)), int(bool(use_layer_normalization)),
                            float(attention_dropout_rate), float(residual_dropout_rate), self.dtype,
                            int(max_batch), int(max_seq or window_size), self.seed)
        h = C.c_void_p()
        rc = self._lib.cmp_model_create(self._ctx, C.byref(cfg), C.byref(h))
        if rc != 0:
            msg = _lib.last_error()
            if self._own_ctx:                       # a refused configuration must not leave its context (three streams) behind
                self._lib.cmp_ctx_destroy(self._ctx)
            self._ctx = None
            raise _lib.HipLibraryError("cmp_model_create failed (status %d): %s" % (rc, msg))
        self._h = h
        # tokens per cmp_score call that `score` packs to: what the library's workspace holds at least (an earlier, larger call may have
        # sized it bigger, which only means smaller calls than possible; with max_seq < window_size a full window exceeds this figure,
        # is sent alone, and the library refuses it by name if its workspace is already sized smaller)
        self._max_tokens = max(1, int(max_batch)) * max(1, min(int(max_seq or window_size), int(window_size)))
        self._max_batch = max(1, int(max_batch))
        self._specs = self._param_specs()
        self._learning_rate = 1e-3
        self._dp = None          # (rank, nranks) once init_data_parallel() ran
        self._datasets = {}      # id(DeviceDataset) -> (the dataset, its cmp_dataset in this model's context)
        self.initialize_parameters(self.seed)

    # ------------------------------------------------------------------ lifetime
    def close(self):
        for _, h in getattr(self, '_datasets', {}).values():      # device datasets live in this model's context: they go first
            self._lib.cmp_dataset_destroy(h)
        self._datasets = {}
        if getattr(self, '_h', None):
            self._lib.cmp_model_destroy(self._h)
            self._h = None
            if self._own_ctx and self._ctx:
                self._lib.cmp_ctx_destroy(self._ctx)
            self._ctx = None
        elif getattr(self, '_ctx', None) and getattr(self, '_own_ctx', False):     # construction stopped after the context
            self._lib.cmp_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ parameters
    def _param_specs(self):
        n = C.c_int()
        _lib.check(self._lib.cmp_param_count(self._h, C.byref(n)))
        out = []
        for i in range(n.value):
            name, rank, shape, numel = C.c_char_p(), C.c_int(), (C.c_int64 * 4)(), C.c_int64()
            _lib.check(self._lib.cmp_param_info(self._h, i, C.byref(name), C.byref(rank), C.byref(shape), C.byref(numel)))
            out.append((name.value.decode(), tuple(int(shape[k]) for k in range(rank.value)), int(numel.value)))
        return out

    @property
    def parameter_names(self):
        return [n for n, _, _ in self._specs]

    def parameter_shape(self, name):
        return {n: s for n, s, _ in self._specs}[name]

    def get_parameter(self, name, kind=_lib.KIND_VALUE):
        shape = self.parameter_shape(name)
        a = np.empty(shape, np.float32)
        _lib.check(self._lib.cmp_param_get(self._h, name.encode(), kind, a.ctypes.data_as(C.c_void_p), a.size), 'cmp_param_get')
        return a

    def set_parameter(self, name, value, kind=_lib.KIND_VALUE):
        a = np.ascontiguousarray(np.asarray(value, dtype=np.float32).reshape(self.parameter_shape(name)))
        _lib.check(self._lib.cmp_param_set(self._h, name.encode(), kind, a.ctypes.data_as(C.c_void_p), a.size), 'cmp_param_set')

    def get_weights(self):
        return {n: self.get_parameter(n) for n in self.parameter_names}

    def set_weights(self, weights):
        for n, v in weights.items():
            self.set_parameter(n, v)

    def initialize_parameters(self, seed=0):
        """TruncatedNormal(mean, stddev) for wte/wpe/Conv1D weights, zeros for biases/beta, ones for gamma
        (transformer.py:115,188-190,670-673; Keras LayerNormalization defaults)."""
        rng = np.random.default_rng(seed)
        for name, shape, _ in self._specs:
            if name.endswith('gamma'):
                v = np.ones(shape, np.float32)
            elif name.endswith(('beta', 'bias')):
                v = np.zeros(shape, np.float32)
            else:
                v = _truncated_normal(rng, shape, self.initializer_mean, self.initializer_stddev)
            self.set_parameter(name, v)

    @property
    def iterations(self):
        v = C.c_int64()
        _lib.check(self._lib.cmp_adam_iter_get(self._h, C.byref(v)))
        return int(v.value)

    @iterations.setter
    def iterations(self, v):
        _lib.check(self._lib.cmp_adam_iter_set(self._h, int(v)))

    # ------------------------------------------------------------------ Keras-surface no-ops used by the CLI
    def compile(self, learning_rate):            # transformer.py:835-844
        self._learning_rate = float(learning_rate)

    def build(self, input_shape=None):           # cli.py:607,640
        return None

    def reset_states(self):                      # cli.py:662
        return None

    def summary(self, print_fn=print):           # cli.py:436-440
        total = 0
        print_fn('Model: "transformer"')
        for n, s, k in self._specs:
            print_fn('%-48s %-16s %d' % (n, s, k))
            total += k
        print_fn('Total params: {:,}'.format(total))
        return total

    # ------------------------------------------------------------------ data parallel
    def init_data_parallel(self, rank, world_size, unique_id, gemm_cus=None):
        """One rank per GPU; `unique_id` = 128 bytes from rank 0's `new_unique_id()` shared by the launcher.
        gemm_cus: CUs the persistent GEMM kernels may occupy while gradients are all-reduced (None/0 = all 256)."""
        _lib.check_single_runtime()      # a second RCCL mapped beside the one the library is bound to: fail here, with the paths
        buf = C.create_string_buffer(bytes(unique_id), 128)
        _lib.check(self._lib.cmp_dp_init(self._ctx, int(rank), int(world_size), buf), 'cmp_dp_init')
        if gemm_cus:
            _lib.check(self._lib.cmp_dp_set_gemm_cus(self._ctx, int(gemm_cus)), 'cmp_dp_set_gemm_cus')
        self._dp = (int(rank), int(world_size))

    def init_data_parallel_exchange(self, rank, world_size, all_reduce):
        """The data-parallel step over the caller's transport (cmp_dp_init_exchange): `all_reduce(dev_ptr, count, hip_stream)` must
        leave the sum over all ranks of `count` float32 at device address `dev_ptr`, ordered on `hip_stream`; it is called once per
        gradient bucket (and once for the 3-float metrics message), on every rank in the same order.  An exception it raises fails
        the train step (HipLibraryError) and is kept in `self.exchange_error`."""
        self.exchange_error = None

        def _cb(user, ptr, count, stream):
            try:
                all_reduce(int(ptr), int(count), int(stream or 0))
                return 0
            except BaseException as e:          # never unwind through the C frames
                self.exchange_error = e
                return 1
        self._xcb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)(_cb)     # kept alive with the model
        _lib.check(self._lib.cmp_dp_init_exchange(self._ctx, int(rank), int(world_size), C.cast(self._xcb, C.c_void_p), None),
                   'cmp_dp_init_exchange')
        self._dp = (int(rank), int(world_size))

    def set_mask_rank(self, rank):
        """Rank folded into the dropout seed (seed ^ mix32(rank)); init_data_parallel sets it to the communicator rank."""
        _lib.check(self._lib.cmp_dp_set_mask_rank(self._ctx, int(rank)), 'cmp_dp_set_mask_rank')

    def all_reduce_sum(self, values):
        """Sum of a small float vector over the data-parallel ranks (RCCL, cmp_dp_allreduce_test)."""
        a = np.ascontiguousarray(np.asarray(values, dtype=np.float32).reshape(-1))
        _lib.check(self._lib.cmp_dp_allreduce_test(self._ctx, a.ctypes.data_as(C.c_void_p), a.size), 'cmp_dp_allreduce_test')
        return a

    def all_reduce_pattern(self, reps=20):
        """The gradient exchange of one train step alone (cmp_dp_allreduce_pattern): the step's own bucket pattern back to back on the
        communication stream.  Returns ms per repetition, bytes and messages per repetition.  Collective: every rank calls it."""
        ms, nbytes, msgs = C.c_double(), C.c_int64(), C.c_int()
        _lib.check(self._lib.cmp_dp_allreduce_pattern(self._h, int(reps), C.byref(ms), C.byref(nbytes), C.byref(msgs)),
                   'cmp_dp_allreduce_pattern')
        return {"ms": ms.value / reps, "bytes": nbytes.value, "messages": msgs.value, "reps": int(reps)}

    def dp_stats(self, reset=False):
        """Gradient-exchange telemetry since the last reset (cmp_dp_stats): steps, the communication time per step that the
        backward pass did not hide (ms), bytes and all-reduce calls per step.  Zeros without a communicator."""
        steps, ms, nbytes, msgs = C.c_int64(), C.c_double(), C.c_int64(), C.c_int()
        _lib.check(self._lib.cmp_dp_stats(self._h, int(bool(reset)), C.byref(steps), C.byref(ms), C.byref(nbytes), C.byref(msgs)),
                   'cmp_dp_stats')
        return {"steps": steps.value, "exposed_ms": ms.value / steps.value if steps.value else 0.0,
                "exposed_ms_total": ms.value, "bytes": nbytes.value, "buckets": msgs.value}

    @staticmethod
    def new_unique_id():
        buf = C.create_string_buffer(128)
        _lib.check(_lib.load().cmp_dp_unique_id(buf), 'cmp_dp_unique_id')
        return buf.raw

    # ------------------------------------------------------------------ forward / steps
    @staticmethod
    def _ids(x):
        a = np.asarray(x)
        if a.dtype != np.int32 or not a.flags.c_contiguous:         # (an int32 C-ordered batch is handed over as it is: no copy per step)
            a = np.ascontiguousarray(a.astype(np.int32))
        if a.ndim == 1:
            a = a[None]
        if a.ndim != 2:
            raise ValueError('expected an int tensor with shape [batch, sequence]')
        return a

    def _check_ids(self, a):
        # one pass: a negative id is a huge unsigned one
        if a.size and int(a.view(np.uint32).max()) >= self.vocab_size:
            raise ValueError('token id outside [0, %d)' % self.vocab_size)

    def __call__(self, inputs, past=None, attention_mask=None, token_type_ids=None, position_ids=None,
                 input_embeddings=None, use_cache=True, training=False):
        """Transformer.call (transformer.py:696-833) -> (logits [B,T,V] float32, presents[, all_hidden_states][, all_attentions]).

        `past` = an earlier call's presents (L tensors [2,B,H,Tp,D], or the lazy Presents object): only the last input
        token is used (:735-737), it sits at position Tp (:760-770), its keys/values are appended to `past` (:423-426)
        and the returned presents hold Tp+1 positions.  `training=True` (:916-917) applies dropout with the masks a train
        step at the current optimizer iteration would draw; together with `past` the attention-probability mask is the new
        token's row of the mask over all Tp+1 positions."""
        if input_embeddings is not None:
            # (it cannot work in the reference either: transformer.py:758 casts inputs=None)
            raise NotImplementedError('input_embeddings is never used by the CLI path')
        x = self._ids(inputs)
        past_len, past_ptrs, keep = 0, None, []
        if past is not None:
            x = np.ascontiguousarray(x[:, -1:])                                  # transformer.py:735-737
            past = list(past)
            if len(past) != self.decoder_layers_count:
                raise ValueError('past must hold one tensor per decoder block')
            H, D = self.attention_head_count, self.embedding_size // self.attention_head_count
            keep = [np.ascontiguousarray(np.asarray(p, dtype=np.float32)) for p in past]
            past_len = int(keep[0].shape[-2])
            for p in keep:
                if p.shape != (2, x.shape[0], H, past_len, D):
                    raise ValueError('past tensors must be [2, batch, heads, past_len, head_size]; got %s' % (p.shape,))
            past_ptrs = (C.c_void_p * len(keep))(*[p.ctypes.data for p in keep])
        self._check_ids(x)
        B, T = x.shape
        if past_len + T > self.window_size:
            raise IndexError('position %d outside the wpe table (window_size %d, transformer.py:675-679,786)'
                             % (past_len + T - 1, self.window_size))
        logits = np.empty((B, T, self.vocab_size), np.float32)
        pos = typ = None
        if token_type_ids is not None:                                           # :787-791: a second wte row per token
            typ = self._ids(token_type_ids)
            if past is not None:
                typ = typ[:, -1:]                                                # :741-742
            typ = np.ascontiguousarray(np.broadcast_to(typ.reshape(-1, typ.shape[-1]), (B, T)))
            self._check_ids(typ)
        if position_ids is not None:                                             # :770-773, 784, 786: rows of wpe, [1,T] or [B,T]
            pos = self._ids(position_ids)
            pos = np.ascontiguousarray(np.broadcast_to(pos.reshape(-1, pos.shape[-1]), (B, T)))
            if pos.size and (pos.min() < 0 or pos.max() >= self.window_size):
                raise IndexError('position id outside the wpe table (window_size %d, transformer.py:675-679,786)' % self.window_size)
        amask = None
        if attention_mask is not None:                                           # :774-779, 356-358: [B, past + new keys], 1 = attend
            raw = np.asarray(attention_mask)
            # the reference casts the mask to float32 and adds (1 - mask) * -1e4 (:774-779): a fractional entry is a soft mask there.
            # The C ABI carries 0 / 1 integers, so anything else is refused rather than truncated to "masked".
            if raw.size and not np.all((raw == 0) | (raw == 1)):
                raise ValueError('attention_mask entries must be 0 or 1 (soft masks are not supported by the HIP path)')
            amask = np.ascontiguousarray(raw.astype(np.int32))
            if amask.shape != (B, past_len + T):
                raise ValueError('attention_mask must be [batch, past_len + sequence] = %s; got %s' % ((B, past_len + T), amask.shape))
        attentions, att_ptrs = None, None
        if self.output_attention_weights:                                        # :360-369, 808-809: [B, H, new queries, all keys] per block
            H = self.attention_head_count
            attentions = [np.empty((B, H, T, past_len + T), np.float32) for _ in range(self.decoder_layers_count)]
            att_ptrs = (C.c_void_p * len(attentions))(*[a.ctypes.data for a in attentions])
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.cmp_forward_ex(self._h, x.ctypes.data_as(C.c_void_p), B, T, past_len, past_ptrs, int(bool(training)),
                                            ptr(pos), ptr(typ), ptr(amask), att_ptrs, logits.ctypes.data_as(C.c_void_p)),
                   'cmp_forward_ex')
        gen = C.c_int64()
        _lib.check(self._lib.cmp_forward_generation(self._h, C.byref(gen)), 'cmp_forward_generation')
        outputs = (logits,)
        if use_cache is True:
            outputs += (Presents(self, B, past_len + T, int(gen.value)),)
        if self.output_hidden_states:
            # transformer.py:800-816, 824-825: the input of every decoder block, then the ln_f output -- L + 1 tensors [B, T, E]
            hidden = []
            for i in range(self.decoder_layers_count + 1):
                h = np.empty((B, T, self.embedding_size), np.float32)
                _lib.check(self._lib.cmp_hidden_get_at(self._h, i, B, T, int(gen.value), h.ctypes.data_as(C.c_void_p)),
                           'cmp_hidden_get_at')
                hidden.append(h)
            outputs += (tuple(hidden),)
        if attentions is not None:
            outputs += (tuple(attentions),)                                      # :827-831
        return outputs

    def _fetch_present(self, layer, B, T, generation):
        """presents[layer] = stack([key, value]) [2,B,H,T,D] of the forward pass that produced this Presents object.  Valid
        until the next forward / train step of the model: a read after that raises (never another pass's tensors)."""
        H = self.attention_head_count
        out = np.empty((2, B, H, T, self.embedding_size // H), np.float32)
        _lib.check(self._lib.cmp_present_get_at(self._h, int(layer), B, T, int(generation), out.ctypes.data_as(C.c_void_p)),
                   'cmp_present_get_at')
        return out

    def train_step(self, x, y, learning_rate=None, sync=True):
        """One iteration of transformer.py:914-930: returns (loss, accuracy) of this rank's batch."""
        x, y = self._ids(x), self._ids(y)
        self._check_ids(x); self._check_ids(y)
        B, T = x.shape
        lr = self._learning_rate if learning_rate is None else float(learning_rate)
        loss, acc = C.c_float(), C.c_float()
        _lib.check(self._lib.cmp_train_step(self._h, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), B, T, lr,
                                            C.byref(loss) if sync else None, C.byref(acc) if sync else None), 'cmp_train_step')
        return (loss.value, acc.value) if sync else None

    def train_step_device(self, x_ptr, y_ptr, B, T, learning_rate=None):
        """x_ptr / y_ptr: HIP device pointers to int32 [B,T] (e.g. torch tensor .data_ptr()); no host sync."""
        lr = self._learning_rate if learning_rate is None else float(learning_rate)
        _lib.check(self._lib.cmp_train_step_dev(self._h, C.c_void_p(x_ptr), C.c_void_p(y_ptr), B, T, lr), 'cmp_train_step_dev')

    def train_step_async(self, x, y, learning_rate=None):
        """Submits one train step without waiting for it (ids staged in pinned memory, uploaded on a copy stream behind the
        previous step); returns a ticket for step_metrics().  At most 3 steps are in flight."""
        x, y = self._ids(x), self._ids(y)
        self._check_ids(x); self._check_ids(y)
        B, T = x.shape
        lr = self._learning_rate if learning_rate is None else float(learning_rate)
        ticket = C.c_int64()
        _lib.check(self._lib.cmp_train_step_async(self._h, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), B, T, lr,
                                                  C.byref(ticket)), 'cmp_train_step_async')
        return int(ticket.value)

    def _dataset_handle(self, dataset):
        """The cmp_dataset of a composer_amd.dataset.DeviceDataset in this model's context: its id stream is uploaded on first use
        and stays in HBM until the model is closed."""
        got = self._datasets.get(id(dataset))
        if got is None:
            ids = np.ascontiguousarray(dataset.ids, dtype=np.uint16)
            layout = dataset.layout
            if layout is not None and not isinstance(layout, _lib.EventGrammar):
                layout = layout.to_c()
            h = C.c_void_p()
            _lib.check(self._lib.cmp_dataset_create(self._ctx, ids.ctypes.data_as(C.c_void_p), len(ids),
                                                    C.byref(layout) if layout is not None else None, C.byref(h)), 'cmp_dataset_create')
            got = self._datasets[id(dataset)] = (dataset, h)
        return got[1]

    def train_step_dataset(self, dataset, plan, learning_rate=None):
        """train_step_async with the batch built on the device: `plan` (augment.PLAN_DTYPE [B], or (offset, transpose, stretch)
        triples) names the rows of `dataset` (a DeviceDataset); x and y never exist on the host.  Returns a ticket for
        step_metrics() / step_metrics_ex()."""
        plan = augment.as_plan(plan)
        lr = self._learning_rate if learning_rate is None else float(learning_rate)
        ticket = C.c_int64()
        _lib.check(self._lib.cmp_train_step_dataset(self._h, self._dataset_handle(dataset), plan.ctypes.data_as(C.c_void_p), len(plan),
                                                    int(dataset.W), lr, C.byref(ticket)), 'cmp_train_step_dataset')
        return int(ticket.value)

    def dataset_batch(self, dataset, plan):
        """(x, y, status) of a plan as the device builds them (cmp_dataset_batch): int32 [B, W] twice and [B, 2]; for tests and
        debugging -- composer_amd.augment.build_batch is the same on the host."""
        plan = augment.as_plan(plan)
        B, W = len(plan), int(dataset.W)
        x, y, st = np.empty((B, W), np.int32), np.empty((B, W), np.int32), np.empty((B, 2), np.int32)
        _lib.check(self._lib.cmp_dataset_batch(self._dataset_handle(dataset), plan.ctypes.data_as(C.c_void_p), B, W,
                                               x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p)),
                   'cmp_dataset_batch')
        return x, y, st

    def step_metrics(self, ticket):
        """(loss, accuracy) of the step `ticket` was issued for; blocks until that step (not later ones) has finished."""
        loss, acc = C.c_float(), C.c_float()
        _lib.check(self._lib.cmp_train_metrics_wait(self._h, int(ticket), C.byref(loss), C.byref(acc)), 'cmp_train_metrics_wait')
        return loss.value, acc.value

    def set_train_options(self, clip_norm=0.0, accumulate_steps=1):
        """cmp_train_options: global-norm clipping (0 off, > 0 on, inf measure only) and gradient accumulation (train_step* become
        micro-steps; every `accumulate_steps`-th call updates).  Discards a pending partial group."""
        clip_norm, accumulate_steps, _ = check_train_options(clip_norm, accumulate_steps)
        _lib.check(self._lib.cmp_train_options(self._h, clip_norm, accumulate_steps), 'cmp_train_options')

    def train_options(self):
        """{'clip_norm', 'accumulate_steps', 'pending_micro_steps'} (cmp_train_options_get)."""
        c, k, p = C.c_float(), C.c_int(), C.c_int()
        _lib.check(self._lib.cmp_train_options_get(self._h, C.byref(c), C.byref(k), C.byref(p)), 'cmp_train_options_get')
        return {'clip_norm': c.value, 'accumulate_steps': k.value, 'pending_micro_steps': p.value}

    def grad_stats(self):
        """(norm | None, scale) of the last enqueued step: the global gradient norm and the clip scale applied; None / 1.0 when no
        norm was computed (clipping off, or a micro-step that did not update).  Synchronises like last_metrics."""
        n, sc = C.c_float(), C.c_float()
        _lib.check(self._lib.cmp_train_grad_stats(self._h, C.byref(n), C.byref(sc)), 'cmp_train_grad_stats')
        return (None if n.value != n.value else n.value), sc.value

    def step_metrics_ex(self, ticket):
        """(loss, accuracy, norm | None, scale) of the step `ticket` was issued for (cmp_train_metrics_wait_ex)."""
        loss, acc, n, sc = C.c_float(), C.c_float(), C.c_float(), C.c_float()
        _lib.check(self._lib.cmp_train_metrics_wait_ex(self._h, int(ticket), C.byref(loss), C.byref(acc), C.byref(n), C.byref(sc)),
                   'cmp_train_metrics_wait_ex')
        return loss.value, acc.value, (None if n.value != n.value else n.value), sc.value

    def last_metrics(self):
        loss, acc = C.c_float(), C.c_float()
        _lib.check(self._lib.cmp_train_metrics(self._h, C.byref(loss), C.byref(acc)), 'cmp_train_metrics')
        return loss.value, acc.value

    def synchronize(self):
        _lib.check(self._lib.cmp_sync(self._ctx), 'cmp_sync')

    @property
    def stream(self):
        return self._lib.cmp_ctx_stream(self._ctx)

    def loss_and_grads(self, x, y):
        """forward(training=True)+backward without the optimizer; gradients via get_parameter(name, KIND_GRAD)."""
        x, y = self._ids(x), self._ids(y)
        self._check_ids(x); self._check_ids(y)
        B, T = x.shape
        loss, acc = C.c_float(), C.c_float()
        _lib.check(self._lib.cmp_loss_and_grads(self._h, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), B, T,
                                                C.byref(loss), C.byref(acc)), 'cmp_loss_and_grads')
        return loss.value, acc.value

    def evaluate(self, dataset, verbose=0):
        """model.evaluate(ds) (cli.py:613): mean sparse-CE and token accuracy over all batches."""
        tot, cor, cnt = 0.0, 0, 0
        for x, y in dataset:
            x, y = self._ids(x), self._ids(y)
            self._check_ids(x); self._check_ids(y)
            B, T = x.shape
            ls, c, n = C.c_double(), C.c_int64(), C.c_int64()
            _lib.check(self._lib.cmp_eval_step(self._h, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), B, T,
                                               C.byref(ls), C.byref(c), C.byref(n)), 'cmp_eval_step')
            tot += ls.value; cor += c.value; cnt += n.value
        if cnt == 0:
            return float('nan'), float('nan')
        return tot / cnt, cor / cnt

    def evaluate_dataset(self, dataset, max_windows=None, batch=None, event_ranges=None):
        """One validation pass on the device (cmp_eval_dataset): mean NLL and accuracy over the windows of the fixed grid
        ids[i (W + 1) : (i + 1)(W + 1)], summed per event class.  `dataset`: a DeviceDataset (its stream is uploaded once, through
        _dataset_handle, with its own window size W) or a plain array of uint16 ids (W = window_size; uploaded for this call).
        `max_windows`: the first N windows of the grid only, a deterministic subset, so successive passes are comparable.  `batch`:
        windows per forward pass (default max_batch); the last batch is ragged, no window is dropped.  `event_ranges`: {event type:
        range of ids} (composer_amd.dataset.event_ranges), at most 8 disjoint classes.  Returns an EvalReport.  Read-only for
        everything that lasts; two calls on the same inputs return the same bits."""
        own = None
        if hasattr(dataset, 'ids') and hasattr(dataset, 'W'):
            handle, n, W = self._dataset_handle(dataset), len(dataset.ids), int(dataset.W)
        else:
            ids = np.asarray(dataset)
            if ids.ndim != 1 or (ids.size and (ids.min() < 0 or ids.max() > 65535)):
                raise ValueError('evaluate_dataset: a DeviceDataset or a 1-D array of event ids that fit uint16 is expected')
            ids = np.ascontiguousarray(ids, dtype=np.uint16)
            n, W = len(ids), int(self.window_size)
            own = C.c_void_p()
            _lib.check(self._lib.cmp_dataset_create(self._ctx, ids.ctypes.data_as(C.c_void_p), n, None, C.byref(own)), 'cmp_dataset_create')
            handle = own
        try:
            windows = n // (W + 1)
            if max_windows is not None:
                if int(max_windows) < 1:
                    raise ValueError('evaluate_dataset: max_windows = %d must be at least 1' % int(max_windows))
                windows = min(windows, int(max_windows))
            names, classes = [], _lib.EvalClasses()
            for t, interval in (event_ranges or {}).items():
                if len(names) >= 8:
                    raise ValueError('evaluate_dataset: at most 8 event classes')
                classes.lo[len(names)], classes.hi[len(names)] = int(interval.start), int(interval.stop)
                names.append(t)
            classes.n = len(names)
            table = _lib.EvalTable()
            _lib.check(self._lib.cmp_eval_dataset(self._h, handle, 0, windows, W, int(batch or self._max_batch), C.byref(classes),
                                                  C.byref(table)), 'cmp_eval_dataset')
        finally:
            if own is not None:
                self._lib.cmp_dataset_destroy(own)
        return EvalReport(names, list(table.nll), list(table.count), list(table.correct), windows=windows)

    # ------------------------------------------------------------------ scoring
    def _score_call(self, x, y):
        """cmp_score on one padded batch: (logp, rank, entropy), each [B, T]."""
        x, y = self._ids(x), self._ids(y)
        self._check_ids(x)
        B, T = x.shape
        logp, rank, ent = np.empty((B, T), np.float32), np.empty((B, T), np.int32), np.empty((B, T), np.float32)
        _lib.check(self._lib.cmp_score(self._h, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), B, T,
                                       logp.ctypes.data_as(C.c_void_p), rank.ctypes.data_as(C.c_void_p),
                                       ent.ctypes.data_as(C.c_void_p)), 'cmp_score')
        return logp, rank, ent

    def score(self, sequences, slide_keep=None):
        """How likely are these event sequences under the model?  `sequences`: one sequence of ids, or a list of (ragged)
        sequences; returns one `SequenceScore`, or a list of them.  Every position n >= 1 of a sequence s is scored against the
        context s[n - c(n) : n], c = slide_context_length(n, window_size, slide_keep) (default window_size // 2): the plain causal
        pass up to window_size, the conditioning of 'kv-slide' generation past it (`score_windows`).  logp / rank / entropy are
        reduced from the fp32 logits on the device (cmp_score: temperature 1, no filter, no grammar); only [B, T] arrays come back.
        A sequence of length 1 yields empty arrays."""
        keep = self._slide_keep(slide_keep)
        single = len(sequences) > 0 and np.ndim(sequences[0]) == 0
        seqs = [sequences] if single else list(sequences)
        for k, s in enumerate(seqs):
            a = np.asarray(s)
            if a.size and (a.min() < 0 or a.max() >= self.vocab_size):
                raise ValueError('score: sequence %d holds an id outside [0, %d)' % (k, self.vocab_size))
        out = score_sequences(self._score_call, seqs, self.window_size, keep, self._max_tokens)
        return out[0] if single else out

    # ------------------------------------------------------------------ decode (cli.py:659-676)
    def _slide_keep(self, slide_keep):
        keep = self.window_size // 2 if slide_keep is None else int(slide_keep)
        slide_context_length(self.window_size + 1, self.window_size, keep)       # the range check
        return keep

    def _set_decode_grammar(self, batched, grammar, banned_ids):
        """cmp_decode_grammar for the chain the next begin call belongs to; with neither argument the chain is switched off again
        only if an earlier call of this object switched it on (a library without the entry point is then never asked for it)."""
        from composer_amd import grammar as gm
        on = getattr(self, '_grammar_on', None)
        if on is None:
            on = self._grammar_on = [False, False]
        if grammar is None and banned_ids is None:
            if on[batched]:
                _lib.check(self._lib.cmp_decode_grammar(self._h, batched, None, None), 'cmp_decode_grammar')
                on[batched] = False
            return
        if grammar is not None and grammar.vocab_size != self.vocab_size:
            raise ValueError('grammar: a layout for %d ids, the model has %d' % (grammar.vocab_size, self.vocab_size))
        words = None
        if banned_ids is not None:
            words = gm.check_static_bans(self.vocab_size, gm.ban_words(self.vocab_size, banned_ids), grammar)
        cg = grammar.to_c() if grammar is not None else None
        _lib.check(self._lib.cmp_decode_grammar(self._h, batched, C.byref(cg) if cg is not None else None,
                                                words.ctypes.data_as(C.c_void_p) if words is not None else None),
                   'cmp_decode_grammar')
        on[batched] = True

    def decode_grammar_state(self, batched=False, row=0):
        """`composer_amd.grammar.GrammarState` of a row after its latest id (cmp_decode_grammar_state): the sounding pitches, the
        pedal and the summed time shifts of prompt ++ ids so far.  Empty while the chain has no layout."""
        from composer_amd import grammar as gm
        w, ped, ts = (C.c_uint32 * 4)(), C.c_int32(0), C.c_int64(0)
        _lib.check(self._lib.cmp_decode_grammar_state(self._h, 1 if batched else 0, int(row), C.byref(w), C.byref(ped), C.byref(ts)),
                   'cmp_decode_grammar_state')
        bits = np.unpackbits(np.array(list(w), '<u4').view(np.uint8), bitorder='little').astype(bool)
        return gm.GrammarState(bits, bool(ped.value), ts.value)

    # Timed generation asks for its ids in chunks and reads the budget state after each.  32 is a choice, not a measurement: one
    # synchronisation per 32 tokens at about 119 us per token, and at most 31 filler steps behind the end of a row.
    BUDGET_CHUNK = 32

    def _check_decode_budget(self, grammar, banned_ids, duration_steps, max_polyphony):
        """(time steps, cap) of a generate call, refused from the arguments as cmp_decode_budget and the begin call would refuse
        them (before the chain's configuration is touched)."""
        from composer_amd import grammar as gm
        steps = 0 if duration_steps is None else int(duration_steps)
        cap = int(max_polyphony)
        if duration_steps is not None and steps < 1:
            raise ValueError('duration_steps=%d must be >= 1' % steps)
        if cap < 0:
            raise ValueError('max_polyphony=%d must be >= 0 (0: no cap)' % cap)
        if steps or cap:
            if grammar is None:
                raise ValueError('duration_steps / max_polyphony need a grammar: the layout says which ids shift time and which '
                                 'are notes (rules=0 is enough)')
            if banned_ids is not None:
                gm.TimedRules(grammar, steps, cap).check_static_bans(gm.ban_words(self.vocab_size, banned_ids))
        return steps, cap

    def _set_decode_budget(self, batched, steps, cap):
        """cmp_decode_budget for the chain the next begin call belongs to; without a budget the chain is switched off again only
        if an earlier call of this object switched it on (as _set_decode_grammar)."""
        on = getattr(self, '_budget_on', None)
        if on is None:
            on = self._budget_on = [False, False]
        if steps == 0 and cap == 0:
            if on[batched]:
                _lib.check(self._lib.cmp_decode_budget(self._h, batched, 0, 0), 'cmp_decode_budget')
                on[batched] = False
            return
        _lib.check(self._lib.cmp_decode_budget(self._h, batched, steps, cap), 'cmp_decode_budget')
        on[batched] = True

    def _set_decode_copy_guard(self, batched, copy_guard):
        """cmp_decode_copy_guard for the chain the next begin call belongs to (a `composer_amd.novelty.CopyGuard`, or None: off);
        switched off again only if an earlier call of this object switched it on (as _set_decode_grammar).  The object holds the
        guard -- and through it the corpus's dataset -- for as long as it is attached."""
        held = getattr(self, '_copy_guard', None)
        if held is None:
            held = self._copy_guard = [None, None]
        if copy_guard is None:
            if held[batched] is not None:
                _lib.check(self._lib.cmp_decode_copy_guard(self._h, batched, None, None), 'cmp_decode_copy_guard')
                held[batched] = None
            return
        ds, opts = copy_guard.attach_args()            # (opens the corpus's dataset again if it was closed since)
        key = (copy_guard, copy_guard.corpus.generation)
        if held[batched] is not None and held[batched][0] is key[0] and held[batched][1] == key[1]:
            return                                     # attached already, to this very dataset: the chain keeps its captured graph
        _lib.check(self._lib.cmp_decode_copy_guard(self._h, batched, ds, C.byref(opts)), 'cmp_decode_copy_guard')
        held[batched] = key

    def decode_copy_guard_state(self, batched=False, row=0):
        """banned_columns of a row after its latest id (cmp_decode_copy_guard_state): the columns the copy rule banned, summed over
        the row's draws in PLAY, that the static vector had not.  0 on a chain begun without a guard."""
        n = C.c_int64(0)
        _lib.check(self._lib.cmp_decode_copy_guard_state(self._h, 1 if batched else 0, int(row), C.byref(n)),
                   'cmp_decode_copy_guard_state')
        return n.value

    def decode_budget_state(self, batched=False, row=0):
        """(steps_left, phase, done_at) of a row after its latest id (cmp_decode_budget_state): the steps of its time budget
        still to go, `composer_amd.grammar.PLAY` / `ENDING` / `DONE`, and the number of ids it had produced when it became DONE
        (-1 before; ids from there on are filler).  (0, PLAY, -1) while the chain has no budget."""
        left, ph, da = C.c_int64(0), C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.cmp_decode_budget_state(self._h, 1 if batched else 0, int(row), C.byref(left), C.byref(ph), C.byref(da)),
                   'cmp_decode_budget_state')
        return left.value, ph.value, da.value

    def _timed_steps(self, length):
        """`length` ids of the batch-1 chain at most, BUDGET_CHUNK per call, until the row is done: the ids up to done_at."""
        out = np.empty(length, np.int32)
        n = 0
        while n < length:
            c = min(self.BUDGET_CHUNK, length - n)
            part = np.empty(c, np.int32)
            _lib.check(self._lib.cmp_decode_steps(self._h, c, part.ctypes.data_as(C.c_void_p)), 'cmp_decode_steps')
            out[n:n + c] = part
            n += c
            done_at = self.decode_budget_state()[2]
            if done_at >= 0:
                return out[:done_at].copy()
        return out

    def _timed_batch_steps(self, B, length):
        """The same for the batched chain, until every row is done: a list of B arrays, row b cut at its done_at."""
        out = np.empty((B, length), np.int32)
        n = 0
        while n < length:
            c = min(self.BUDGET_CHUNK, length - n)
            part = np.empty((B, c), np.int32)
            _lib.check(self._lib.cmp_decode_batch_steps(self._h, c, part.ctypes.data_as(C.c_void_p)), 'cmp_decode_batch_steps')
            out[:, n:n + c] = part
            n += c
            if all(self.decode_budget_state(True, b)[2] >= 0 for b in range(B)):      # (stops reading at the first unfinished row)
                break
        done = [self.decode_budget_state(True, b)[2] for b in range(B)]
        return [out[b, :(d if d >= 0 else n)].copy() for b, d in enumerate(done)]

    def generate(self, prompt_ids, length, temperature=1.0, mode='kv', seed=None, slide_keep=None, top_k=0, top_p=1.0,
                 grammar=None, banned_ids=None, duration_steps=None, max_polyphony=0, copy_guard=None):
        """Returns `length` generated ids.  mode 'literal' restates cli.py:663-676 as written (no `past`),
        mode 'kv' is model(x, past=presents).  temperature <= 0 -> greedy argmax.  mode 'kv-slide' is 'kv' that goes on past
        window_size: when the cache is full the last `slide_keep` tokens (default window_size // 2) are re-encoded from position 0
        and decoding continues on them (`slide_context_length` is the context every id is drawn from).
        top_k / top_p: truncated sampling on the device (0 / 1.0: off) -- every id is drawn from the columns
        `sampling_keep_set(logits, temperature, top_k, top_p)` names, renormalised.
        grammar (a `composer_amd.grammar.EventGrammar`) / banned_ids (ids, a bool mask or ban words): event-grammar decoding -- ids
        the grammar bans in the state of prompt ++ ids so far, and the banned ids, are never drawn (they read -inf, before top_k /
        top_p rank the row and for the greedy argmax too).  Default: off, the sampler as it was.
        duration_steps / max_polyphony: timed generation (cmp_decode_budget; both need `grammar`, rules 0 is enough).  With
        duration_steps the generated part lasts exactly that many time steps and ends with every note released and the pedal
        up: `length` is then the cap on events, the ids come back as soon as the row is done (fewer than `length` of them), or
        all `length` ids when the cap came first (`decode_budget_state()[2]` is then -1).  max_polyphony: never more than that
        many pitches sounding at once (0: no cap).
        copy_guard (`Corpus.guard(max_copy, ...)`): no draw extends a verbatim match of prompt ++ ids with the corpus past max_copy
        events (cmp_decode_copy_guard; TIME_SHIFT ids are exempt); `decode_copy_guard_state()` counts the columns it banned."""
        p = np.ascontiguousarray(np.asarray(prompt_ids, dtype=np.int32).reshape(-1))
        top_k, top_p = check_sampling(top_k, top_p)
        steps, cap = self._check_decode_budget(grammar, banned_ids, duration_steps, max_polyphony)
        self._set_decode_grammar(0, grammar, banned_ids)
        self._set_decode_budget(0, steps, cap)
        self._set_decode_copy_guard(0, copy_guard)
        filters = top_k != 0 or top_p != 1.0
        if mode == 'kv-slide':
            keep = self._slide_keep(slide_keep)
            if filters:
                _lib.check(self._lib.cmp_decode_begin_ex(self._h, p.ctypes.data_as(C.c_void_p), len(p), _lib.DECODE_KV, keep,
                                                         float(temperature), top_k, top_p,
                                                         int(self.seed if seed is None else seed)), 'cmp_decode_begin_ex')
            else:
                _lib.check(self._lib.cmp_decode_begin_slide(self._h, p.ctypes.data_as(C.c_void_p), len(p), keep, float(temperature),
                                                            int(self.seed if seed is None else seed)), 'cmp_decode_begin_slide')
            if steps:
                return self._timed_steps(int(length))
            out = np.empty(length, np.int32)
            _lib.check(self._lib.cmp_decode_steps(self._h, int(length), out.ctypes.data_as(C.c_void_p)), 'cmp_decode_steps')
            return out
        if slide_keep is not None:
            raise ValueError("slide_keep goes with mode='kv-slide'")
        m = {'literal': _lib.DECODE_LITERAL, 'reference-literal': _lib.DECODE_LITERAL, 'kv': _lib.DECODE_KV,
             'kv-cache': _lib.DECODE_KV}[mode]
        if m == _lib.DECODE_KV and len(p) + length - 1 > self.window_size:
            raise IndexError('prompt_len + length - 1 = %d exceeds window_size %d (wpe rows, transformer.py:675-679,786)'
                             % (len(p) + length - 1, self.window_size))
        if filters:
            _lib.check(self._lib.cmp_decode_begin_ex(self._h, p.ctypes.data_as(C.c_void_p), len(p), m, 0, float(temperature), top_k,
                                                     top_p, int(self.seed if seed is None else seed)), 'cmp_decode_begin_ex')
        else:
            _lib.check(self._lib.cmp_decode_begin(self._h, p.ctypes.data_as(C.c_void_p), len(p), m, float(temperature),
                                                  int(self.seed if seed is None else seed)), 'cmp_decode_begin')
        if steps:
            return self._timed_steps(int(length))
        out = np.empty(length, np.int32)
        _lib.check(self._lib.cmp_decode_steps(self._h, int(length), out.ctypes.data_as(C.c_void_p)), 'cmp_decode_steps')
        return out

    def generate_batch(self, prompts, length, temperature=1.0, mode='kv', seed=None, slide_keep=None, top_k=0, top_p=1.0,
                       grammar=None, banned_ids=None, duration_steps=None, max_polyphony=0, copy_guard=None):
        """B independent sequences decoded together: returns int32 [B, length].  `prompts` is a list of id sequences (ragged
        rows allowed); row b samples with seed + b, so it equals `generate(prompts[b], length, seed=seed + b)` in its first id
        and depends on nothing but its own prompt and seed.  Modes, temperature and slide_keep as in `generate`; in 'kv-slide'
        every row slides on its own length.  temperature, top_k and top_p are each a scalar (every row) or a sequence of B values
        (row b's own): a row's ids depend on its own three only.  grammar / banned_ids as in `generate`: one grammar and one ban
        vector for all rows, the state each row's own.
        duration_steps / max_polyphony as in `generate`: one budget for all rows, each row charged from its own prompt's time.
        With duration_steps the result is a list of B arrays of unequal length (row b cut where it was done, or all `length`
        ids when the cap came first); decoding stops when every row is done, so a finished row costs at most the filler steps
        until the slowest row ends (plus the rest of that chunk of BUDGET_CHUNK steps).
        copy_guard as in `generate`: one guard for all rows, history and counter each row's own."""
        steps, cap = self._check_decode_budget(grammar, banned_ids, duration_steps, max_polyphony)
        self._set_decode_grammar(1, grammar, banned_ids)
        self._set_decode_budget(1, steps, cap)
        self._set_decode_copy_guard(1, copy_guard)
        rows = [np.asarray(p, dtype=np.int64).reshape(-1) for p in prompts]
        slide = mode == 'kv-slide'
        if slide:
            keep = self._slide_keep(slide_keep)
        elif slide_keep is not None:
            raise ValueError("slide_keep goes with mode='kv-slide'")
        m = {'literal': _lib.DECODE_LITERAL, 'reference-literal': _lib.DECODE_LITERAL, 'kv': _lib.DECODE_KV,
             'kv-cache': _lib.DECODE_KV, 'kv-slide': _lib.DECODE_KV}[mode]
        if not 1 <= len(rows) <= 256:
            raise ValueError('generate_batch: %d rows; 1 to 256 rows are supported' % len(rows))
        for b, r in enumerate(rows):
            if len(r) == 0:
                raise ValueError('generate_batch: row %d is empty' % b)
            if r.min() < 0 or r.max() >= self.vocab_size:
                raise ValueError('generate_batch: row %d holds an id outside [0, %d)' % (b, self.vocab_size))
            if m == _lib.DECODE_KV and not slide and len(r) + length - 1 > self.window_size:
                raise IndexError('generate_batch: row %d: prompt_len + length - 1 = %d exceeds window_size %d (wpe rows, '
                                 'transformer.py:675-679,786)' % (b, len(r) + length - 1, self.window_size))
        B, ld = len(rows), max(len(r) for r in rows)
        buf = np.zeros((B, ld), np.int32)
        for b, r in enumerate(rows):
            buf[b, :len(r)] = r
        lens = np.array([len(r) for r in rows], np.int32)

        def per_row(v, name, dtype):
            if np.ndim(v) == 0:
                return np.full(B, v, dtype)
            a = np.asarray(v).reshape(-1)
            if a.size != B:
                raise ValueError('generate_batch: %s holds %d values for %d rows' % (name, a.size, B))
            return np.ascontiguousarray(a.astype(dtype))
        if np.ndim(temperature) or np.ndim(top_k) or np.ndim(top_p) or top_k != 0 or top_p != 1.0:
            tk = np.atleast_1d(np.asarray(top_k)).reshape(-1)
            tp = np.atleast_1d(np.asarray(top_p)).reshape(-1)
            for k in tk:
                check_sampling(k, 1.0)
            for q in tp:
                check_sampling(0, q)
            ta, ka, pa = per_row(temperature, 'temperature', np.float32), per_row(top_k, 'top_k', np.int32), per_row(top_p, 'top_p', np.float32)
            _lib.check(self._lib.cmp_decode_batch_begin_ex(self._h, buf.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), B,
                                                           ld, m, keep if slide else 0, ta.ctypes.data_as(C.c_void_p),
                                                           ka.ctypes.data_as(C.c_void_p), pa.ctypes.data_as(C.c_void_p),
                                                           int(self.seed if seed is None else seed)),
                       'cmp_decode_batch_begin_ex')
        elif slide:
            _lib.check(self._lib.cmp_decode_batch_begin_slide(self._h, buf.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p),
                                                              B, ld, keep, float(temperature),
                                                              int(self.seed if seed is None else seed)),
                       'cmp_decode_batch_begin_slide')
        else:
            _lib.check(self._lib.cmp_decode_batch_begin(self._h, buf.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), B,
                                                        ld, m, float(temperature), int(self.seed if seed is None else seed)),
                       'cmp_decode_batch_begin')
        self._decode_batch_rows = B
        if steps:
            return self._timed_batch_steps(B, int(length))
        out = np.empty((B, length), np.int32)
        _lib.check(self._lib.cmp_decode_batch_steps(self._h, int(length), out.ctypes.data_as(C.c_void_p)), 'cmp_decode_batch_steps')
        return out

    def decode_slide_stats(self, batched=False):
        """(rows re-encoded by slides, forward passes run for them) since the chain's last begin (cmp_decode_slide_stats)."""
        rs, fc = C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib.cmp_decode_slide_stats(self._h, 1 if batched else 0, C.byref(rs), C.byref(fc)), 'cmp_decode_slide_stats')
        return rs.value, fc.value

    def decode_logits(self):
        """float32 [V]: the logits the latest per-token step of the batch-1 decode drew its id from (cmp_decode_logits_get)."""
        out = np.empty(self.vocab_size, np.float32)
        _lib.check(self._lib.cmp_decode_logits_get(self._h, out.ctypes.data_as(C.c_void_p)), 'cmp_decode_logits_get')
        return out

    def decode_batch_logits(self):
        """float32 [B, V] after `generate_batch`: the logits its last per-token step drew every row's id from
        (cmp_decode_batch_logits_get)."""
        B = getattr(self, '_decode_batch_rows', 0)
        if not B:
            raise _lib.HipLibraryError('decode_batch_logits: call generate_batch first')
        out = np.empty((B, self.vocab_size), np.float32)
        _lib.check(self._lib.cmp_decode_batch_logits_get(self._h, out.ctypes.data_as(C.c_void_p)), 'cmp_decode_batch_logits_get')
        return out

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        sd = {}
        for n in self.parameter_names:
            sd['model/' + n] = self.get_parameter(n)
            sd['optimizer/m/' + n] = self.get_parameter(n, _lib.KIND_ADAM_M)
            sd['optimizer/v/' + n] = self.get_parameter(n, _lib.KIND_ADAM_V)
        sd['optimizer/iter'] = np.int64(self.iterations)
        return sd

    def load_state_dict(self, sd, expect_partial=False):
        for n in self.parameter_names:
            self.set_parameter(n, sd['model/' + n])
            if 'optimizer/m/' + n in sd:
                self.set_parameter(n, sd['optimizer/m/' + n], _lib.KIND_ADAM_M)
                self.set_parameter(n, sd['optimizer/v/' + n], _lib.KIND_ADAM_V)
            elif not expect_partial:
                raise KeyError('optimizer slot for ' + n)
        if 'optimizer/iter' in sd:
            self.iterations = int(sd['optimizer/iter'])

    def load_from_checkpoint(self, restoredir):
        """BaseModel.load_from_checkpoint (reference composer/models/__init__.py:66-90): restores the latest
        checkpoint in `restoredir` (model only, expect_partial); logs and exits(1) on failure."""
        try:
            mgr = ckpt.CheckpointManager(restoredir, max_to_keep=None)
            if mgr.latest_checkpoint is None:
                raise FileNotFoundError('no checkpoint in ' + str(restoredir))
            sd, _meta = ckpt.load(mgr.latest_checkpoint)
            self.load_state_dict(sd, expect_partial=True)
            logging.info('Model restored from \'{}\'.'.format(mgr.latest_checkpoint))
        except Exception:
            logging.error('Failed to restore model from \'{}\'.'.format(restoredir))
            exit(1)

    # ------------------------------------------------------------------ train loop (transformer.py:846-960)
    def train(self, dataset, input_shape, logdir, restoredir=None, epochs=None, learning_rate=1e-3,
              save_frequency_mode=ModelSaveFrequencyMode.EPOCH, save_frequency=1, max_checkpoints=1,
              show_progress_bar=True, max_steps=None, checkpoint_format='npz', clip_norm=0.0, accumulate_steps=1, warmup_steps=0,
              eval_dataset=None, eval_freq=0, eval_max_windows=None, early_stop_patience=0, keep_best=False, eval_event_ranges=None):
        """clip_norm / accumulate_steps: set_train_options; warmup_steps: warmup_lr.  With accumulate_steps = k > 1 every dataset batch is
        a micro-batch: `step`, max_steps and save_frequency count OPTIMISER steps, the logged loss / accuracy of a step are the means
        over its k micro-batches, a group may span an epoch boundary, checkpoints are written at group boundaries only and a partial
        group left at the end is discarded.

        Validation (eval_dataset with eval_freq > 0; off by default, and then nothing here differs): every eval_freq optimiser steps,
        where a checkpoint save would drain the pipeline, and once more at the end of the run if its last step was not evaluated,
        evaluate_dataset runs over eval_dataset (the first eval_max_windows windows) and `val_loss`, `val_accuracy` and one
        `val_nll/<class>` per event class with events (eval_event_ranges: {class name: range of ids}) are logged at the step.  keep_best:
        the state with the lowest val_loss so far is kept in <logdir>/best/ (one checkpoint, meta {'step', 'epoch', 'val_loss'}); the
        rolling checkpoints are untouched.  early_stop_patience = P > 0: after P passes in a row without a lower val_loss the loop
        ends as max_steps ends it.  The ValidationTracker's state travels in every npz checkpoint's meta ('validation'), so a restored
        run continues the count.  Data-parallel: every rank runs the pass, rank 0 logs, saves and decides (exchange_verdict)."""
        clip_norm, k, warmup_steps = check_train_options(clip_norm, accumulate_steps, warmup_steps)
        eval_freq, eval_max_windows, early_stop_patience, keep_best = check_eval_options(eval_freq, eval_max_windows, early_stop_patience,
                                                                                       keep_best)
        validate = eval_dataset is not None and eval_freq > 0
        if (early_stop_patience or keep_best) and not validate:
            raise ValueError('early_stop_patience / keep_best need an eval_dataset')
        tracker = ValidationTracker(early_stop_patience) if validate else None
        if clip_norm != 0.0 or k != 1 or hasattr(self._lib, 'cmp_train_options'):   # (an older library as the other arm of an A/B lacks it)
            self.set_train_options(clip_norm, k)
        clip_on = clip_norm > 0.0
        logdir = Path(logdir) if logdir is not None else None
        if restoredir is not None:
            logdir = Path(restoredir)                                            # :884-885
        rank = self._dp[0] if self._dp else 0
        manager = ckpt.CheckpointManager(logdir, max_to_keep=max_checkpoints, format=checkpoint_format)   # :890-891
        step, epoch = 1, 1
        if restoredir is not None:                                               # :894-900
            try:
                sd, meta = ckpt.load(manager.latest_checkpoint)
                self.load_state_dict(sd)
                step, epoch = int(meta['step']), int(meta['epoch'])
                if tracker is not None:
                    tracker.load_state(meta.get('validation'))
                logging.info('Model restored from \'{}\'.'.format(manager.latest_checkpoint))
            except Exception:
                logging.error('Failed to restore model from \'{}\'.'.format(restoredir))
                exit(1)
        summary = ckpt.ScalarLog(logdir / 'train') if rank == 0 else None        # :903
        first_step = step
        save_frequency_mode = ModelSaveFrequencyMode(save_frequency_mode)
        history = []

        def save():
            if rank != 0:
                return None
            meta = {'step': step, 'epoch': epoch}
            if tracker is not None:
                meta['validation'] = tracker.state()
            return manager.save(self.state_dict(), meta)

        best_manager = ckpt.CheckpointManager(logdir / 'best', max_to_keep=1, format=checkpoint_format) if keep_best and rank == 0 else None
        last_eval = None                                                         # the step number of the latest validation pass

        def validation_pass(st):
            """The pass after optimiser step `st` (the pipeline is drained); True when the run should stop."""
            nonlocal last_eval
            last_eval = st
            report = self.evaluate_dataset(eval_dataset, max_windows=eval_max_windows, event_ranges=eval_event_ranges)
            is_best, stop = tracker.update(st, report.loss) if rank == 0 else (False, False)
            if self._dp and self._dp[1] > 1:
                is_best, stop = exchange_verdict(self.all_reduce_sum, rank, is_best, stop)
            if rank == 0:
                summary.scalar('val_loss', report.loss, st)
                summary.scalar('val_accuracy', report.accuracy, st)
                for t, (count, nll, _) in report.by_event_type.items():
                    if count:
                        summary.scalar('val_nll/{}'.format(t), nll, st)
                summary.flush()
                if show_progress_bar:
                    print('\n- step {}: val_loss {:.4f} - val_accuracy {:.4f}{}'.format(st, report.loss, report.accuracy,
                                                                                      ' (best)' if is_best else ''))
                if is_best and best_manager is not None:
                    best_manager.save(self.state_dict(), {'step': st, 'epoch': epoch, 'val_loss': report.loss})
                    if (logdir / 'config.yml').exists():                         # a model directory of its own: generate / score / evaluate
                        shutil.copyfile(logdir / 'config.yml', logdir / 'best' / 'config.yml')
                if stop:
                    logging.info('Early stop at step {}: val_loss {:.6f} has not improved on the best {:.6f} at step {} for {} passes.'.format(
                        st, report.loss, tracker.best if tracker.best is not None else float('nan'), tracker.best_step, tracker.bad_passes))
            return stop

        done = False
        group = []                                                               # (loss, accuracy) of the retired micro-steps of the open group
        micro = 0                                                                # micro-steps submitted into the open group
        while (epochs is None or epoch < epochs) and not done:                   # :907 (epoch starts at 1)
            logging.info('Epoch {}'.format(epoch if epochs is None else '{}/{}'.format(epoch, epochs)))
            ep_loss, ep_correct, ep_n, t0 = 0.0, 0.0, 0, time.time()
            # The device runs up to two steps ahead of this loop: step s is submitted (ids uploaded on the copy stream behind
            # step s-1) and the metrics of step s-1 are read and logged while s computes.  Logged values, their step numbers
            # and the checkpoint contents are those of the reference's synchronous loop (a save first drains the pipeline).
            pending = []                                                         # [(ticket, step number, lr, last micro-step of its group)]
            ep_batches = 0

            def retire(upto):
                nonlocal ep_loss, ep_correct
                while len(pending) > upto:
                    tk, st, lr, last = pending.pop(0)
                    if k == 1 and not clip_on:
                        loss, acc = self.step_metrics(tk)
                    else:                                                        # means over the micro-batches; the last one holds the norm
                        loss, acc, norm, _ = self.step_metrics_ex(tk)
                        group.append((loss, acc))
                        if not last:
                            continue
                        loss, acc = sum(v[0] for v in group) / len(group), sum(v[1] for v in group) / len(group)
                        del group[:]
                    ep_loss += loss; ep_correct += acc
                    history.append((st, loss, acc))
                    if summary:
                        summary.scalar('loss', loss, st)                         # :933-936
                        summary.scalar('accuracy', acc, st)
                        if clip_on:
                            summary.scalar('grad_norm', float('nan') if norm is None else norm, st)
                        if warmup_steps:
                            summary.scalar('learning_rate', lr, st)
                    if show_progress_bar and rank == 0 and (st % 10 == 1):
                        print('\r- loss: {:.4f} - accuracy: {:.4f}'.format(loss, acc), end='', flush=True)   # :939

            for batch in dataset:                                                # :914
                lr = warmup_lr(learning_rate, step, warmup_steps)
                micro += 1
                ep_batches += 1
                if isinstance(batch, DeviceBatch):                               # built on the device from its plan
                    ticket = self.train_step_dataset(batch.dataset, batch.plan, lr)
                else:
                    ticket = self.train_step_async(batch[0], batch[1], lr)
                pending.append((ticket, step, lr, micro == k))
                retire(1)
                if micro < k:                                                    # a micro-step that does not update: no optimiser step yet
                    continue
                micro = 0
                ep_n += 1
                if validate and step % eval_freq == 0:
                    retire(0)
                    done = validation_pass(step)
                if save_frequency_mode == ModelSaveFrequencyMode.GLOBAL_STEP and step % save_frequency == 0:
                    retire(0)
                    path = save()                                                # :941-943
                    if path and show_progress_bar:
                        print('\nSaved checkpoint for step {} at {}.'.format(step, path))
                step += 1                                                        # :945
                if done or (max_steps is not None and step - first_step >= max_steps):
                    done = True
                    break
            retire(0)
            if ep_batches == 0:
                logging.error('The dataset yielded no batches.')
                break
            last_epoch = done or (epochs is not None and epoch + 1 >= epochs)
            if validate and last_epoch and step > first_step and last_eval != step - 1:
                validation_pass(step - 1)                                        # the end of the run: its last step, if not evaluated yet
            if summary and ep_n:
                summary.scalar('epoch_loss', ep_loss / ep_n, epoch)              # :949-951
                summary.scalar('epoch_accuracy', ep_correct / ep_n, epoch)
            if save_frequency_mode == ModelSaveFrequencyMode.EPOCH and epoch % save_frequency == 0:
                path = save()                                                    # :953-955
                if path and show_progress_bar:
                    print('\nSaved checkpoint for epoch {} at {}.'.format(epoch, path))
            epoch += 1                                                           # :960
        if micro:
            logging.info('Discarding a partial group of {} micro-batch(es) (accumulate_steps {}).'.format(micro, k))
            self.set_train_options(clip_norm, k)
        if summary:
            summary.close()
        return history
