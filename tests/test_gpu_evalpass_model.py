"""-m gpu: cmp_eval_dataset / Transformer.evaluate_dataset against the float64 oracle, on the gA golden configuration of
tests/test_gpu_score_model.py (V 390, E 64, H 4, L 2, window_size 16, weight matrices x 12, dropout 0).

Streams.  UNIFORM: 17 * 37 + 5 ids uniform in [0, 390), default_rng(11): 37 windows, 592 rows, the 5 trailing ids belong to no window;
batch 8, so the last batch holds 5 windows.  Computed on the CPU from the oracle before the values were fixed: 0 of 592 rows
undecidable, 2 correct, class counts 203 / 182 / 47 / 156 / 2 / 2.  GREEDY: 12 windows built one by one, every next id with probability
1/2 the oracle's own argmax of the context so far (default_rng(3)), else uniform: about half the rows correct (CPU: see
test_greedy_stream_exercises_correct).

Bounds.  The project holds fp32 logits to 1e-4 of the oracle, so per row |nll - ref| <= 2e-4 + 1e-5 ref (test_gpu_score_model.py); per
class that is summed: |nll_sum - ref| <= count (2e-4 + 1e-5 ref / count).  count is exact.  A row is decided correct when no other
column comes within 2e-4 of the target's logit from below, decided wrong when another column exceeds it by more than 2e-4; `correct`
must lie between the rows decided correct and the rows not decided wrong, and at most 2 % of the rows may be undecidable."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import golden, transformer_oracle as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
W = 16
SCALE = 12.0
TOL_Z = 2e-4
BATCH = 8
N_WINDOWS = 37
NAMES = ("NOTE_ON", "NOTE_OFF", "VELOCITY", "TIME_SHIFT", "SUSTAIN_ON", "SUSTAIN_OFF")


def setup():
    g = golden.load(os.path.join(HERE, "golden", "transformer_gA.npz"))
    V, E, H, L = [int(v) for v in g["cfg"]][:4]
    params = {k[6:]: g[k].astype(np.float64) for k in g.files if k.startswith("param:")}
    params["wpe/embeddings"] = params["wpe/embeddings"][:W]
    kinds = {n: kind for n, _, kind in O.param_specs(V, E, W, L)}
    params = {n: (v * SCALE if kinds[n] not in ("ones", "zeros") else v).astype(np.float32) for n, v in params.items()}
    return (V, E, H, L), params


def make_model(dims, params, dtype="fp32", max_batch=BATCH, dropout=0.0):
    from composer_amd.transformer import Transformer
    V, E, H, L = dims
    m = Transformer(V, E, W, L, H, attention_dropout_rate=dropout, residual_dropout_rate=dropout, dtype=dtype, seed=0, max_batch=max_batch,
                    max_seq=W)
    m.set_weights(params)
    return m


def event_ranges():
    from composer_amd import dataset as ds
    return ds.event_ranges(ds.event_value_ranges(10, 100, 32))


def uniform_stream():
    return np.random.default_rng(11).integers(0, 390, 17 * N_WINDOWS + 5).astype(np.uint16)


def greedy_stream(orc, windows=12, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(windows):
        w = [int(rng.integers(0, 390))]
        for _ in range(W):
            z = np.asarray(orc.forward(np.asarray(w)[None])[0][0, -1], np.float64)
            w.append(int(np.argmax(z)) if rng.random() < 0.5 else int(rng.integers(0, 390)))
        out += w
    return np.asarray(out, np.uint16)


def oracle_table(orc, ids, ranges):
    """Per class: float64 nll sum, count, rows decided correct, rows not decided wrong; and the undecidable rows of the stream."""
    n = len(ids) // (W + 1)
    k = len(ranges)
    nll, count, lo, hi = np.zeros(k + 1), np.zeros(k + 1, np.int64), np.zeros(k + 1, np.int64), np.zeros(k + 1, np.int64)
    undecidable = 0
    for i in range(n):
        w = ids[i * (W + 1):(i + 1) * (W + 1)].astype(np.int64)
        z = np.asarray(orc.forward(w[None, :W])[0][0], np.float64)
        for t in range(W):
            y = int(w[t + 1])
            c = next((j for j, r in enumerate(ranges.values()) if r.start <= y < r.stop), k)
            mx = z[t].max()
            nll[c] += (mx + np.log(np.exp(z[t] - mx).sum())) - z[t, y]
            count[c] += 1
            gap = z[t, y] - np.delete(z[t], y).max()
            lo[c] += gap > TOL_Z
            hi[c] += gap >= -TOL_Z
            undecidable += abs(gap) <= TOL_Z
    return nll, count, lo, hi, undecidable


@pytest.fixture(scope="module")
def env():
    dims, params = setup()
    V, E, H, L = dims
    orc = O.OracleTransformer(O.Config(V, E, W, L, H), {k: v.astype(np.float64) for k, v in params.items()})
    m = make_model(dims, params)
    ids = uniform_stream()
    ref = oracle_table(orc, ids, event_ranges())
    yield dims, params, orc, m, ids, ref
    m.close()


def check_against_oracle(report, ref, rows):
    nll, count, lo, hi, undecidable = ref
    assert undecidable <= 0.02 * rows, (undecidable, rows)
    assert report.count == count.tolist() and report.events == rows
    worst = 0.0
    for c in range(len(count)):
        lim = count[c] * (2e-4 + 1e-5 * (nll[c] / count[c] if count[c] else 0.0))
        err = abs(report.nll[c] - nll[c])
        worst = max(worst, err / lim if lim else (0.0 if err == 0 else np.inf))
        assert err <= lim, (c, report.nll[c], nll[c], lim)
        assert lo[c] <= report.correct[c] <= hi[c], (c, report.correct[c], int(lo[c]), int(hi[c]))
    return worst


def test_uniform_stream_matches_the_oracle(env):
    dims, params, orc, m, ids, ref = env
    rep = m.evaluate_dataset(ids, batch=BATCH, event_ranges=event_ranges())
    worst = check_against_oracle(rep, ref, N_WINDOWS * W)
    print("\n[evalpass-oracle] uniform: worst |nll_sum - ref| / bound %.3f, loss %.6f (oracle %.6f), correct %d, undecidable %d"
          % (worst, rep.loss, ref[0].sum() / ref[1].sum(), sum(rep.correct), ref[4]))
    assert ref[1].tolist() == [203, 182, 47, 156, 2, 2, 0] and ref[4] == 0 and int(ref[2].sum()) == int(ref[3].sum()) == 2
    assert rep.windows == N_WINDOWS and rep.other[0] == 0
    by = rep.by_event_type
    assert [by[t][0] for t in event_ranges()] == [203, 182, 47, 156, 2, 2]
    assert rep.loss == pytest.approx(ref[0].sum() / ref[1].sum(), abs=2e-4 + 1e-5 * rep.loss)
    # a second pass: the same bits
    again = m.evaluate_dataset(ids, batch=BATCH, event_ranges=event_ranges())
    assert again.nll == rep.nll and again.count == rep.count and again.correct == rep.correct
    # no classes: everything in slot 0, the same rows
    flat = m.evaluate_dataset(ids, batch=BATCH)
    assert flat.count == [N_WINDOWS * W] and flat.correct == [sum(rep.correct)]
    assert flat.nll[0] == pytest.approx(sum(rep.nll), rel=1e-12)


def test_greedy_stream_exercises_correct(env):
    dims, params, orc, m, _, _ = env
    ids = greedy_stream(orc)
    ref = oracle_table(orc, ids, event_ranges())
    rows = 12 * W
    rep = m.evaluate_dataset(ids, batch=5, event_ranges=event_ranges())      # 5 + 5 + 2 windows
    worst = check_against_oracle(rep, ref, rows)
    print("\n[evalpass-oracle] greedy: worst / bound %.3f, correct %d of %d (oracle interval %d .. %d), undecidable %d"
          % (worst, sum(rep.correct), rows, ref[2].sum(), ref[3].sum(), ref[4]))
    assert 0.35 * rows <= sum(rep.correct) <= 0.65 * rows


def test_loss_agrees_with_evaluate_on_one_row_batches(env):
    dims, params, orc, m, ids, ref = env
    rep = m.evaluate_dataset(ids, batch=BATCH)
    win = ids[:17 * N_WINDOWS].reshape(N_WINDOWS, 17).astype(np.int32)
    loss, acc = m.evaluate([(win[i:i + 1, :-1], win[i:i + 1, 1:]) for i in range(N_WINDOWS)])
    assert abs(rep.loss - loss) <= 2e-4 + 1e-5 * abs(loss), (rep.loss, loss)
    assert rep.accuracy == pytest.approx(acc, abs=1e-12)


def test_bf16_loss_against_the_oracle(env):
    dims, params, orc, m, ids, ref = env
    mb = make_model(dims, params, dtype="bf16")
    rep = mb.evaluate_dataset(ids, batch=BATCH, event_ranges=event_ranges())
    mb.close()
    want = ref[0].sum() / ref[1].sum()
    print("\n[evalpass-bf16] loss %.6f, float64 oracle %.6f" % (rep.loss, want))
    assert rep.count == ref[1].tolist()
    assert abs(rep.loss - want) <= 1e-2 * want, (rep.loss, want)


def test_max_windows_is_the_cut_stream_bit_for_bit(env):
    from composer_amd.dataset import DeviceDataset
    dims, params, orc, m, ids, ref = env
    a = m.evaluate_dataset(ids, max_windows=10, batch=BATCH, event_ranges=event_ranges())
    b = m.evaluate_dataset(ids[:170], batch=BATCH, event_ranges=event_ranges())
    assert a.windows == b.windows == 10 and a.events == 160
    assert a.nll == b.nll and a.count == b.count and a.correct == b.correct
    # a DeviceDataset (uploaded once, kept by the model) gives the bits of the plain array
    dd = DeviceDataset(ids, BATCH, W, shuffle=False)
    c = m.evaluate_dataset(dd, max_windows=10, batch=BATCH, event_ranges=event_ranges())
    assert c.nll == a.nll and c.count == a.count and len(m._datasets) == 1
    assert m.evaluate_dataset(dd, max_windows=1000).windows == N_WINDOWS


def test_refusals_come_before_any_device_work(env):
    from composer_amd import _lib
    from composer_amd.dataset import DeviceDataset
    dims, params, orc, m, ids, ref = env
    dd = DeviceDataset(ids, BATCH, W, shuffle=False)
    h = m._dataset_handle(dd)
    table = _lib.EvalTable()
    call = lambda model, handle, first, n, T, batch, k=None: model._lib.cmp_eval_dataset(
        model._h, handle, first, n, T, batch, C.byref(k) if k is not None else None, C.byref(table))
    assert call(m, h, 0, N_WINDOWS, W, BATCH) == 0
    for args, word in (((0, N_WINDOWS + 1, W, BATCH), "outside the stream"), ((30, 8, W, BATCH), "outside the stream"),
                       ((-1, 2, W, BATCH), "outside the stream"), ((0, 0, W, BATCH), "outside the stream"),
                       ((0, 4, W, BATCH + 1), "max_batch"), ((0, 4, W, 0), "max_batch"), ((0, 4, W + 1, BATCH), "window_size"),
                       ((0, 4, 0, BATCH), "window_size")):
        assert call(m, h, *args) == -1 and word in _lib.last_error(), (args, _lib.last_error())
    k = _lib.EvalClasses()
    k.n, k.lo[0], k.hi[0], k.lo[1], k.hi[1] = 2, 0, 200, 199, 390
    assert call(m, h, 0, 4, W, BATCH, k) == -1 and "overlaps" in _lib.last_error()
    k.n, k.hi[0] = 1, 391
    assert call(m, h, 0, 4, W, BATCH, k) == -1 and "outside the vocabulary" in _lib.last_error()
    k.n = 9
    assert call(m, h, 0, 4, W, BATCH, k) == -1 and "at most 8" in _lib.last_error()
    big = DeviceDataset(np.array([1, 2, 390] * 20, np.uint16), BATCH, W, shuffle=False)            # an id the model does not know
    assert call(m, m._dataset_handle(big), 0, 1, W, BATCH) == -1 and "largest id" in _lib.last_error()
    other = make_model(dims, params)                                                             # a context of its own
    assert call(other, h, 0, 4, W, BATCH) == -1 and "different contexts" in _lib.last_error()
    other.close()
    with pytest.raises(ValueError):
        m.evaluate_dataset(ids, max_windows=0)


def test_a_pass_leaves_the_training_state_alone(env, monkeypatch):
    """A pending accumulation group (accumulate_steps 2, one micro-step submitted) and its ticket still unretired; dropout 0.1.  A pass
    in that state changes nothing a twin model without the pass does not show: parameters, Adam moments, iterations, the pending
    count, the ticket's metrics, and the next step (its loss, and the parameters and moments after its update).  bf16 with
    COMPOSER_DETERMINISTIC=1: the mode whose steps are bitwise reproducible, so the twins are compared bit for bit."""
    from composer_amd import _lib
    monkeypatch.setenv("COMPOSER_DETERMINISTIC", "1")
    dims, params, orc, m0, ids, ref = env
    V = dims[0]
    rng = np.random.default_rng(9)
    xs = rng.integers(0, V, (2, 4, W)).astype(np.int32)
    ys = rng.integers(0, V, (2, 4, W)).astype(np.int32)
    kinds = (_lib.KIND_VALUE, _lib.KIND_ADAM_M, _lib.KIND_ADAM_V)
    snap = lambda m: [{n: m.get_parameter(n, k) for n in m.parameter_names} for k in kinds]
    runs = []
    for with_pass in (False, True):
        m = make_model(dims, params, dtype="bf16", dropout=0.1)
        m.set_train_options(clip_norm=1.0, accumulate_steps=2)
        ticket = m.train_step_async(xs[0], ys[0], 1e-2)
        if with_pass:
            rep = m.evaluate_dataset(ids, batch=BATCH, event_ranges=event_ranges())
            assert rep.events == N_WINDOWS * W and np.isfinite(rep.loss)
        pending, iters = m.train_options()["pending_micro_steps"], m.iterations
        first = m.step_metrics_ex(ticket)
        before = snap(m)
        second = m.step_metrics_ex(m.train_step_async(xs[1], ys[1], 1e-2))
        runs.append((pending, iters, first, before, second, m.iterations, snap(m)))
        m.close()
    a, b = runs
    assert a[0] == b[0] == 1 and a[1] == b[1] == 0 and a[5] == b[5] == 1
    assert a[2] == b[2] and a[4] == b[4], (a[2], b[2], a[4], b[4])
    for sa, sb in ((a[3], b[3]), (a[6], b[6])):
        for ka, kb in zip(sa, sb):
            assert all(np.array_equal(ka[n], kb[n]) for n in ka)
    assert not all(np.array_equal(a[3][0][n], a[6][0][n]) for n in a[3][0])        # the second micro-step did update
