"""-m gpu: the train step fed by a device dataset (cmp_train_step_dataset, Transformer.train_step_dataset, `train --augment-*`)
against the same step fed with host-built batches (cmp_train_step_async): the same losses and the same weights, bit for bit --
x and y are integers and equal, so nothing about the step may differ.

A tiny fp32 model (V 390, E 64, L 2, H 4, W 32, B 4, dropout 0.1); the id stream is the default-layout stream of tests/batch_cases.py.
Every model runs with COMPOSER_DETERMINISTIC=1: the one mode whose steps are bitwise reproducible (no float atomics; the default step
sums its embedding, bias and split-K gradients with float atomics, so even two runs of the SAME entry point differ in the last bits of
the weights), as in the other tests that compare two runs bit for bit."""
import numpy as np
import pytest
import yaml
from click.testing import CliRunner

import batch_cases as bc

pytestmark = pytest.mark.gpu

V, E, L, H, W, B = 390, 64, 2, 4, 32, 4


@pytest.fixture(autouse=True)
def reproducible_steps(monkeypatch):
    monkeypatch.setenv("COMPOSER_DETERMINISTIC", "1")         # read when a model's workspace is allocated: at its first step


def model(seed=7):
    from composer_amd.transformer import Transformer
    return Transformer(V, E, W, L, H, attention_dropout_rate=0.1, residual_dropout_rate=0.1, dtype="fp32", seed=seed, max_batch=B,
                       max_seq=W)


def same_weights(a, b):
    wa, wb = a.get_weights(), b.get_weights()
    assert wa.keys() == wb.keys()
    diff = {k: float(np.abs(wa[k] - wb[k]).max()) for k in wa if not np.array_equal(wa[k], wb[k])}
    assert not diff, diff
    return True


def dataset(**kw):
    from composer_amd import dataset as D
    ids, g = bc.stream("default")
    return D.DeviceDataset(ids, B, W, g, shuffle=True, seed=3, **kw)


def test_identity_plans_are_the_host_cut_windows_bit_for_bit():
    from composer_amd import dataset as D
    ids, _ = bc.stream("default")
    dev, host = model(), model()
    dd, wd = dataset(), D.WindowDataset(ids, B, W, shuffle=True, seed=3)
    n = 0
    for batch, (x, y) in zip(dd, wd):
        la = dev.step_metrics(dev.train_step_dataset(dd, batch.plan, 1e-3))
        lb = host.step_metrics(host.train_step_async(x, y, 1e-3))
        assert la == lb and np.isfinite(la[0])
        n += 1
        if n == 3:
            break
    assert dev.iterations == host.iterations == 3 and same_weights(dev, host)
    dev.close(); host.close()


def test_augmenting_plans_equal_the_host_restatement_fed_to_the_async_step():
    from composer_amd import augment
    dev, host = model(), model()
    dd = dataset(random_crop=True, transpose=6, stretch=0.3)
    plans = [dd.plan(0, i) for i in range(3)]
    every = np.concatenate(plans)
    assert (every["transpose"] != 0).any() and (every["stretch_q10"] != 1024).any() and (every["offset"] % (W + 1) != 0).any()
    x0, y0, st0 = dev.dataset_batch(dd, plans[0])                        # cmp_dataset_batch: the device's batch, read back
    hx, hy, hst = augment.build_batch(dd.ids, dd.layout, plans[0], W)
    assert np.array_equal(x0, hx) and np.array_equal(y0, hy) and np.array_equal(st0, hst)
    # all three steps in flight before the first wait: the plan goes through the ticket's slot, three deep
    ta = [dev.train_step_dataset(dd, p, 1e-3) for p in plans]
    tb = [host.train_step_async(*dd.host_batch(p), 1e-3) for p in plans]
    got, want = [dev.step_metrics_ex(t) for t in ta], [host.step_metrics_ex(t) for t in tb]
    assert got == want and all(np.isfinite(g[0]) for g in got), (got, want)
    assert dev.iterations == host.iterations == 3 and same_weights(dev, host)
    dev.close(); host.close()


def test_the_same_with_accumulation_and_clipping():
    """accumulate_steps = 2, clip_norm = 0.5, three optimiser steps (six plans).

    Measured on the parent's step, fed by cmp_train_step_async with the same host batches in five runs (this model,
    COMPOSER_DETERMINISTIC=1): after the FIRST micro-step of a group every gradient agrees bit for bit; from the second on, 6 to 8 of
    the weight-matrix gradients differ in their last bits between two runs (bf16: wte alone) -- a split-K weight gradient that adds
    into a non-zero G is summed with float atomics in every mode --, and after three optimiser steps all 24 parameters differ: over
    the ten pairs of runs the root mean square of the difference over all weights is 3.05e-10 .. 3.46e-10, its maximum 3.7e-9 ..
    1.6e-8 (the maximum is one element with a tiny gradient, where Adam's g / (|g| + eps) amplifies a last bit, and moves by a factor
    of 16 from pair to pair; the root mean square by 13 %).  So two runs of the reference itself are not bit-equal under accumulation,
    and the weights of such a run are held here to the reference's own run-to-run error instead:
      * everything that IS reproducible is compared bit for bit: the first micro-step's loss, accuracy and all gradients; the
        second micro-step's loss and accuracy (a forward pass on parameters that have not moved yet);
      * after three optimiser steps rms(device-fed - host-fed) <= 4 x rms(host-fed - host-fed again) over all weights: the stable
        statistic of the two, with a margin of 4 over a quantity that varies by 13 % (a reproducible reference, rms 0, makes it
        exact equality).  Device-fed against host-fed measured 3.11e-10 .. 3.78e-10 in fifteen pairs; one row of every batch cut one
        token later gives 6.6e-4, two million times the limit."""
    from composer_amd import _lib
    dd = dataset(random_crop=True, transpose=6, stretch=0.3)
    plans = [dd.plan(0, i) for i in range(6)]

    def run(device_fed):
        m = model()
        m.set_train_options(0.5, 2)
        submit = (lambda p: m.train_step_dataset(dd, p, 1e-3)) if device_fed else (lambda p: m.train_step_async(*dd.host_batch(p), 1e-3))
        metrics = [m.step_metrics_ex(submit(plans[0]))]
        grads = {n: m.get_parameter(n, _lib.KIND_GRAD) for n in m.parameter_names}
        metrics += [m.step_metrics_ex(submit(p)) for p in plans[1:]]
        out = (metrics, grads, m.get_weights(), m.iterations)
        m.close()
        return out
    dev, host, again = run(True), run(False), run(False)
    assert dev[3] == host[3] == 3
    assert dev[0][0] == host[0][0] and dev[0][1][:2] == host[0][1][:2], (dev[0][:2], host[0][:2])
    assert all(np.array_equal(dev[1][n], host[1][n]) for n in host[1]) and any(np.abs(v).max() > 0 for v in host[1].values())
    assert [g[2] is not None for g in dev[0]] == [False, True] * 3 and dev[0][1][3] < 1.0      # the norm on every second step; it binds
    assert all(np.isfinite(g[0]) for g in dev[0])
    flat = lambda w: np.concatenate([w[n].ravel() for n in sorted(w)]).astype(np.float64)
    rms = lambda a, b: float(np.sqrt(np.mean((flat(a) - flat(b)) ** 2)))
    spread, diff = rms(host[2], again[2]), rms(dev[2], host[2])
    print("accumulated: rms(host - host again) %.3g, rms(device-fed - host-fed) %.3g" % (spread, diff))
    assert spread < 1e-7                                                 # last-bit noise (an optimiser step moves a weight by 1e-3)
    assert diff <= 4 * spread, (diff, spread)


def test_train_loop_on_a_default_device_dataset_returns_the_window_dataset_history(tmp_path):
    from composer_amd import dataset as D
    ids, _ = bc.stream("default")
    dev, host = model(), model()
    ha = dev.train(dataset(), (B, W), tmp_path / "a", epochs=2, learning_rate=1e-3, show_progress_bar=False, max_steps=4)
    hb = host.train(D.WindowDataset(ids, B, W, shuffle=True, seed=3), (B, W), tmp_path / "b", epochs=2, learning_rate=1e-3,
                    show_progress_bar=False, max_steps=4)
    assert len(ha) == 4 and ha == hb
    assert same_weights(dev, host)
    dev.close(); host.close()


def test_every_refusal_leaves_the_model_usable():
    from composer_amd import _lib, dataset as D
    from composer_amd.grammar import EventGrammar
    ids, g = bc.stream("default")
    n = len(ids)
    dev, twin = model(), model()
    dd = dataset()
    ok = dd.plan(0, 0)

    def with_row(**kw):
        p = ok.copy()
        for k, v in kw.items():
            p[k][1] = v
        return p
    bare = D.DeviceDataset(ids, B, W, None, shuffle=True, seed=3)
    too_big = ids.copy(); too_big[100] = V                               # an id the model's vocabulary does not hold
    wide = EventGrammar(V + 200, 0, 300, 128, 100, rules=0)              # a layout that is fine for 590 ids and leaves [0, 390)
    refused = [(dd, with_row(offset=-1), "offset"), (dd, with_row(offset=n - W), "offset"), (dd, with_row(stretch_q10=511), "stretch"),
               (dd, with_row(stretch_q10=1537), "stretch"), (dd, with_row(transpose=128), "transpose"),
               (bare, with_row(transpose=1), "layout"), (bare, with_row(stretch_q10=1000), "layout"),
               (D.DeviceDataset(too_big, B, W, g), ok, "largest id"), (D.DeviceDataset(ids, B, W, wide), ok, "outside the vocabulary")]
    for d, plan, word in refused:
        with pytest.raises(_lib.HipLibraryError, match=word):
            dev.train_step_dataset(d, plan, 1e-3)
    with pytest.raises(_lib.HipLibraryError, match="offset"):
        dev.dataset_batch(dd, with_row(offset=n))
    assert dev.iterations == 0
    # nothing was enqueued, no ticket was spent, no state moved: the next step is the twin's first step
    la = dev.step_metrics(dev.train_step_dataset(bare, ok, 1e-3))          # (an identity plan needs no layout)
    lb = twin.step_metrics(twin.train_step_async(*dd.host_batch(ok), 1e-3))
    assert la == lb and same_weights(dev, twin)
    dev.close(); twin.close()


def test_cli_train_with_augmentation_writes_a_checkpoint(tmp_path):
    from composer_amd import checkpoint as ckpt, cli, dataset as D
    root = tmp_path / "data"
    (root / "train").mkdir(parents=True)
    D.write_synthetic_data_file(root / "train" / "a.data", 10 * 2 * 33 + 50, seed=21)
    cfg = yaml.safe_load(open(cli.get_default_config()))
    cfg["transformer"]["model"].update(window_size=32, decoder_layers_count=2, embedding_size=64, attention_head_count=4)
    cfg["transformer"]["train"]["batch_size"] = 2
    cfg["transformer"]["runtime"] = {"dtype": "fp32", "seed": 5}
    cfg_path = tmp_path / "cfg.yml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    res = CliRunner().invoke(cli.cli, ["train", "transformer", str(root), "--logdir", str(tmp_path / "logs"), "-c", str(cfg_path), "-e", "2",
                                       "--no-show-progress-bar", "--augment-transpose", "3", "--augment-stretch", "0.05", "--random-crop",
                                       "--max-steps", "3", "--save-freq", "3"], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    (run,) = list((tmp_path / "logs").iterdir())
    assert sorted(p.name for p in run.glob("ckpt-*")) == ["ckpt-1.npz"]
    sd, meta = ckpt.load(str(run / "ckpt-1"))
    assert int(meta["step"]) == 3 and int(sd["optimizer/iter"]) == 3
    assert all(np.isfinite(v).all() for v in sd.values())
