"""CPU checks of the augmentation contract (composer_amd/augment.py, include/composer_hip.h "device dataset") and of
DeviceDataset's plans.  Integers only: every comparison is equality."""
import numpy as np
import pytest
from click.testing import CliRunner

import batch_cases as bc
from composer_amd import augment, cli, config
from composer_amd import dataset as ds
from composer_amd.grammar import EventGrammar

G = EventGrammar.from_dataset_params(10, 100, 32, rules=0)        # 0 / 128 / 288, M = 100
TS0, M = G.time_shift0, G.time_shift_n
VEL0 = 256


def shift(steps):
    return TS0 + steps - 1


def steps_of(ids, g=G):
    ids = np.asarray(ids)
    sel = (ids >= g.time_shift0) & (ids < g.time_shift0 + g.time_shift_n)
    return int((ids[sel] - g.time_shift0 + 1).sum())


def test_R_is_monotone_and_the_identity_at_1024():
    for f in (512, 513, 1000, 1023, 1024, 1025, 1100, 1536):
        r = [augment.R(t, f) for t in range(0, 5000)]
        assert all(b >= a for a, b in zip(r, r[1:])), f
        assert r[0] == 0
    assert all(augment.R(t, 1024) == t for t in range(0, 5000))
    assert augment.R(2 ** 40, 1536) == (2 ** 40 * 1536 + 512) >> 10          # beyond 32 bits


@pytest.mark.parametrize("name", ["default", "small"])
@pytest.mark.parametrize("f", [512, 700, 1000, 1024, 1100, 1536])
def test_emitted_steps_of_a_span_sum_to_R_of_its_total(name, f):
    ids, g = bc.stream(name)
    for a, b in ((0, 300), (290, 700), (305, 563), (1303, 1400), (3500, 6200), (0, 6200)):
        src = ids[a:b]
        em = augment.stretch_tokens(src, g, f)
        assert steps_of(em, g) == augment.R(steps_of(src, g), f), (a, b)
        # the other events come through untouched and in order
        other = lambda v: v[(v < g.time_shift0) | (v >= g.time_shift0 + g.time_shift_n)]
        assert np.array_equal(other(em), other(src.astype(np.int64)))
        # canonical chunking: inside a run only the last id may be shorter than M steps
        sh = (em >= g.time_shift0) & (em < g.time_shift0 + g.time_shift_n)
        for i in range(len(em) - 1):
            if sh[i] and sh[i + 1]:
                assert em[i] == g.time_shift0 + g.time_shift_n - 1


def test_f_1024_is_a_plain_copy_even_on_non_canonical_runs():
    src = np.array([5, shift(30), shift(50), 130, shift(100), shift(100), shift(1), 7] * 3, np.uint16)
    assert list(augment.stretch_tokens([shift(30), shift(50)], G, 1024)) == [shift(80)]     # the walk itself re-chunks ...
    W = 9
    x, y, st = augment.build_row(src, G, 2, 0, 1024, W)                                     # ... so build_row does not walk
    assert np.array_equal(x, src[2:2 + W]) and np.array_equal(y, src[3:3 + W]) and st == (W + 1, 0)
    x, y, st = augment.build_row(src, None, 2, 0, 1024, W)                                  # and needs no layout
    assert np.array_equal(x, src[2:2 + W]) and st == (W + 1, 0)


def test_runs_that_round_to_nothing_vanish():
    # R(1) - R(0) = 1 but R(2) - R(1) = 0 at f = 512: the second one-step run disappears, the events around it stay
    src = [5, shift(1), 6, shift(1), 7, shift(2), 8]
    assert list(augment.stretch_tokens(src, G, 512)) == [5, shift(1), 6, 7, shift(1), 8]


def test_a_multiple_of_M_emits_no_remainder_token():
    assert list(augment.stretch_tokens([shift(100), shift(100)], G, 1024)) == [shift(100), shift(100)]
    assert list(augment.stretch_tokens([shift(100), shift(100)], G, 1536)) == [shift(100)] * 3
    assert list(augment.stretch_tokens([shift(100), shift(50)], G, 1024)) == [shift(100), shift(50)]
    assert list(augment.stretch_tokens([shift(40), shift(40)], G, 512)) == [shift(40)]


def test_transpose_clamps_at_0_and_127_for_note_on_and_note_off_and_leaves_the_rest():
    every = np.arange(G.vocab_size)
    for k in (-12, -1, 0, 1, 12):
        out = augment.transpose_tokens(every, G, k)
        for base in (G.note_on0, G.note_off0):
            assert np.array_equal(out[base:base + 128], base + np.clip(np.arange(128) + k, 0, 127))
        rest = np.r_[VEL0:G.vocab_size]
        assert np.array_equal(out[rest], every[rest])                   # velocities, time shifts, pedal
    assert augment.transpose_tokens([G.note_on0, G.note_off0], G, -12).tolist() == [G.note_on0, G.note_off0]
    assert augment.transpose_tokens([G.note_on0 + 127, G.note_off0 + 127], G, 12).tolist() == [G.note_on0 + 127, G.note_off0 + 127]
    g2 = EventGrammar.from_dataset_params(10, 50, 4, rules=0)           # the layout is the caller's: another one moves other ids
    assert augment.transpose_tokens([259, 260], g2, 5).tolist() == [259, 260]


def test_long_runs_of_one_step_shifts_fall_back_at_f_512():
    W = 16
    src = np.array([shift(1)] * 40 + [5] * 10, np.uint16)               # 34 tokens of the span emit one id of 17 steps
    x, y, st = augment.build_row(src, G, 0, 12, 512, W)
    assert st == (1, augment.FALLBACK)                                  # the bit itself: this case must keep falling back
    assert np.array_equal(x, src[:W]) and np.array_equal(y, src[1:W + 1])
    src[3] = G.note_on0 + 120                                           # the fallback row is still transposed
    x, _, st = augment.build_row(src, G, 0, 12, 512, W)
    assert st[1] == augment.FALLBACK and x[3] == G.note_on0 + 127


def test_build_batch_is_build_row_per_row_and_the_cases_cover_what_they_were_built_for():
    for name in ("default", "small"):
        ids, g = bc.stream(name)
        for W, B, plan in bc.cases(name):
            x, y, st = augment.build_batch(ids, g, plan, W)
            assert x.shape == (B, W) and y.shape == (B, W) and st.shape == (B, 2) and x.dtype == np.int32
            assert np.array_equal(x[:, 1:], y[:, :-1])
            for b in range(B):
                xr, yr, sr = augment.build_row(ids, g, plan["offset"][b], plan["transpose"][b], plan["stretch_q10"][b], W)
                assert np.array_equal(x[b], xr) and np.array_equal(y[b], yr) and tuple(st[b]) == sr
            assert x.min() >= 0 and max(x.max(), y.max()) < g.vocab_size
    missing = set(bc.ALL_FEATURES) - bc.covered()
    assert not missing, missing


def test_plan_and_option_refusals():
    ids, g = bc.stream("default")
    n = len(ids)
    for bad in ((-1, 0, 1024), (n - 8 + 1, 0, 1024), (0, 0, 511), (0, 0, 1537), (0, 128, 1024)):
        with pytest.raises(ValueError):
            augment.build_row(ids, g, *bad, 7)
    with pytest.raises(ValueError):
        augment.build_row(ids, None, 0, 1, 1024, 7)                     # not the identity: needs a layout
    with pytest.raises(ValueError):
        augment.build_row(ids, None, 0, 0, 1000, 7)
    augment.build_row(ids, g, n - 8, 0, 1024, 7)                        # the last legal offset
    assert augment.check_augment_options() == (0, 0.0, False)
    assert augment.check_augment_options(12, 0.5, True) == (12, 0.5, True)
    for kw in ({"transpose": -1}, {"transpose": 13}, {"stretch": -0.1}, {"stretch": 0.51}, {"stretch": float("nan")}):
        with pytest.raises(ValueError):
            augment.check_augment_options(**kw)
    for kw in ({"transpose": 1.5}, {"transpose": True}, {"stretch": "0.1"}, {"random_crop": 1}):
        with pytest.raises(TypeError):
            augment.check_augment_options(**kw)
    assert augment.stretch_bounds(0.5) == (512, 1536) and augment.stretch_bounds(0.0) == (1024, 1024)
    with pytest.raises(ValueError):
        ds.DeviceDataset(ids, 4, 32, None, transpose=3)


def test_default_device_dataset_walks_window_dataset_order():
    ids, g = bc.stream("default")
    for shuffle, world in ((True, 1), (False, 1), (True, 2)):
        for rank in range(world):
            wd = ds.WindowDataset(ids, 4, 32, shuffle=shuffle, seed=3, rank=rank, world_size=world)
            dd = ds.DeviceDataset(ids, 4, 32, g, shuffle=shuffle, seed=3, rank=rank, world_size=world)
            assert len(dd) == len(wd) > 3
            for epoch in range(2):                                      # one pass = one epoch, reshuffled
                n = 0
                for (x, y), batch in zip(wd, dd):
                    assert isinstance(batch, ds.DeviceBatch) and batch.dataset is dd
                    assert (batch.plan["transpose"] == 0).all() and (batch.plan["stretch_q10"] == 1024).all()
                    assert (batch.plan["offset"] % 33 == 0).all()
                    hx, hy = dd.host_batch(batch.plan)
                    assert np.array_equal(hx, x) and np.array_equal(hy, y)
                    n += 1
                assert n == len(wd)


def test_plans_are_a_pure_function_of_seed_epoch_and_batch():
    ids, g = bc.stream("default")
    kw = dict(shuffle=True, seed=5, random_crop=True, transpose=4, stretch=0.25)
    a, b = ds.DeviceDataset(ids, 4, 32, g, **kw), ds.DeviceDataset(ids, 4, 32, g, **kw)
    first = [bt.plan.copy() for bt in a]
    second = [bt.plan.copy() for bt in a]                               # the next epoch draws anew
    assert not all(np.array_equal(p, q) for p, q in zip(first, second))
    for i, p in enumerate(first):
        assert np.array_equal(p, b.plan(0, i)) and np.array_equal(second[i], b.plan(1, i))      # no hidden state: (epoch, batch) only
    assert not np.array_equal(ds.DeviceDataset(ids, 4, 32, g, **dict(kw, seed=6)).plan(0, 0), first[0])
    every = np.concatenate(first + second)
    assert every["offset"].min() >= 0 and every["offset"].max() <= len(ids) - 33 and (every["offset"] % 33 != 0).any()
    assert set(every["transpose"]) <= set(range(-4, 5)) and len(set(every["transpose"])) > 4
    assert every["stretch_q10"].min() >= 768 and every["stretch_q10"].max() <= 1280 and len(set(every["stretch_q10"])) > 8
    # turning augmentation on does not move the windows: the grid order is the plain dataset's
    plain = ds.DeviceDataset(ids, 4, 32, g, shuffle=True, seed=5)
    aug = ds.DeviceDataset(ids, 4, 32, g, shuffle=True, seed=5, transpose=4, stretch=0.25)
    for i in range(len(plain)):
        assert np.array_equal(plain.plan(0, i)["offset"], aug.plan(0, i)["offset"])
    # two ranks split one global batch
    r0 = ds.DeviceDataset(ids, 2, 32, g, rank=0, world_size=2, **kw).plan(0, 1)
    r1 = ds.DeviceDataset(ids, 2, 32, g, rank=1, world_size=2, **kw).plan(0, 1)
    assert np.array_equal(np.concatenate([r0, r1]), first[1])


def test_cli_options_yaml_keys_and_refusals(tmp_path, monkeypatch):
    import click
    default = config.get(cli.get_default_config())
    assert cli.augment_options_from(default) == (0, 0.0, False)
    assert cli.train_options_from(default) == (0.0, 1, 0)               # the pinned 3-tuple is untouched
    f = tmp_path / "c.yml"
    f.write_text("transformer:\n    train: {batch_size: 1, learning_rate: 0.001, augment_transpose: 3, augment_stretch: 0.05, random_crop: true}\n")
    c = config.get(f)
    assert cli.augment_options_from(c) == (3, 0.05, True)
    assert cli.augment_options_from(c, augment_transpose=0, random_crop=False) == (0, 0.05, False)
    bad = tmp_path / "bad.yml"
    bad.write_text("transformer:\n    train: {batch_size: 1, learning_rate: 0.001, augment_stretch: 0.75}\n")
    with pytest.raises(click.UsageError):
        cli.augment_options_from(config.get(bad))

    def no_device(*a, **k):
        raise AssertionError("a model was created for a command line that must be refused")
    monkeypatch.setattr(cli, "create_model", no_device)
    rec = tmp_path / "set.tfrecord"
    rec.write_bytes(b"")
    for args, word in ((["--augment-transpose", "13"], "augment_transpose"), (["--augment-stretch", "0.6"], "augment_stretch"),
                       (["--augment-transpose", "-1"], "augment_transpose")):
        r = CliRunner().invoke(cli.cli, ["train", "transformer", str(tmp_path), "--logdir", str(tmp_path / "log")] + args)
        assert r.exit_code == 2 and "Usage" in r.output and word in r.output, r.output
    for args in (["--augment-transpose", "3"], ["--augment-stretch", "0.1"], ["--random-crop"]):       # a tfrecord holds pre-cut batches
        r = CliRunner().invoke(cli.cli, ["train", "transformer", str(rec), "--logdir", str(tmp_path / "log")] + args)
        assert r.exit_code == 2 and "pre-cut" in r.output, r.output
