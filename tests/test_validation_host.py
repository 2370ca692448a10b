"""No GPU: the host side of validation during training -- ValidationTracker, the rank-0 verdict exchange, EvalReport's arithmetic, the
option and config plumbing of `composer train`, and the command lines that are refused before any device use."""
import math

import click
import numpy as np
import pytest
from click.testing import CliRunner

from composer_amd import cli, config, dataset as D
from composer_amd.transformer import EvalReport, ValidationTracker, check_eval_options, exchange_verdict


# ------------------------------------------------------------------------------------------------ ValidationTracker
def test_tracker_improvement_and_patience():
    t = ValidationTracker(patience=2)
    assert t.update(10, 3.0) == (True, False)                  # the first finite loss is the best
    assert t.update(20, 2.5) == (True, False)
    assert t.update(30, 2.5) == (False, False)                 # equal is not an improvement
    assert t.update(40, 2.4) == (True, False)                  # ... and an improvement resets the count
    assert t.update(50, 2.6) == (False, False)
    assert t.update(60, 2.4) == (False, True)                  # two passes in a row without one
    assert (t.best, t.best_step, t.bad_passes) == (2.4, 40, 2)


def test_tracker_min_delta_is_strict():
    t = ValidationTracker(patience=0, min_delta=0.1)
    assert t.update(1, 1.0)[0]
    assert not t.update(2, 0.95)[0] and not t.update(3, 0.9)[0]           # 0.9 < 1.0 - 0.1 is false
    assert t.update(4, 0.8999)[0] and t.best == 0.8999
    with pytest.raises(ValueError):
        ValidationTracker(patience=-1)
    with pytest.raises(ValueError):
        ValidationTracker(min_delta=-0.1)
    with pytest.raises(ValueError):
        ValidationTracker(min_delta=math.nan)


def test_tracker_nan_never_improves_and_patience_zero_never_stops():
    t = ValidationTracker(patience=0)
    assert t.update(1, math.nan) == (False, False) and t.best is None
    assert t.update(2, 5.0) == (True, False)                   # the first FINITE loss
    for s in range(3, 40):
        assert t.update(s, math.nan if s % 2 else 6.0) == (False, False)
    assert t.best == 5.0 and t.bad_passes == 37
    t = ValidationTracker(patience=1)
    assert t.update(1, math.nan) == (False, True)


def test_tracker_state_round_trip():
    t = ValidationTracker(patience=3)
    for s, v in ((2, 4.0), (4, 3.0), (6, 3.5)):
        t.update(s, v)
    import json
    state = json.loads(json.dumps(t.state()))                  # as a checkpoint's meta carries it
    u = ValidationTracker.from_state(state, patience=3)
    assert u.state() == t.state() == {"best": 3.0, "best_step": 4, "bad_passes": 1}
    assert u.update(8, 3.2) == (False, False) and u.update(10, 3.1) == (False, True)
    fresh = ValidationTracker.from_state(None, patience=3)     # a checkpoint from before the feature: the count starts
    assert fresh.state() == {"best": None, "best_step": None, "bad_passes": 0}
    empty = ValidationTracker.from_state(json.loads(json.dumps(ValidationTracker(2).state())), patience=2)
    assert empty.update(1, 1.0) == (True, False)


# ------------------------------------------------------------------------------------------------ the verdict exchange
def test_rank_zero_decides_for_every_rank():
    """World size 2, a fake all_reduce_sum that adds the per-rank vectors.  Rank 1's own numbers never stop (its losses keep
    improving); rank 0's do at pass 3: both ranks leave the loop at the same pass."""
    losses = {0: [3.0, 3.1, 3.2, 3.3], 1: [3.0, 2.9, 2.8, 2.7]}
    trackers = {r: ValidationTracker(patience=2) for r in (0, 1)}
    stopped = {0: None, 1: None}
    for p in range(4):
        own = {r: trackers[r].update(p + 1, losses[r][p]) for r in (0, 1)}
        assert own[1][1] is False
        sent = {}
        for r in (0, 1):                                       # every rank hands in its vector; the fake adds them
            exchange_verdict(lambda v, r=r: sent.setdefault(r, np.asarray(v, np.float32)), r, *own[r])
        total = sent[0] + sent[1]
        assert (sent[1] == 0).all()                            # only rank 0 contributes
        verdict = {r: exchange_verdict(lambda v: total, r, *own[r]) for r in (0, 1)}
        assert verdict[0] == verdict[1] == own[0]
        for r in (0, 1):
            if verdict[r][1] and stopped[r] is None:
                stopped[r] = p + 1
        if verdict[0][1]:
            break
    assert stopped == {0: 3, 1: 3}


# ------------------------------------------------------------------------------------------------ EvalReport
def test_eval_report_arithmetic():
    names = ["a", "b", "c"]
    r = EvalReport(names, [6.0, 0.0, 1.5, 0.5, 9, 9, 9, 9, 9], [4, 0, 1, 1, 0, 0, 0, 0, 0], [2, 0, 1, 0, 0, 0, 0, 0, 0], windows=3)
    assert r.events == 6 and r.loss == 8.0 / 6 and r.accuracy == 0.5 and r.windows == 3
    assert r.bits_per_event == r.loss / math.log(2) and r.perplexity == math.exp(r.loss)
    by = r.by_event_type
    assert list(by) == names and by["a"] == (4, 1.5, 0.5) and by["c"] == (1, 1.5, 1.0)
    assert by["b"][0] == 0 and math.isnan(by["b"][1]) and math.isnan(by["b"][2])          # an empty class: NaN, not a division error
    assert r.other == (1, 0.5, 0.0)
    d = r.to_dict()
    assert d["events"] == 6 and d["by_event_type"]["a"] == {"count": 4, "nll_per_event": 1.5, "accuracy": 0.5} and d["other"]["count"] == 1
    empty = EvalReport([], [0.0], [0], [0])
    assert empty.events == 0 and all(math.isnan(v) for v in (empty.loss, empty.accuracy, empty.bits_per_event, empty.perplexity))
    assert "other" not in empty.to_dict()
    with pytest.raises(ValueError):
        EvalReport(names, [1.0], [1], [1])


# ------------------------------------------------------------------------------------------------ options and config
def test_check_eval_options():
    assert check_eval_options() == (0, None, 0, False)
    assert check_eval_options(5, 10, 2, True) == (5, 10, 2, True)
    for bad in ((-1, None, 0, False), (1, 0, 0, False), (1, -3, 0, False), (1, None, -1, False), (0, None, 2, False), (0, None, 0, True)):
        with pytest.raises(ValueError):
            check_eval_options(*bad)


def test_yaml_keys_are_optional_and_flags_override_them(tmp_path):
    default = config.get(cli.get_default_config())
    assert cli.eval_options_from(default) == (0, "test", None, 0, False)
    bare = tmp_path / "bare.yml"                               # a reference file: none of the keys
    bare.write_text("transformer:\n    train: {batch_size: 1, learning_rate: 0.001}\n")
    assert cli.eval_options_from(config.get(bare)) == (0, "test", None, 0, False)
    keyed = tmp_path / "keyed.yml"
    keyed.write_text("transformer:\n    train: {batch_size: 1, learning_rate: 0.001, eval_freq: 50, eval_split: valid, eval_max_windows: 64, "
                     "early_stop_patience: 4, keep_best_checkpoint: true}\n")
    c = config.get(keyed)
    assert cli.eval_options_from(c) == (50, "valid", 64, 4, True)
    assert cli.eval_options_from(c, eval_freq=10, eval_split="test", eval_max_windows=8, early_stop_patience=0,
                                 keep_best_checkpoint=False) == (10, "test", 8, 0, False)
    assert cli.eval_options_from(c, early_stop_patience=1) == (50, "valid", 64, 1, True)
    with pytest.raises(click.UsageError):
        cli.eval_options_from(c, eval_freq=0)                  # the keys ask for patience and keep-best: nothing to act on
    with pytest.raises(click.UsageError):
        cli.eval_options_from(default, eval_freq=5, eval_split="../x")
    bad = tmp_path / "bad.yml"
    bad.write_text("transformer:\n    train: {batch_size: 1, learning_rate: 0.001, eval_freq: -2}\n")
    with pytest.raises(click.UsageError):
        cli.eval_options_from(config.get(bad))


def _dataset(tmp_path, test_events=None):
    root = tmp_path / "data"
    (root / "train").mkdir(parents=True)
    D.write_synthetic_data_file(root / "train" / "a.data", 600, seed=1)
    if test_events is not None:
        (root / "test").mkdir()
        if test_events:
            D.write_synthetic_data_file(root / "test" / "b.data", test_events, seed=2)
    return root


def test_cli_refuses_before_touching_a_device(tmp_path, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a model was created for a command line that must be refused")
    monkeypatch.setattr(cli, "create_model", no_device)
    log = ["--logdir", str(tmp_path / "log")]
    for args, word in ((["--eval-freq", "-1"], "--eval-freq"), (["--eval-max-windows", "0"], "--eval-max-windows"),
                       (["--early-stop-patience", "-1"], "--early-stop-patience")):
        r = CliRunner().invoke(cli.cli, ["train", "transformer", str(tmp_path)] + log + args)
        assert r.exit_code == 2 and "Usage" in r.output and word in r.output, r.output
        assert not (tmp_path / "log").exists()
    root = _dataset(tmp_path)                                  # no test folder
    for args, word in ((["--early-stop-patience", "2"], "eval_freq"), (["--keep-best-checkpoint"], "eval_freq"),
                       (["--eval-freq", "2"], "missing"), (["--eval-freq", "2", "--eval-split", "valid"], "valid")):
        r = CliRunner().invoke(cli.cli, ["train", "transformer", str(root)] + log + args)
        assert r.exit_code == 2 and "Usage" in r.output and word in r.output, r.output
    rec = tmp_path / "set.tfrecord"                            # a .tfrecord has no folders
    rec.write_bytes(b"")
    r = CliRunner().invoke(cli.cli, ["train", "transformer", str(rec)] + log + ["--eval-freq", "2"])
    assert r.exit_code == 2 and "directory dataset" in r.output, r.output
    (tmp_path / "e").mkdir()
    empty = _dataset(tmp_path / "e", test_events=0)            # an empty test folder
    r = CliRunner().invoke(cli.cli, ["train", "transformer", str(empty)] + log + ["--eval-freq", "2"])
    assert r.exit_code == 2 and "holds no .data file" in r.output, r.output
    (tmp_path / "s").mkdir()
    short = _dataset(tmp_path / "s", test_events=100)          # the default window_size is larger than that
    r = CliRunner().invoke(cli.cli, ["train", "transformer", str(short)] + log + ["--eval-freq", "2"])
    assert r.exit_code == 2 and "window_size + 1" in r.output, r.output


def test_eval_stream_is_the_split_in_file_order(tmp_path):
    root = _dataset(tmp_path, test_events=300)
    D.write_synthetic_data_file(root / "test" / "a.data", 40, seed=3)
    c = config.get(cli.get_default_config())
    c.transformer.model.window_size = 16
    ids = cli.get_eval_stream(root, c, "test")
    files = D.get_processed_files(root / "test")
    assert ids.dtype == np.uint16 and len(ids) == 340 and (ids == D.read_id_stream(files)).all()
    ranges = cli.event_class_ranges(c)
    assert list(ranges) == ["NOTE_ON", "NOTE_OFF", "VELOCITY", "TIME_SHIFT", "SUSTAIN_ON", "SUSTAIN_OFF"]
    assert ranges["SUSTAIN_OFF"].stop == 390
