"""Train options on the host: the clip-scale and warm-up restatements, the CLI's range checks (before any device use) and the
optional YAML keys `transformer.train.{clip_norm, accumulate_steps, warmup_steps}`."""
import math

import pytest
from click.testing import CliRunner

from composer_amd import cli, config
from composer_amd.transformer import check_train_options, clip_scale, warmup_lr


def test_clip_scale_is_tf_clip_by_global_norm():
    assert clip_scale(0.5, 1.0) == 1.0                    # below the clip
    assert clip_scale(1.0, 1.0) == 1.0                    # at the clip: norm <= clip_norm
    assert clip_scale(4.0, 1.0) == 0.25                   # above it: clip_norm / norm
    assert clip_scale(1e30, math.inf) == 1.0              # an infinite clip measures only
    assert clip_scale(123.0, 0.0) == 1.0                  # 0 = off
    assert math.isnan(clip_scale(math.nan, 1.0)) and math.isnan(clip_scale(math.nan, math.inf))


def test_warmup_lr():
    lr = 1e-3
    assert warmup_lr(lr, 1, 4) == lr * 0.25
    assert warmup_lr(lr, 4, 4) == lr
    assert warmup_lr(lr, 5, 4) == lr
    assert warmup_lr(lr, 1, 0) == lr and warmup_lr(lr, 1000, 0) == lr       # off
    assert [warmup_lr(3.0, s, 3) for s in (1, 2, 3, 4)] == [1.0, 2.0, 3.0, 3.0]


def test_option_ranges():
    assert check_train_options(0, 1, 0) == (0.0, 1, 0)
    assert check_train_options(math.inf, 4, 10) == (math.inf, 4, 10)
    for bad in ((-1, 1, 0), (math.nan, 1, 0), (0, 0, 0), (0, 1.5, 0), (0, 1, -1)):
        with pytest.raises(ValueError):
            check_train_options(*bad)


@pytest.mark.parametrize("args, word", [(["--clip-norm", "-1"], "--clip-norm"), (["--clip-norm", "nan"], "--clip-norm"),
                                        (["--accumulate-steps", "0"], "--accumulate-steps"), (["--warmup-steps", "-1"], "--warmup-steps")])
def test_cli_refuses_bad_values_before_touching_a_device(args, word, tmp_path, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a model was created for a command line that must be refused")
    monkeypatch.setattr(cli, "create_model", no_device)
    r = CliRunner().invoke(cli.cli, ["train", "transformer", str(tmp_path), "--logdir", str(tmp_path / "log")] + args)
    assert r.exit_code == 2 and "Usage" in r.output and word in r.output
    assert not (tmp_path / "log").exists()


def test_yaml_keys_are_optional_and_flags_override_them(tmp_path):
    default = config.get(cli.get_default_config())
    assert cli.train_options_from(default) == (0.0, 1, 0)
    bare = tmp_path / "bare.yml"                          # the reference's file: no such keys
    bare.write_text("transformer:\n    train: {batch_size: 1, learning_rate: 0.001}\n")
    assert cli.train_options_from(config.get(bare)) == (0.0, 1, 0)
    f = tmp_path / "c.yml"
    f.write_text("transformer:\n    train: {batch_size: 1, learning_rate: 0.001, clip_norm: 0.5, accumulate_steps: 4, warmup_steps: 100}\n")
    c = config.get(f)
    assert cli.train_options_from(c) == (0.5, 4, 100)
    assert cli.train_options_from(c, clip_norm=2.0) == (2.0, 4, 100)
    assert cli.train_options_from(c, accumulate_steps=1, warmup_steps=0) == (0.5, 1, 0)
    inf = tmp_path / "inf.yml"
    inf.write_text("transformer:\n    train: {batch_size: 1, learning_rate: 0.001, clip_norm: .inf}\n")
    assert cli.train_options_from(config.get(inf)) == (math.inf, 1, 0)
    bad = tmp_path / "bad.yml"
    bad.write_text("transformer:\n    train: {batch_size: 1, learning_rate: 0.001, accumulate_steps: 0}\n")
    import click
    with pytest.raises(click.UsageError):
        cli.train_options_from(config.get(bad))
