"""-m gpu: validation during training through the command line -- `train --eval-freq / --keep-best-checkpoint / --early-stop-patience`,
the resume of the tracker's count, and `evaluate --by-event-type`.  Synthetic train/ and test/ folders, window 16, fp32, 2 blocks.
The test split holds 5 windows and 3 more events: with batch 2 its last batch is ragged."""
import json
import logging

import numpy as np
import pytest
import yaml
from click.testing import CliRunner

pytestmark = pytest.mark.gpu
W = 16
TEST_WINDOWS = 5


def make_data(tmp_path, learning_rate=None):
    from composer_amd import cli, dataset as D
    root = tmp_path / "data"
    (root / "train").mkdir(parents=True); (root / "test").mkdir()
    D.write_synthetic_data_file(root / "train" / "a.data", 10 * 2 * (W + 1) + 5, seed=21)
    D.write_synthetic_data_file(root / "test" / "b.data", TEST_WINDOWS * (W + 1) + 3, seed=22)
    cfg = yaml.safe_load(open(cli.get_default_config()))
    cfg["transformer"]["model"].update(window_size=W, decoder_layers_count=2, embedding_size=64, attention_head_count=4)
    cfg["transformer"]["train"]["batch_size"] = 2
    if learning_rate is not None:
        cfg["transformer"]["train"]["learning_rate"] = learning_rate
    cfg["transformer"]["runtime"] = {"dtype": "fp32", "seed": 5}
    cfg_path = tmp_path / "cfg.yml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    return root, cfg_path


def train(root, cfg_path, logs, *args):
    from composer_amd import cli
    base = ["train", "transformer", str(root), "--logdir", str(logs), "-c", str(cfg_path), "-e", "100", "--no-show-progress-bar"]
    res = CliRunner().invoke(cli.cli, base + list(args), catch_exceptions=False)
    assert res.exit_code == 0, res.output
    return res


def scalars(run, tag):
    rows = [json.loads(l) for l in open(run / "train" / "scalars.jsonl")]
    return [(r["step"], r["value"]) for r in rows if r["tag"] == tag]


@pytest.fixture(scope="module")
def run_a(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("evalpass_a")
    root, cfg_path = make_data(tmp)
    train(root, cfg_path, tmp / "logs", "--eval-freq", "2", "--max-steps", "6", "--keep-best-checkpoint", "--save-freq", "3")
    (run,) = list((tmp / "logs").iterdir())
    return tmp, root, run


def test_run_a_logs_validation_and_keeps_the_best_state(run_a):
    from composer_amd import checkpoint as ckpt, cli, config as cfgmod, dataset as D
    tmp, root, run = run_a
    val = scalars(run, "val_loss")
    assert [s for s, _ in val] == [2, 4, 6] and all(np.isfinite(v) for _, v in val)
    assert [s for s, _ in scalars(run, "val_accuracy")] == [2, 4, 6]
    assert [s for s, _ in scalars(run, "val_nll/NOTE_ON")] == [2, 4, 6]
    assert [s for s, _ in scalars(run, "loss")] == [1, 2, 3, 4, 5, 6]
    # the rolling checkpoints are what --save-freq 3 alone writes; best/ holds one checkpoint, of the lowest val_loss
    assert sorted(p.name for p in run.glob("ckpt-*")) == ["ckpt-1.npz", "ckpt-2.npz"]
    assert len(list((run / "best").glob("ckpt-*"))) == 1
    mgr = ckpt.CheckpointManager(run / "best", max_to_keep=1)
    _, meta = ckpt.load(mgr.latest_checkpoint)
    step, loss = min(val, key=lambda sv: (sv[1], sv[0]))
    assert meta["val_loss"] == loss and meta["step"] == step and meta["epoch"] == 1
    _, rolling = ckpt.load(str(run / "ckpt-2"))
    assert rolling["step"] == 6 and rolling["validation"]["best"] == loss and rolling["validation"]["best_step"] == step
    # the restored parameters give that loss again, bit for bit
    config = cfgmod.get(run / "best" / "config.yml")
    model, _ = cli.create_model(cli.ModelType.TRANSFORMER, config)
    model.load_from_checkpoint(run / "best")
    ids = D.read_id_stream(D.get_processed_files(root / "test"))
    rep = model.evaluate_dataset(D.DeviceDataset(ids, 2, W, shuffle=False), event_ranges=cli.event_class_ranges(config))
    model.close()
    assert rep.windows == TEST_WINDOWS and rep.events == TEST_WINDOWS * W
    assert rep.loss == loss


def test_best_is_restorable_with_generate(run_a):
    from composer_amd import cli, dataset as D
    tmp, root, run = run_a
    out = tmp / "gen.data"
    res = CliRunner().invoke(cli.cli, ["generate", "transformer", str(run / "best"), str(out), "--prompt-ids", "60,300,188", "--length", "8"])
    assert res.exit_code == 0, res.output
    assert len(D.read_data_file(out)[0]) >= 8


def test_evaluate_by_event_type(run_a):
    from composer_amd import cli
    tmp, root, run = run_a
    out = tmp / "eval.json"
    res = CliRunner().invoke(cli.cli, ["evaluate", "transformer", str(root), str(run), "--by-event-type", "--json", str(out)])
    assert res.exit_code == 0, res.output
    lines = [l for l in res.output.splitlines() if l.startswith("  ") and " count " in l]
    assert [l.split(":")[0].strip() for l in lines] == ["NOTE_ON", "NOTE_OFF", "VELOCITY", "TIME_SHIFT", "SUSTAIN_ON", "SUSTAIN_OFF"]
    rep = json.load(open(out))
    assert rep["events"] == TEST_WINDOWS * W == sum(int(l.split(" count ")[1].split()[0]) for l in lines)
    assert sum(v["count"] for v in rep["by_event_type"].values()) == rep["events"]
    assert any(l.startswith("loss ") and " accuracy " in l for l in res.output.splitlines())
    # without the flag: the call it was (two windows per batch, the remainder dropped)
    res = CliRunner().invoke(cli.cli, ["evaluate", "transformer", str(root), str(run)])
    assert res.exit_code == 0 and res.output.strip().splitlines()[-1].startswith("loss "), res.output


def test_run_b_stops_early_and_run_c_resumes_the_count(tmp_path, caplog):
    root, cfg_path = make_data(tmp_path, learning_rate=0.0)
    caplog.set_level(logging.INFO)
    common = ("--eval-freq", "1", "--early-stop-patience", "2", "--save-freq", "1")
    # run B: the parameters never move, every pass returns the same bits: pass 1 is the best, passes 2 and 3 do not improve
    train(root, cfg_path, tmp_path / "b", *common, "--max-steps", "50")
    (run,) = list((tmp_path / "b").iterdir())
    val = scalars(run, "val_loss")
    assert [s for s, _ in val] == [1, 2, 3] and len({v for _, v in val}) == 1
    assert [s for s, _ in scalars(run, "loss")] == [1, 2, 3]
    assert "Early stop at step 3: val_loss" in caplog.text and "at step 1" in caplog.text
    # run C: stopped by --max-steps after two passes, resumed: the count continues from the checkpoint's meta
    caplog.clear()
    train(root, cfg_path, tmp_path / "c", *common, "--max-steps", "2")
    (run,) = list((tmp_path / "c").iterdir())
    assert [s for s, _ in scalars(run, "val_loss")] == [1, 2] and "Early stop" not in caplog.text
    from composer_amd import cli
    res = CliRunner().invoke(cli.cli, ["train", "transformer", str(root), "--restoredir", str(run), "-e", "100", "--no-show-progress-bar",
                                       *common, "--max-steps", "50"], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    val = scalars(run, "val_loss")
    assert len(val) == 3 and len({v for _, v in val}) == 1                # one more step, one more pass
    assert "Early stop at step" in caplog.text and "at step 1" in caplog.text


def test_the_last_step_is_evaluated_when_the_run_ends_between_passes(tmp_path):
    root, cfg_path = make_data(tmp_path)
    train(root, cfg_path, tmp_path / "logs", "--eval-freq", "4", "--max-steps", "6", "--eval-max-windows", "3")
    (run,) = list((tmp_path / "logs").iterdir())
    assert [s for s, _ in scalars(run, "val_loss")] == [4, 6]
    assert not (run / "best").exists()                        # --keep-best-checkpoint was not asked for
