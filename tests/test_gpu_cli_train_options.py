"""-m gpu: `composer train ... --accumulate-steps 2 --clip-norm 0.5 --warmup-steps 3` on a synthetic `.data` file: steps, --max-steps
and the checkpoint's `step` count OPTIMISER steps, and the event file holds the new scalars beside `loss`."""
import glob

import numpy as np
import pytest
import yaml
from click.testing import CliRunner

pytestmark = pytest.mark.gpu


def test_train_with_accumulation_clipping_and_warmup(tmp_path):
    from composer_amd import checkpoint as ckpt, cli, dataset as D, tbevents
    from composer_amd.transformer import warmup_lr
    root = tmp_path / "data"
    (root / "train").mkdir(parents=True)
    D.write_synthetic_data_file(root / "train" / "a.data", 10 * 2 * 129 + 50, seed=21)     # 10 batches of 2 windows of 129
    cfg = yaml.safe_load(open(cli.get_default_config()))
    cfg["transformer"]["model"].update(window_size=128, decoder_layers_count=2)
    cfg["transformer"]["train"]["batch_size"] = 2
    cfg["transformer"]["train"]["clip_norm"] = 100.0              # the flag overrides the key
    cfg["transformer"]["runtime"] = {"dtype": "fp32", "seed": 5}
    cfg_path = tmp_path / "cfg.yml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    lr = cfg["transformer"]["train"]["learning_rate"]
    res = CliRunner().invoke(cli.cli, ["train", "transformer", str(root), "--logdir", str(tmp_path / "logs"), "-c", str(cfg_path), "-e", "2",
                                       "--no-show-progress-bar", "--max-steps", "4", "--save-freq", "4", "--accumulate-steps", "2",
                                       "--clip-norm", "0.5", "--warmup-steps", "3"], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    (run,) = list((tmp_path / "logs").iterdir())
    (path,) = glob.glob(str(run / "train" / "events.out.tfevents.*"))
    _, ev = tbevents.read_scalars(path)
    by = {}
    for tag, step, value, _ in ev:
        by.setdefault(tag, []).append((step, value))
    for tag in ("loss", "accuracy", "grad_norm", "learning_rate"):
        assert [s for s, _ in by[tag]] == [1, 2, 3, 4], (tag, by[tag])             # 4 optimiser steps from 8 batches
    assert all(np.isfinite(v) and v > 0.5 for _, v in by["grad_norm"])              # an untrained model: the clip at 0.5 binds
    assert np.allclose([v for _, v in by["learning_rate"]], [lr / 3, 2 * lr / 3, lr, lr], rtol=1e-6)
    assert [warmup_lr(lr, s, 3) for s in (1, 2, 3, 4)] == pytest.approx([v for _, v in by["learning_rate"]], rel=1e-6)
    assert sorted(p.name for p in run.glob("ckpt-*")) == ["ckpt-1.npz"]
    sd, meta = ckpt.load(str(run / "ckpt-1"))
    assert int(meta["step"]) == 4 and int(sd["optimizer/iter"]) == 4                # the optimiser step, not the batch count
