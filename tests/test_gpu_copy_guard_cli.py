"""-m gpu: `generate --max-copy` end to end.  A freshly initialised model is decoded once without the option; its output, written
into the train split of a synthetic directory dataset, is then the corpus of a second run with `--novelty-against D --max-copy 8`:
the `novelty:` line that reported the whole sample as one match now reports none above the bound (TIME_SHIFT events may extend
one: they are exempt), and the `copy-guard:` line counts the columns the rule took away."""
import re

import numpy as np
import pytest
import yaml
from click.testing import CliRunner

pytestmark = pytest.mark.gpu

M = 8


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    from composer_amd import checkpoint as ckpt, cli, config
    tmp = tmp_path_factory.mktemp("copyguard")
    cfg = yaml.safe_load(open(cli.get_default_config()))
    cfg["transformer"]["model"].update(embedding_size=64, window_size=64, decoder_layers_count=2, attention_head_count=4)
    cfg["transformer"]["train"]["batch_size"] = 8
    cfg["transformer"]["runtime"] = {"dtype": "fp32", "seed": 0}
    run = tmp / "run"
    run.mkdir()
    (run / "config.yml").write_text(yaml.safe_dump(cfg))
    model, _ = cli.create_model(cli.ModelType.TRANSFORMER, config.get(run / "config.yml"))          # freshly initialised
    ckpt.CheckpointManager(run, max_to_keep=1).save(model.state_dict(), {"step": 1, "epoch": 1})
    model.close()
    return tmp, run


def test_max_copy_keeps_the_sample_from_playing_the_dataset_back(run_dir):
    from composer_amd import cli, dataset as ds
    tmp, run = run_dir
    prompt = [60, 300, 188]
    common = ["--prompt-ids", ",".join(map(str, prompt)), "--length", "40"]
    train = tmp / "set" / "train"
    train.mkdir(parents=True)
    ds.write_synthetic_data_file(train / "a.data", 300, seed=1)
    # the unguarded output becomes a piece of the dataset
    res = CliRunner().invoke(cli.cli, ["generate", "transformer", str(run), str(train / "b.data")] + common)
    assert res.exit_code == 0, res.output
    free = ds.read_data_file(train / "b.data")[0].astype(np.int32)[len(prompt):]
    ts = lambda a: (a >= 288) & (a < 388)                                    # the default layout's TIME_SHIFT ids
    assert int((~ts(free[M:])).sum()) >= 8                                   # ids the rule has to ban: the test cannot pass vacuously
    args = ["--novelty-against", str(tmp / "set"), "--novelty-min-match", str(M + 1)]
    res = CliRunner().invoke(cli.cli, ["generate", "transformer", str(run), str(tmp / "again.data")] + common + args)
    assert res.exit_code == 0, res.output
    line = re.findall(r"^novelty: sample 0 (.*)$", res.output, flags=re.M)[0]
    assert line.startswith("events 40 longest 40 ") and "in train/b.data offset %d " % len(prompt) in line, line     # played back whole
    res = CliRunner().invoke(cli.cli, ["generate", "transformer", str(run), str(tmp / "guarded.data")] + common + args + ["--max-copy", str(M)])
    assert res.exit_code == 0, res.output
    got = ds.read_data_file(tmp / "guarded.data")[0].astype(np.int32)[len(prompt):]
    assert len(got) == 40 and got.tolist() != free.tolist()
    banned = re.findall(r"^copy-guard: sample 0 banned_columns (\d+)$", res.output, flags=re.M)
    assert len(banned) == 1 and int(banned[0]) > 0, res.output
    line = re.findall(r"^novelty: sample 0 (.*)$", res.output, flags=re.M)[0]
    longest = int(re.match(r"events 40 longest (\d+) ", line).group(1))
    assert longest < 40, line
    if longest > M:                                                          # only TIME_SHIFT events may carry a match past the bound
        at = int(re.search(r" at (\d+) in ", line).group(1))
        assert ts(got[at + M:at + longest]).all(), (line, got.tolist())
    # every match in prompt ++ sample, by the host restatement
    conf = cli.get_config_from_restoredir(str(run))
    corpus = cli.open_novelty_corpus(str(tmp / "set"), conf)
    try:
        seq = np.concatenate([np.asarray(prompt, np.int32), got])
        rep = corpus.match_host([seq], min_match=M + 1)[0]
        for s in np.flatnonzero(rep.len > M):
            assert ts(seq[s + M:s + int(rep.len[s])]).all(), (int(s), int(rep.len[s]))
    finally:
        corpus.close()
    # with --num-samples: one line per sample
    res = CliRunner().invoke(cli.cli, ["generate", "transformer", str(run), str(tmp / "many.data")] + common + args
                             + ["--max-copy", str(M), "--num-samples", "3", "--constrain", "--decode-mode", "kv-slide"])
    assert res.exit_code == 0, res.output
    assert [int(i) for i in re.findall(r"^copy-guard: sample (\d+) banned_columns \d+$", res.output, flags=re.M)] == [0, 1, 2]


def test_max_copy_needs_novelty_against(run_dir):
    from composer_amd import cli
    tmp, run = run_dir
    res = CliRunner().invoke(cli.cli, ["generate", "transformer", str(run), str(tmp / "x.data"), "--prompt-ids", "60,300", "--length", "8",
                                       "--max-copy", "8"])
    assert res.exit_code != 0 and "--max-copy goes with --novelty-against" in res.output, res.output
    (tmp / "empty" / "train").mkdir(parents=True, exist_ok=True)
    for bad in ("0", "65"):
        res = CliRunner().invoke(cli.cli, ["generate", "transformer", str(run), str(tmp / "x.data"), "--prompt-ids", "60,300", "--length", "8",
                                           "--novelty-against", str(tmp / "empty"), "--max-copy", bad])
        assert res.exit_code != 0 and "--max-copy %s: must be in [1, 64]" % bad in res.output, res.output
    assert not (tmp / "x.data").exists()
