"""-m gpu: `composer novelty` and `generate --novelty-against` end to end on a synthetic directory dataset: a file cut out of the
training set is found whole, its transposed copy only with --transpose, the --json arrays are the host restatement's
(composer_amd.novelty.match_table), and the lines `generate` prints equal Corpus.match on the ids it wrote while the files
themselves are those of the run without the option."""
import json
import re

import numpy as np
import pytest
import yaml
from click.testing import CliRunner

pytestmark = pytest.mark.gpu

CUT = (100, 160)               # the events of b.data the query file holds


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from composer_amd import dataset as ds
    root = tmp_path_factory.mktemp("novelty")
    train = root / "set" / "train"
    train.mkdir(parents=True)
    events = {name: ds.write_synthetic_data_file(train / (name + ".data"), 400, seed=i) for i, name in enumerate("abc")}
    cut = events["b"][CUT[0]:CUT[1]]
    ds.write_data_file(root / "cut.data", cut)
    up = [(t, v + 3 if t in (ds.NOTE_ON, ds.NOTE_OFF) and v + 3 <= 127 else v) for t, v in cut]
    ds.write_data_file(root / "cut_up3.data", up)
    files = sorted(train.glob("*.data"))
    ids, starts, names = ds.read_id_stream_pieces(files, (10, 100, 32))
    assert starts.tolist() == [0, 400, 800] and len(ids) == 1200
    return root, ids, starts


def table(env, path, min_match, N, fold=False):
    from composer_amd import dataset as ds, novelty
    import novelty_cases as nc
    _, ids, starts = env
    q = ds.read_data_file(path)[0].astype(np.int32)
    return q, novelty.match_table(ids, starts, q, nc.LAYOUT, min_match, N, nc.VELOCITY if fold else None)


def test_novelty_command(env, tmp_path):
    from composer_amd import cli
    root = env[0]
    out = tmp_path / "n.json"
    files = [str(root / "cut.data"), str(root / "cut_up3.data")]
    res = CliRunner().invoke(cli.cli, ["novelty", str(root / "set")] + files + ["--min-match", "4", "--json", str(out)])
    assert res.exit_code == 0, res.output
    n = CUT[1] - CUT[0]
    first = [l for l in res.output.splitlines() if l.startswith(files[0] + ":")][0]
    assert first.startswith("%s: events %d longest %d (" % (files[0], n, n)), first
    assert "in train/b.data offset %d transpose +0 coverage 1.000000" % CUT[0] in first, first
    rep = json.load(open(out))
    assert rep["corpus_events"] == 1200 and rep["min_match"] == 4 and rep["transpose"] == 0
    for f, entry in zip(files, rep["files"]):
        q, (ln, ps, ks) = table(env, f, 4, 0)
        assert entry["len"] == ln.tolist() and entry["pos"] == ps.tolist() and entry["k"] == ks.tolist(), f
    plain_longest = rep["files"][1]["longest"]["length"]
    # the transposed copy: found under k = -3 once the transpositions are tried
    res = CliRunner().invoke(cli.cli, ["novelty", str(root / "set"), files[1], "--min-match", "4", "--transpose", "3",
                                       "--ignore-velocity", "--json", str(out)])
    assert res.exit_code == 0, res.output
    rep = json.load(open(out))
    q, (ln, ps, ks) = table(env, files[1], 4, 3, fold=True)
    e = rep["files"][0]
    assert e["len"] == ln.tolist() and e["pos"] == ps.tolist() and e["k"] == ks.tolist()
    assert e["longest"]["transpose"] == -3 and e["longest"]["file"] == "train/b.data" and e["longest"]["length"] > plain_longest
    assert e["longest"]["offset"] == CUT[0] + e["longest"]["position"]
    assert e["coverage"] >= e["longest"]["length"] / n


def test_generate_novelty_against(env, tmp_path):
    from composer_amd import checkpoint as ckpt, cli, config, dataset as ds
    root = env[0]
    cfg = yaml.safe_load(open(cli.get_default_config()))
    cfg["transformer"]["model"].update(embedding_size=64, window_size=64, decoder_layers_count=2, attention_head_count=4)
    cfg["transformer"]["train"]["batch_size"] = 8
    cfg["transformer"]["runtime"] = {"dtype": "fp32", "seed": 0}
    run = tmp_path / "run"
    run.mkdir()
    (run / "config.yml").write_text(yaml.safe_dump(cfg))
    conf = config.get(run / "config.yml")
    model, _ = cli.create_model(cli.ModelType.TRANSFORMER, conf)              # freshly initialised
    ckpt.CheckpointManager(run, max_to_keep=1).save(model.state_dict(), {"step": 1, "epoch": 1})
    model.close()
    prompt = [60, 300, 188]
    common = ["--prompt-ids", ",".join(map(str, prompt)), "--length", "40", "--num-samples", "3"]
    (tmp_path / "plain").mkdir(); (tmp_path / "checked").mkdir()
    res = CliRunner().invoke(cli.cli, ["generate", "transformer", str(run), str(tmp_path / "plain" / "o.data")] + common)
    assert res.exit_code == 0, res.output
    assert "novelty:" not in res.output
    res = CliRunner().invoke(cli.cli, ["generate", "transformer", str(run), str(tmp_path / "checked" / "o.data")] + common
                             + ["--novelty-against", str(root / "set"), "--novelty-min-match", "1", "--novelty-transpose", "1"])
    assert res.exit_code == 0, res.output
    names = ["o-%d.data" % i for i in range(3)]
    assert sorted(p.name for p in (tmp_path / "checked").iterdir()) == names
    for nme in names:                                                          # the same files as without the option
        assert (tmp_path / "checked" / nme).read_bytes() == (tmp_path / "plain" / nme).read_bytes()
    logged = re.findall(r"^novelty: sample (\d+) (.*)$", res.output, flags=re.M)
    assert [int(i) for i, _ in logged] == [0, 1, 2]
    gen = [ds.read_data_file(tmp_path / "checked" / nme)[0].astype(np.int32)[len(prompt):] for nme in names]
    assert all(len(g) == 40 for g in gen)
    corpus = cli.open_novelty_corpus(str(root / "set"), conf)
    try:
        reports = corpus.match(gen, min_match=1, transpose=1)
        host = corpus.match_host(gen, min_match=1, transpose=1)
    finally:
        corpus.close()
    assert [line for _, line in logged] == [r.line() for r in reports] == [r.line() for r in host]
    assert any(r.longest[0] >= 1 for r in reports) and any(r.coverage < 1.0 for r in reports)      # (something to report, not everything)
