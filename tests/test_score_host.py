"""Not-GPU tests of the host side of scoring (include/composer_hip.h, "scoring"): the window plan against the sliding-window
context rule, the ragged packing against a fake cmp_score, the figures a result derives, and the CLI refusals of --keep-best."""
import math

import numpy as np
import pytest
import yaml
from click.testing import CliRunner

from composer_amd import dataset as ds
from composer_amd.transformer import SequenceScore, score_sequences, score_windows, slide_context_length


@pytest.mark.parametrize("W", [4, 16])
def test_score_windows_realise_the_contract(W):
    for keep in range(1, W):
        for n in range(1, 4 * W + 4):
            wins = score_windows(n, W, keep)
            if n == 1:
                assert wins == []
                continue
            assert wins[0] == (0, min(n - 1, W), 0)
            seen = {}
            for j, (start, length, first) in enumerate(wins):
                assert 1 <= length <= W and 0 <= first < length and start >= 0 and start + length <= n - 1, (n, keep, wins)
                if j >= 1:
                    assert start == W + 1 + (j - 1) * (W - keep + 1) - keep and first == keep - 1
                for r in range(first, length):
                    pos = start + r + 1                      # row r holds the logits of this position, context s[start : pos]
                    assert pos not in seen, (n, keep, pos)
                    seen[pos] = (start, r + 1)
            assert sorted(seen) == list(range(1, n)), (n, keep)
            for pos, (start, ctx) in seen.items():
                assert ctx == slide_context_length(pos, W, keep) and start + ctx == pos, (n, keep, pos)


def test_score_windows_refuse_bad_arguments():
    for keep in (0, 4, -1):
        with pytest.raises(ValueError):
            score_windows(10, 4, keep)
    with pytest.raises(ValueError):
        score_windows(0, 4, 2)


@pytest.mark.parametrize("max_tokens", [1, 8, 20, 1000])
@pytest.mark.parametrize("keep", [1, 4, 7])
def test_ragged_packing_puts_every_tag_in_its_slot(max_tokens, keep):
    W = 8
    lengths = [1, 2, W, W + 1, W + 2, 2 * W + 3]
    seqs = [np.array([1000 * (k + 1) + i for i in range(n)]) for k, n in enumerate(lengths)]
    calls = []

    def fake(x, y):
        """Echoes the target's (sequence, position) tag through logp, the first input of the row's context through entropy and the
        row number through rank; checks the padding rules on the way."""
        B, T = x.shape
        assert x.dtype == np.int32 and y.dtype == np.int32 and y.shape == (B, T) and B * T <= max(max_tokens, T)
        calls.append((B, T))
        for b in range(B):
            scored = np.flatnonzero(y[b] >= 0)
            assert scored.size and (np.diff(scored) == 1).all()                  # one run of scored rows ...
            assert (x[b, scored[-1] + 1:] == 0).all() and (y[b, scored[-1] + 1:] == -1).all()   # ... then id 0 / target -1
            # teacher forcing: a scored row's target is the next row's input
            assert (y[b, scored[:-1]] == x[b, scored[:-1] + 1]).all()
        return y.astype(np.float32), np.tile(np.arange(T, dtype=np.int32), (B, 1)), np.repeat(x[:, :1], T, 1).astype(np.float32)

    res = score_sequences(fake, seqs, W, keep, max_tokens)
    assert len(res) == len(seqs)
    for k, (s, r) in enumerate(zip(seqs, res)):
        assert len(r) == len(s) - 1 and r.targets.tolist() == s[1:].tolist()
        assert r.logp.tolist() == s[1:].astype(np.float32).tolist(), k
        for pos in range(1, len(s)):
            c = slide_context_length(pos, W, keep)
            assert r.rank[pos - 1] == c - 1 and r.entropy[pos - 1] == s[pos - c], (k, pos)
    assert res[0].logp.size == 0 and res[0].rank.dtype == np.int32
    if max_tokens >= 1000:
        assert len(calls) == 1                                   # everything fits one call
    if max_tokens == 1:
        assert all(B == 1 for B, _ in calls)                     # a window is never split: one per call when nothing more fits


def test_sequence_score_figures():
    rng = np.random.default_rng(0)
    vr = ds.event_value_ranges(10, 100, 32)
    rg = ds.event_ranges(vr)
    V = ds.vocab_size(10, 100, 32)
    targets = rng.integers(0, V, 500).astype(np.int32)
    targets[:3] = [388, 389, 0]
    logp = -rng.random(500).astype(np.float32) * 5
    rank = rng.integers(0, 4, 500).astype(np.int32)
    r = SequenceScore(targets, logp, rank, np.ones(500, np.float32))
    nll = -logp.astype(np.float64).mean()
    assert r.events == 500 and r.nll_per_event == pytest.approx(nll, rel=1e-12)
    assert r.bits_per_event == pytest.approx(nll / math.log(2), rel=1e-12)
    assert r.perplexity == pytest.approx(math.exp(nll), rel=1e-12)
    assert r.top1_accuracy == (rank == 0).mean()
    # by_event_type against np.bincount over the class of every target
    cls = np.zeros(V, np.int64)
    for t, interval in rg.items():
        cls[interval.start:interval.stop] = t
    counts = np.bincount(cls[targets], minlength=7)
    sums = np.bincount(cls[targets], weights=-logp.astype(np.float64), minlength=7)
    got = r.by_event_type(rg)
    assert list(got) == list(rg) and sum(c for c, _ in got.values()) == 500
    for t in rg:
        assert got[t][0] == counts[t]
        assert got[t][1] == pytest.approx(sums[t] / counts[t], rel=1e-12)
    d = r.to_dict()
    assert d["events"] == 500 and d["rank"] == rank.tolist() and d["logp"] == [float(v) for v in logp]
    empty = SequenceScore([], [], [], [])
    assert len(empty) == 0 and math.isnan(empty.nll_per_event) and math.isnan(empty.perplexity) and math.isnan(empty.top1_accuracy)
    assert all(c == 0 and math.isnan(v) for c, v in empty.by_event_type(rg).values())
    with pytest.raises(ValueError):
        SequenceScore([1, 2], [0.0], [0], [0.0])


def _restoredir(tmp_path):
    from composer_amd import cli
    cfg = yaml.safe_load(open(cli.get_default_config()))
    d = tmp_path / "run"
    d.mkdir()
    (d / "config.yml").write_text(yaml.safe_dump(cfg))           # a restoredir holding only config.yml
    return d, cfg["transformer"]["model"]["window_size"]


def test_keep_best_is_refused_before_any_device_work(tmp_path, monkeypatch):
    from composer_amd import cli

    def no_model(*a, **k):
        raise AssertionError("the model was created before --keep-best was validated")
    monkeypatch.setattr(cli, "create_model", no_model)
    run, W = _restoredir(tmp_path)
    base = ["generate", "transformer", str(run), str(tmp_path / "o.data"), "--prompt-ids", "5,6,7"]
    for args, needle in ((["--keep-best", "0"], "--keep-best 0"), (["--keep-best", "2"], "--keep-best 2"),
                         (["--num-samples", "3", "--keep-best", "4"], "--keep-best 4"),
                         (["--num-samples", "3", "--keep-best", "-1"], "--keep-best -1")):
        res = CliRunner().invoke(cli.cli, base + args)
        assert res.exit_code == 2 and needle in res.output and "--num-samples" in res.output, res.output
    res = CliRunner().invoke(cli.cli, ["generate", "transformer", str(run), str(tmp_path / "o.data"), "--prompt-ids", "",
                                       "--num-samples", "2", "--keep-best", "1", "--length", "8"])
    assert res.exit_code == 2 and "--keep-best" in res.output and "empty" in res.output, res.output
    # the reference's literal loop past the window cannot be scored: named, explicit or chosen by default
    for mode in (["--decode-mode", "reference-literal"], []):
        res = CliRunner().invoke(cli.cli, base + mode + ["--num-samples", "2", "--keep-best", "1", "--length", str(W)])
        assert res.exit_code == 2 and "reference-literal" in res.output and "--keep-best" in res.output, res.output


def test_keep_best_reaches_the_model_when_it_can_be_scored(tmp_path, monkeypatch):
    from composer_amd import cli

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(cli, "create_model", stop)
    run, W = _restoredir(tmp_path)
    base = ["generate", "transformer", str(run), str(tmp_path / "o.data"), "--prompt-ids", "5,6,7", "--num-samples", "3"]
    for extra in (["--keep-best", "1", "--length", "16"], ["--keep-best", "3", "--length", str(W - 2)],
                  ["--keep-best", "2", "--decode-mode", "kv-slide", "--length", str(2 * W)],
                  ["--keep-best", "1", "--decode-mode", "reference-literal", "--length", str(W - 3)], []):
        res = CliRunner().invoke(cli.cli, base + extra)
        assert isinstance(res.exception, Reached), res.output


def test_score_command_refusals(tmp_path, monkeypatch):
    from composer_amd import cli

    def no_model(*a, **k):
        raise AssertionError("the model was created before the arguments were validated")
    monkeypatch.setattr(cli, "create_model", no_model)
    run, W = _restoredir(tmp_path)
    good = tmp_path / "a.data"
    ds.write_synthetic_data_file(good, 20, seed=1)
    other = tmp_path / "b.data"
    ds.write_synthetic_data_file(other, 20, seed=1, velocity_bins=16)
    res = CliRunner().invoke(cli.cli, ["score", "transformer", str(run), str(good), "--slide-keep", str(W)])
    assert res.exit_code == 2 and "--slide-keep" in res.output, res.output
    res = CliRunner().invoke(cli.cli, ["score", "transformer", str(run), str(other)])
    assert res.exit_code == 1 and "preprocessed with" in res.output, res.output
    res = CliRunner().invoke(cli.cli, ["score", "transformer", str(run), str(tmp_path / "c.txt")])
    assert res.exit_code == 2 and ".data" in res.output, res.output
    res = CliRunner().invoke(cli.cli, ["score", "transformer", str(run)])
    assert res.exit_code == 2, res.output
