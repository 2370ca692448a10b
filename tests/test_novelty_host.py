"""CPU: the host restatement of the novelty check (composer_amd/novelty.py) against a triple-loop statement of the recurrence of
include/composer_hip.h, the case builder's features, NoveltyReport on hand-written arrays, every refusal that is decided on the host
and the CLI's usage errors -- none of it touches a device."""
import numpy as np
import pytest
from click.testing import CliRunner

import novelty_cases as nc
from composer_amd import novelty
from composer_amd.dataset import write_synthetic_data_file


def test_the_cases_cover_what_they_were_built_for():
    missing = set(nc.ALL_FEATURES) - nc.covered()
    assert not missing, missing


def naive_equal(xt, ct, k, layout, vel):
    """Token equality of the contract, one pair at a time."""
    if vel is not None and vel[0] <= xt < vel[0] + vel[1]:
        return vel[0] <= ct < vel[0] + vel[1]
    if layout is not None:
        for base in (layout.note_on0, layout.note_off0):
            if base <= xt < base + 128:
                p = xt - base + k
                return 0 <= p <= 127 and ct == base + p
    return xt == ct


def naive_table(corpus, starts, x, layout, min_match, N, vel):
    n, L = len(corpus), len(x)
    is_start = set(int(s) for s in starts)
    best = [(0, 0, 0, 0)] * L                                  # keys (m, -|k|, k < 0, -p)
    for k in range(-N, N + 1):
        m = [[0] * (n + 1) for _ in range(L + 1)]
        for s in range(L - 1, -1, -1):
            for p in range(n - 1, -1, -1):
                if naive_equal(int(x[s]), int(corpus[p]), k, layout, vel):
                    cont = 0 if (s + 1 == L or p + 1 == n or (p + 1) in is_start) else m[s + 1][p + 1]
                    m[s][p] = 1 + cont
                    best[s] = max(best[s], (m[s][p], -abs(k), 1 if k < 0 else 0, -p, k))
    ln, ps, ks = np.zeros(L, np.int32), np.full(L, -1, np.int64), np.zeros(L, np.int32)
    for s, b in enumerate(best):
        if b[0] >= min_match:
            ln[s], ps[s], ks[s] = b[0], -b[3], b[4]
    return ln, ps, ks


@pytest.mark.parametrize("name", nc.SMALL)
def test_match_table_equals_the_triple_loop(name):
    c = nc.case(name)
    ref = nc.reference(name)
    for b, row in enumerate(c.rows):
        ln, ps, ks = naive_table(c.corpus, c.starts, row, c.layout, c.min_match, c.N, c.velocity)
        for got, want in zip((ref[0][b], ref[1][b], ref[2][b]), (ln, ps, ks)):
            assert np.array_equal(got[:len(row)], want), (name, b, np.argwhere(got[:len(row)] != want)[:4].tolist())
        assert (ref[0][b, len(row):] == 0).all() and (ref[1][b, len(row):] == -1).all() and (ref[2][b, len(row):] == 0).all()


def test_report_on_hand_written_arrays():
    #      s:  0  1  2  3  4  5  6  7  8  9
    length = [0, 3, 2, 0, 0, 0, 4, 3, 0, 0]
    pos = [-1, 10, 11, -1, -1, -1, 25, 26, -1, -1]
    k = [0, 0, 0, 0, 0, 0, -2, -2, 0, 0]
    ids = [5, 288, 290, 7, 7, 7, 288 + 99, 3, 288 + 49, 130]
    r = novelty.NoveltyReport(length, pos, k, ids, starts=[0, 20, 40], names=["a", "b", "c"], layout=nc.LAYOUT, time_step_ms=10)
    assert r.coverage == 7 / 10                                            # [1, 4) and [6, 10)
    assert r.longest == (4, 6, "b", 5, -2)
    assert r.longest_seconds == (100 + 50) * 10 / 1000.0                   # the two TIME_SHIFTs inside [6, 10)
    none = novelty.NoveltyReport([0, 0], [-1, -1], [0, 0])
    assert none.longest == (0, -1, None, -1, 0) and none.coverage == 0.0 and none.longest_seconds == 0.0
    assert novelty.coverage_of([5, 0, 0]) == 1.0                            # an interval is clipped to the query
    tie = novelty.NoveltyReport([2, 0, 2, 0], [8, -1, 1, -1], [0, 0, 1, 0], starts=[0], names=["only"])
    assert tie.longest == (2, 0, "only", 8, 0)                             # the first of equals


def test_a_piece_matches_itself_whole():
    c = nc.case("n5000_fold")
    bounds = list(c.starts) + [c.n]
    i = int(np.argmin(np.diff(bounds)))                    # the shortest piece
    a, b = int(bounds[i]), int(bounds[i + 1])
    piece = c.corpus[a:b].astype(np.int32)
    assert 1 <= len(piece) <= 2000
    ln, ps, ks = novelty.match_table(c.corpus, c.starts, piece, c.layout, 1, 2, None)
    assert ln[0] == len(piece) and ps[0] <= a and ks[0] == 0 and novelty.coverage_of(ln) == 1.0
    assert (ln == len(piece) - np.arange(len(piece))).all()            # nothing runs on across the piece's end


def test_every_refusal_that_is_decided_on_the_host():
    ids = np.arange(100, dtype=np.uint16)
    V = nc.VELOCITY
    for kw in (dict(starts=[1, 5]), dict(starts=[0, 7, 3]), dict(starts=[0, 100]), dict(starts=[]), dict(starts=[0, -1]),
               dict(starts=[0, 5], names=["a"]), dict(velocity_range=(-1, 4)), dict(velocity_range=(65530, 10)),
               dict(layout=nc.LAYOUT, velocity_range=(100, 40)), dict(layout=nc.LAYOUT, velocity_range=(250, 10))):
        with pytest.raises(ValueError):
            novelty.Corpus(ids, **kw)
    with pytest.raises(ValueError):
        novelty.Corpus(ids[:1])
    with pytest.raises(ValueError):
        novelty.Corpus(np.asarray([0, 70000]))
    plain = novelty.Corpus(ids)
    full = novelty.Corpus(ids, [0, 50], ["a", "b"], nc.LAYOUT, V)
    q = [1, 2, 3]
    for corpus, seqs, kw in ((full, [q], dict(min_match=0)), (full, [q], dict(transpose=-1)), (full, [q], dict(transpose=25)),
                             (plain, [q], dict(transpose=1)),                         # no layout
                             (plain, [q], dict(ignore_velocity=True)),                # no velocity range
                             (full, [[]], {}), (full, [[1, -1]], {}), (full, [[65535]], {}), (full, [[0] * 32769], {}),
                             (full, [], {})):
        with pytest.raises(ValueError):
            corpus.match_arrays(seqs, **kw)
        if seqs:
            with pytest.raises(ValueError):
                corpus.match(seqs, **kw)
        assert corpus._ds is None                                  # refused before any device use
    with pytest.raises(ValueError):
        full.match_arrays([q] * 257)
    with pytest.raises(ValueError):
        novelty.match_table(ids, None, q, None, 1, 1)              # N > 0 without a layout
    bad = type("L", (), dict(note_on0=0, note_off0=100, time_shift0=288, time_shift_n=100))()
    with pytest.raises(ValueError):
        novelty.match_table(ids, None, q, bad, 1, 0)               # overlapping note ranges
    assert [r.longest[0] for r in full.match_host([[10, 11, 12, 13]], min_match=2)] == [4]


def test_cli_usage_errors_come_before_any_device_use(tmp_path, monkeypatch):
    from composer_amd import cli, _lib
    monkeypatch.setattr(_lib, "require_gpu", lambda: (_ for _ in ()).throw(AssertionError("the device was asked for")))
    (tmp_path / "set" / "train").mkdir(parents=True)
    write_synthetic_data_file(tmp_path / "set" / "train" / "a.data", 50, seed=1)
    q = str(tmp_path / "set" / "train" / "a.data")
    (tmp_path / "q.txt").write_text("x")
    run = CliRunner().invoke
    for args in (["novelty", str(tmp_path / "set"), q, "--min-match", "0"],
                 ["novelty", str(tmp_path / "set"), q, "--transpose", "25"],
                 ["novelty", str(tmp_path / "set"), q, "--transpose", "-1"],
                 ["novelty", str(tmp_path / "set"), q, "-c", "a.yml", "--restoredir", "b"],
                 ["novelty", str(tmp_path / "nowhere"), q],
                 ["novelty", str(tmp_path / "set"), q, "--split", "test"],
                 ["novelty", str(tmp_path / "set"), str(tmp_path / "q.txt")],
                 ["novelty", str(tmp_path / "set")],
                 ["generate", "transformer", "restore", "out.mid", "--prompt-ids", "1", "--novelty-min-match", "4"],
                 ["generate", "transformer", "restore", "out.mid", "--prompt-ids", "1", "--novelty-transpose", "2"],
                 ["generate", "transformer", "restore", "out.mid", "--prompt-ids", "1", "--novelty-against", str(tmp_path / "nowhere")],
                 ["generate", "transformer", "restore", "out.mid", "--prompt-ids", "1", "--novelty-against", str(tmp_path / "set"),
                  "--novelty-min-match", "0"],
                 ["generate", "transformer", "restore", "out.mid", "--prompt-ids", "1", "--novelty-against", str(tmp_path / "set"),
                  "--novelty-transpose", "30"],
                 ["generate", "transformer", "restore", "out.mid", "--prompt-ids", "1", "--novelty-against", str(tmp_path / "set"),
                  "--length", "40000"]):
        r = run(cli.cli, args)
        assert r.exit_code == 2 and "Usage:" in r.output, (args, r.exit_code, r.output[-300:])
