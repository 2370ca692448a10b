"""-m gpu: cmp_score / Transformer.score / `composer score` / `generate --keep-best` against the float64 oracle and against the decode
chain, on the gA golden configuration (V 390, E 64, H 4, L 2) at window_size 16.

Weights.  The golden parameters are a stddev-0.02 initialisation: nearly flat logits, where the rank of a target is decided by
differences far below the fp32 logits tolerance.  Every weight matrix (wte, wpe, the Conv1D weights) is multiplied by SCALE = 12:
max |z| ~ 8.5, mean entropy 4.6 nats, and the oracle alone puts the rank interval (below) at a single value at 383 of the 390
scored positions, 98.2 % (computed on the CPU from the float64 oracle before the value was fixed -- 94.6 % at 8, 98.7 % at 16,
where the float32 oracle already sits 2.3e-5 from float64; the test asserts >= 90 %).

Bounds.  The project holds fp32 logits to 1e-4 of the oracle; z[y] and logsumexp(z) each move by at most that, so
|logp - ref| <= 2e-4 + 1e-5 |ref|, and the same for the entropy.  The rank must lie in [#{c : z[c] > z[y] + 2e-4},
#{c != y : z[c] > z[y] - 2e-4}] of the oracle's float64 logits: every comparison against z[y] relaxed by 2e-4 either way.
Scoring against decoding: twice the bound tests/test_gpu_decode_logits.py holds the chain's logits to (two device paths, each
within 4 * floor + 1e-6 max |z| of the oracle, floor = max |z32 - z64| of the float32 oracle on the same contexts)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import yaml
from click.testing import CliRunner

from oracle import golden, transformer_oracle as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
W = 16
SCALE = 12.0
KEEPS = (1, W // 2, W - 1)
LENGTHS = (2, W, W + 1, W + 2, 2 * W + 3, 3 * W)
TOL_Z = 2e-4


def setup():
    """(V, E, H, L), params (float32, scaled, wpe cut to W rows), the sequences."""
    g = golden.load(os.path.join(HERE, "golden", "transformer_gA.npz"))
    V, E, H, L = [int(v) for v in g["cfg"]][:4]
    params = {k[6:]: g[k].astype(np.float64) for k in g.files if k.startswith("param:")}
    params["wpe/embeddings"] = params["wpe/embeddings"][:W]
    kinds = {n: kind for n, _, kind in O.param_specs(V, E, W, L)}
    params = {n: (v * SCALE if kinds[n] not in ("ones", "zeros") else v).astype(np.float32) for n, v in params.items()}
    rng = np.random.default_rng(5)
    seqs = [rng.integers(0, V, n).astype(np.int32) for n in LENGTHS]
    return (V, E, H, L), params, seqs


def oracle_of(dims, params, **kw):
    V, E, H, L = dims
    return O.OracleTransformer(O.Config(V, E, W, L, H), {k: v.astype(np.float64) for k, v in params.items()}, **kw)


def make_model(dims, params, dtype="fp32", max_batch=8):
    from composer_amd.transformer import Transformer
    V, E, H, L = dims
    m = Transformer(V, E, W, L, H, attention_dropout_rate=0.0, residual_dropout_rate=0.0, dtype=dtype, seed=0, max_batch=max_batch,
                    max_seq=W)
    m.set_weights(params)
    return m


_ROWS = {}


def contract_logits(orc, s, n, keep):
    """float64 logits s[n] is scored from: the last row of a forward pass over the contract's context (cached per context)."""
    from composer_amd.transformer import slide_context_length
    c = slide_context_length(n, W, keep)
    key = (id(orc), tuple(int(t) for t in s[n - c:n]))
    if key not in _ROWS:
        _ROWS[key] = np.asarray(orc.forward(np.asarray(s[n - c:n])[None])[0][0, -1], np.float64)
    return _ROWS[key]


def reduce64(z, y, tol=TOL_Z):
    """(logp, entropy, rank_lo, rank_hi) of one float64 logits row."""
    z = np.asarray(z, np.float64)
    mx = z.max()
    lse = mx + np.log(np.exp(z - mx).sum())
    p = np.exp(z - lse)
    ent = lse - (p * z).sum()
    others = np.delete(z, y)
    return z[y] - lse, ent, int((others > z[y] + tol).sum()), int((others > z[y] - tol).sum())


def reference(orc, s, keep):
    out = [reduce64(contract_logits(orc, s, n, keep), int(s[n])) for n in range(1, len(s))]
    return [np.array(col) for col in zip(*out)] if out else [np.zeros(0)] * 4


def single_valued_share(orc, seqs):
    lo_hi = [(lo, hi) for keep in KEEPS for s in seqs for lo, hi in zip(*reference(orc, s, keep)[2:])]
    return sum(lo == hi for lo, hi in lo_hi) / len(lo_hi)


@pytest.fixture(scope="module")
def env():
    dims, params, seqs = setup()
    orc = oracle_of(dims, params)
    m = make_model(dims, params)
    yield dims, params, seqs, orc, m
    m.close()


def test_score_matches_the_oracle(env):
    dims, params, seqs, orc, m = env
    single = total = 0
    worst = [0.0, 0.0]
    for keep in KEEPS:
        res = m.score(seqs, slide_keep=keep)
        assert len(res) == len(seqs)
        for s, r in zip(seqs, res):
            logp, ent, lo, hi = reference(orc, s, keep)
            assert len(r) == len(s) - 1 and r.targets.tolist() == s[1:].tolist()
            for k, (got, ref) in enumerate(((r.logp, logp), (r.entropy, ent))):
                q = np.abs(got - ref) / (2e-4 + 1e-5 * np.abs(ref))
                worst[k] = max(worst[k], float(q.max()))
                assert (q <= 1.0).all(), (keep, len(s), "logp" if k == 0 else "entropy", float(q.max()))
            assert ((r.rank >= lo) & (r.rank <= hi)).all(), (keep, len(s), r.rank.tolist(), lo.tolist(), hi.tolist())
            single += int((lo == hi).sum()); total += len(lo)
    print("\n[score-oracle] worst error / bound: logp %.3f entropy %.3f; rank interval single-valued at %d of %d positions"
          % (worst[0], worst[1], single, total))
    assert single >= 0.9 * total, (single, total)
    one = m.score(seqs[0], slide_keep=1)                       # one sequence in, one result out
    assert len(one) == 1 and one.logp[0] == m.score(seqs, slide_keep=1)[0].logp[0]
    lone = m.score([np.array([7])])                            # a sequence of length 1: empty arrays, no error
    assert len(lone) == 1 and len(lone[0]) == 0


def test_scoring_equals_decoding(env):
    """Greedy kv-slide decode, one id per call, the logits read after each: the teacher-forced score of prompt ++ ids must see the
    distribution every id was drawn from."""
    from composer_amd import _lib
    dims, params, seqs, orc, m = env
    V = dims[0]
    keep, P, n_gen = W // 2, 3, 2 * W + 6
    prompt = np.ascontiguousarray(seqs[-1][:P])
    z0 = np.zeros((1, P, V), np.float32)
    _lib.check(m._lib.cmp_forward_logits(m._h, prompt.ctypes.data_as(C.c_void_p), 1, P, z0.ctypes.data_as(C.c_void_p)), "forward_logits")
    _lib.check(m._lib.cmp_decode_begin_slide(m._h, prompt.ctypes.data_as(C.c_void_p), P, keep, 0.0, 0), "begin_slide")
    ids, Z, one = [], [z0[0, -1].copy()], np.zeros(1, np.int32)
    for k in range(n_gen):
        _lib.check(m._lib.cmp_decode_steps(m._h, 1, one.ctypes.data_as(C.c_void_p)), "steps")
        ids.append(int(one[0]))
        if k:
            Z.append(m.decode_logits())
    s = np.concatenate([prompt, np.array(ids, np.int32)])
    assert len(s) > 2 * W + P
    r = m.score(s, slide_keep=keep)
    # the chain's bound, from the two oracles on the contexts of the generated positions
    o32 = O.OracleTransformer(O.Config(V, dims[1], W, dims[3], dims[2]), params, dtype=np.float32)
    z64 = np.stack([contract_logits(orc, s, n, keep) for n in range(P, len(s))])
    z32 = np.stack([contract_logits(o32, s, n, keep) for n in range(P, len(s))])
    floor, zmax = float(np.abs(z32 - z64).max()), float(np.abs(z64).max())
    bound = 2 * (4 * floor + 1e-6 * zmax)
    worst, exact = 0.0, 0
    for k, n in enumerate(range(P, len(s))):
        assert int(np.argmax(Z[k])) == ids[k]                     # greedy: the drawn id is the chain's argmax (lowest index)
        logp, _, lo, hi = reduce64(Z[k], ids[k], tol=bound)
        err = abs(float(r.logp[n - 1]) - logp)
        worst = max(worst, err)
        assert err <= bound, (k, n, err, bound, floor)
        assert lo == 0 and lo <= r.rank[n - 1] <= hi, (k, n, int(r.rank[n - 1]), lo, hi)
        exact += int(r.rank[n - 1] == 0)
    print("\n[score-decode] worst |logp_score - logp_decode| %.3e bound %.3e (floor %.3e, max|z| %.2f); rank 0 at %d of %d"
          % (worst, bound, floor, zmax, exact, n_gen))
    assert exact >= 0.9 * n_gen


def test_packing_does_not_matter(env):
    """A ragged list in one call, every sequence alone, and a model whose workspace holds one window per call: the same figures to
    the fp32 bound (the GEMMs of passes with other row counts may sum in another order: no bitwise claim).  The rank of every
    packing lies in the oracle's relaxed interval: two packings can differ only where another column is within the fp32 tolerance
    of z[y], and are equal wherever the interval is a single value."""
    dims, params, seqs, orc, m = env
    together = m.score(seqs, slide_keep=W // 2)
    small = make_model(dims, params, max_batch=1)
    for s, a in zip(seqs, together):
        _, _, lo, hi = reference(orc, s, W // 2)
        assert ((a.rank >= lo) & (a.rank <= hi)).all(), (len(s), a.rank.tolist(), lo.tolist(), hi.tolist())
        for b in (m.score(s, slide_keep=W // 2), small.score(s, slide_keep=W // 2)):
            assert len(a) == len(b) and ((b.rank >= lo) & (b.rank <= hi)).all(), (len(s), b.rank.tolist(), lo.tolist(), hi.tolist())
            assert (a.rank == b.rank)[lo == hi].all()
            for x, y in ((a.logp, b.logp), (a.entropy, b.entropy)):
                assert (np.abs(x - y) <= 2e-4 + 1e-5 * np.abs(y)).all()
    small.close()


def test_bf16_mean_nll_of_a_full_row(env):
    dims, params, seqs, orc, m = env
    s = seqs[3][:W + 1]                                           # W inputs, W scored positions: one full-length row
    ob = oracle_of(dims, params, emulate_bf16=True)
    z = np.asarray(ob.forward(s[None, :W])[0][0], np.float64)
    ref = -np.mean([reduce64(z[t], int(s[t + 1]))[0] for t in range(W)])
    mb = make_model(dims, params, dtype="bf16")
    got = mb.score(s).nll_per_event
    mb.close()
    print("\n[score-bf16] mean NLL %.6f, emulate_bf16 oracle %.6f" % (got, ref))
    assert abs(got - ref) <= 2e-3 * ref, (got, ref)


def test_score_leaves_the_training_state_alone(env, monkeypatch):
    """cmp_score between the micro-steps of an accumulation group: parameters, G, iterations, the pending count and the final step's
    result are those of the run without it; and the last step's metrics stay readable behind a score call.  bf16 with
    COMPOSER_DETERMINISTIC=1: the one mode whose steps are bitwise reproducible (no float atomics), so the two runs are compared
    bit for bit."""
    from composer_amd import _lib
    monkeypatch.setenv("COMPOSER_DETERMINISTIC", "1")
    dims, params, seqs, orc, m0 = env
    V = dims[0]
    rng = np.random.default_rng(9)
    xs = rng.integers(0, V, (3, 2, W)).astype(np.int32)
    ys = rng.integers(0, V, (3, 2, W)).astype(np.int32)
    runs = []
    for with_score in (False, True):
        m = make_model(dims, params, dtype="bf16")
        m.set_train_options(clip_norm=1.0, accumulate_steps=3)
        out = []
        for j in range(3):
            out.append(m.train_step(xs[j], ys[j], 1e-2))
            if with_score:
                before = (m.train_options()["pending_micro_steps"], m.iterations, m.last_metrics(),
                          {n: m.get_parameter(n) for n in m.parameter_names})
                r = m.score(seqs, slide_keep=3)
                assert all(np.isfinite(q.logp).all() for q in r)
                assert m.train_options()["pending_micro_steps"] == before[0] == (j + 1) % 3
                assert m.iterations == before[1] and m.last_metrics() == before[2]
                assert all((m.get_parameter(n) == v).all() for n, v in before[3].items())
        runs.append((out, m.iterations, m.grad_stats(), {n: m.get_parameter(n) for n in m.parameter_names},
                     {n: m.get_parameter(n, _lib.KIND_GRAD) for n in m.parameter_names},
                     {n: m.get_parameter(n, _lib.KIND_ADAM_M) for n in m.parameter_names},
                     {n: m.get_parameter(n, _lib.KIND_ADAM_V) for n in m.parameter_names}))
        m.close()
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1] == 1 and a[2] == b[2]
    for k in (3, 4, 5, 6):
        assert all((a[k][n] == b[k][n]).all() for n in a[k]), k


def test_score_leaves_both_decode_chains_alone(env):
    """A batch-1 kv-slide chain and a batched kv-slide chain, both sampling at temperature 1 and both in flight on one model, stepped
    one id at a time; Transformer.score on a large ragged batch (its first call also allocates the inspection staging the entropy
    goes through) before the first slide, between the two chains' steps, and right after the slide.  The ids, decode_logits() and
    the batched logits of every step equal, bit for bit, those of the same run without the score calls."""
    from composer_amd import _lib
    dims, params, seqs, orc, m0 = env
    V = dims[0]
    keep, n_steps, B = 5, W + 12, 3                               # prompts of 3 .. 5 ids: the first slide comes at step 12 .. 14
    rng = np.random.default_rng(21)
    prompt = rng.integers(0, V, 4).astype(np.int32)
    rows = [rng.integers(0, V, n).astype(np.int32) for n in (3, 5, 4)]
    buf = np.zeros((B, 5), np.int32)
    for b, r in enumerate(rows):
        buf[b, :len(r)] = r
    lens = np.array([len(r) for r in rows], np.int32)
    big = [rng.integers(0, V, n).astype(np.int32) for n in (3 * W, 2 * W + 3, W + 2, W, 7, 2, 4 * W + 1)]
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    runs = []
    for with_score in (False, True):
        m = make_model(dims, params)
        lib, h = m._lib, m._h
        _lib.check(lib.cmp_decode_begin_slide(h, P(prompt), len(prompt), keep, 1.0, 77), "begin_slide")
        _lib.check(lib.cmp_decode_batch_begin_slide(h, P(buf), P(lens), B, buf.shape[1], keep, 1.0, 123), "batch_begin_slide")
        m._decode_batch_rows = B
        one, col = np.zeros(1, np.int32), np.zeros((B, 1), np.int32)
        ids, Z, idsb, Zb = [], [], [], []
        for k in range(n_steps):
            _lib.check(lib.cmp_decode_steps(h, 1, P(one)), "steps")
            ids.append(int(one[0]))
            if with_score and k in (5, 13):                       # between the two chains' steps
                m.score(big[:3], slide_keep=keep)
            _lib.check(lib.cmp_decode_batch_steps(h, 1, P(col)), "batch_steps")
            idsb.append(col[:, 0].copy())
            if k:
                Z.append(m.decode_logits())
                Zb.append(m.decode_batch_logits())
            if with_score and k in (2, 11, 12, 14, 15, 20):       # before, around and after the first slides of all four rows
                res = m.score(big, slide_keep=3)
                assert all(np.isfinite(r.logp).all() for r in res)
        runs.append((ids, np.array(Z), np.array(idsb), np.array(Zb), m.decode_slide_stats(False), m.decode_slide_stats(True)))
        m.close()
    a, b = runs
    assert a[4][0] >= 1 and a[5][0] >= B                          # every row slid at least once
    assert a[0] == b[0] and np.array_equal(a[2], b[2]) and a[4] == b[4] and a[5] == b[5]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    assert len(set(a[0])) > 3                                     # sampling, not a constant stream


def test_score_refuses_bad_input_ids(env):
    from composer_amd import _lib
    dims, params, seqs, orc, m = env
    x = np.array([[1, 2, dims[0]]], np.int32)
    y = np.array([[2, 3, 4]], np.int32)
    out = np.zeros((1, 3), np.float32)
    rc = m._lib.cmp_score(m._h, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), 1, 3, out.ctypes.data_as(C.c_void_p), None, None)
    assert rc == -1 and "outside" in _lib.last_error()
    with pytest.raises(ValueError):
        m.score([[1, 2, -1]])
    # a target outside [0, V) is the "not scored" mark, and null outputs are skipped
    x[0, 2] = 3
    y[0, 1] = -1
    rk = np.zeros((1, 3), np.int32)
    _lib.check(m._lib.cmp_score(m._h, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), 1, 3, out.ctypes.data_as(C.c_void_p),
                                rk.ctypes.data_as(C.c_void_p), None), "cmp_score")
    assert rk[0, 1] == -1 and out[0, 1] == 0 and rk[0, 0] >= 0 and out[0, 0] < 0


# ------------------------------------------------------------------------------------------------ CLI
def _restoredir(tmp_path, dims, params):
    """A restoredir the CLI can load: config.yml for this geometry and a checkpoint of `params`."""
    from composer_amd import checkpoint as ckpt, cli
    V, E, H, L = dims
    cfg = yaml.safe_load(open(cli.get_default_config()))
    cfg["transformer"]["model"].update(embedding_size=E, window_size=W, decoder_layers_count=L, attention_head_count=H)
    cfg["transformer"]["train"]["batch_size"] = 8
    cfg["transformer"]["runtime"] = {"dtype": "fp32", "seed": 0}
    d = tmp_path / "run"
    d.mkdir()
    (d / "config.yml").write_text(yaml.safe_dump(cfg))
    sd = {"model/" + n: v for n, v in params.items()}
    sd["optimizer/iter"] = np.int64(0)
    ckpt.CheckpointManager(d, max_to_keep=1).save(sd, {"step": 1, "epoch": 1})
    return d


def test_cli_score_on_data_and_midi_files(env, tmp_path):
    from composer_amd import cli, dataset as ds, notes as nt
    dims, params, seqs, orc, m = env
    run = _restoredir(tmp_path, dims, params)
    data = tmp_path / "piece.data"
    ds.write_synthetic_data_file(data, 3 * W + 5, seed=3)
    res = CliRunner().invoke(cli.cli, ["generate", "transformer", str(run), str(tmp_path / "gen.mid"), "--prompt-ids", "270,60,300,188",
                                       "--length", str(2 * W), "--decode-mode", "kv-slide", "--constrain"])
    assert res.exit_code == 0, res.output
    mid = tmp_path / "gen.mid"
    out = tmp_path / "scores.json"
    res = CliRunner().invoke(cli.cli, ["score", "transformer", str(run), str(data), str(mid), "--slide-keep", "5", "--by-event-type",
                                       "--json", str(out)])
    assert res.exit_code == 0, res.output
    ids = [ds.read_data_file(data)[0].astype(np.int32), np.array(nt.prompt_ids_from_midi(mid, None), np.int32)]
    assert len(ids[1]) > 1
    want = m.score(ids, slide_keep=5)
    lines = [l for l in res.output.splitlines() if " events " in l]
    assert len(lines) == 2
    rep = json.load(open(out))
    assert rep["slide_keep"] == 5 and rep["window_size"] == W and len(rep["files"]) == 2
    for path, line, r, e, seq in zip((data, mid), lines, want, rep["files"], ids):
        f = re.match(r"(.+): events (\d+) nll (\S+) bits (\S+) perplexity (\S+) top1 (\S+)$", line)
        assert f and f.group(1) == str(path) and int(f.group(2)) == r.events
        for got, ref in zip(f.groups()[2:], (r.nll_per_event, r.bits_per_event, r.perplexity, r.top1_accuracy)):
            assert float(got) == pytest.approx(ref, rel=1e-6)          # two models, two workspaces: the fp32 figures, not the bits
        assert e["file"] == str(path) and e["events"] == r.events
        assert np.allclose(e["logp"], r.logp, rtol=1e-5, atol=2e-4) and np.allclose(e["entropy"], r.entropy, rtol=1e-5, atol=2e-4)
        # the rank of both models inside the oracle's relaxed interval: they can differ only where another column lies within the
        # fp32 tolerance of z[y], and are equal wherever the interval is a single value
        _, _, lo, hi = reference(orc, seq, 5)
        cli_rank = np.array(e["rank"])
        assert len(cli_rank) == r.events and ((cli_rank >= lo) & (cli_rank <= hi)).all() and ((r.rank >= lo) & (r.rank <= hi)).all()
        assert (cli_rank == r.rank)[lo == hi].all()
        assert sum(v["count"] for v in e["by_event_type"].values()) == r.events
        assert e["nll_per_event"] == pytest.approx(-np.mean(np.array(e["logp"], np.float64)), rel=1e-9)   # the arrays round-trip
    assert sum(l.startswith("  ") and " count " in l for l in res.output.splitlines()) == 12


def test_cli_generate_keep_best(env, tmp_path):
    from composer_amd import cli, dataset as ds
    dims, params, seqs, orc, m = env
    run = _restoredir(tmp_path, dims, params)
    common = ["--prompt-ids", "60,300,188", "--length", str(W + 6), "--decode-mode", "kv-slide", "--slide-keep", "6", "--num-samples", "4"]
    (tmp_path / "all").mkdir(); (tmp_path / "best").mkdir()
    res = CliRunner().invoke(cli.cli, ["generate", "transformer", str(run), str(tmp_path / "all" / "o.data")] + common)
    assert res.exit_code == 0, res.output
    plain = [ds.read_data_file(tmp_path / "all" / ("o-%d.data" % i))[0].tolist() for i in range(4)]
    res = CliRunner().invoke(cli.cli, ["generate", "transformer", str(run), str(tmp_path / "best" / "o.data")] + common
                             + ["--keep-best", "2"])
    assert res.exit_code == 0, res.output
    assert sorted(p.name for p in (tmp_path / "best").iterdir()) == ["o-0.data", "o-1.data"]           # exactly two files
    kept = [ds.read_data_file(tmp_path / "best" / ("o-%d.data" % i))[0].tolist() for i in range(2)]
    logged = re.findall(r"keep-best: sample (\d+) seed (\d+) mean log-probability (\S+)", res.output)
    assert [int(i) for i, _, _ in logged] == [0, 1, 2, 3] and [int(s) for _, s, _ in logged] == [0, 1, 2, 3]
    scores = [float(v) for _, _, v in logged]
    order = sorted(range(4), key=lambda i: (-scores[i], i))[:2]
    assert re.search(r"keep-best: kept %d,%d\b" % tuple(order), res.output)
    assert kept == [plain[i] for i in order]                                                          # two of the four, best first
    # the logged score is the mean log-probability of the generated positions under Transformer.score
    for i in range(4):
        r = m.score(plain[i], slide_keep=6)
        assert scores[i] == pytest.approx(float(np.mean(r.logp[2:].astype(np.float64))), abs=2e-4)
