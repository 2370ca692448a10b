"""CPU checks of truncated sampling's host surface: `sampling_keep_set` (the contract of include/composer_hip.h, "truncated
sampling", that the device sampler is held to by tests/test_gpu_sampling_truncation.py) against a brute-force restatement, the
argument rule, and the CLI's `--top-k` / `--top-p` validation, which runs from the arguments before a model (and so a device) is
touched.  The fixed logits rows of the GPU kernel-level test are built here, and their distance from a top-p boundary is asserted
here too, so a row that sits on a boundary is found without a GPU."""
import math

import numpy as np
import pytest
import yaml
from click.testing import CliRunner

DELTA = 1e-9            # a top-p case is undecidable when a cumulative mass lies this close to top_p (relative to the total): float64
                        # sums of < 4096 positive terms differ between two orders by < 4096 * 2^-53 ~ 5e-13, exp by a few ulp
KERNEL_MARGIN = 1e-6    # the fixed kernel-level rows keep at least this distance, so none of their cases is ever skipped
TEMPERATURES = (0.7, 1.0, 1.6)


def brute_keep_set(z, temperature, top_k, top_p):
    """The contract written out with Python floats (doubles) and a Python sort.  Returns (sorted kept columns, margin): margin
    is the smallest |cum[n] / total - top_p| over the candidates' prefixes (inf when top_p is off)."""
    z = [float(np.float32(v)) for v in z]
    V = len(z)
    order = sorted(range(V), key=lambda c: (-z[c], c))
    if 0 < top_k < V:
        order = order[:top_k]
    margin = math.inf
    tp = float(np.float32(top_p))
    if tp < 1.0:
        t = float(np.float32(temperature))
        q = [math.exp((z[c] - z[order[0]]) / t) for c in order]
        total = math.fsum(q)
        cum, n = 0.0, None
        for i, v in enumerate(q):
            cum += v
            margin = min(margin, abs(cum / total - tp))
            if n is None and cum >= tp * total:
                n = i + 1
        order = order[:n if n is not None else len(order)]
    return sorted(order), margin


def round3_row(V):
    """the logits row of tests/test_gpu_round3.py's sampler test: dominant columns, a -25 group, an exact tie"""
    z = np.random.default_rng(5).standard_normal(V).astype(np.float32) * 1.5
    z[[3, 77, 200]] += 4.0
    z[[10, 11, 12, 389]] = -25.0
    z[[20, 21]] = 0.5
    return z


def row97(seed=98):
    """V = 97: not a multiple of 64, fewer columns than threads (seed 97 put a cumulative mass 6.8e-7 from top_p = 0.95 at
    temperature 1, inside KERNEL_MARGIN: replaced, as test_the_fixed_kernel_rows_are_away_from_every_top_p_boundary asks)"""
    z = np.random.default_rng(seed).standard_normal(97).astype(np.float32) * 2.0
    z[[5, 50]] += 3.0
    z[[30, 31, 32]] = -1.25                      # an exact three-way tie
    return z


def straddle_row(V=390, k=40, seed=7):
    """an exact tie across the top-k cut: the columns at ranks k - 2 .. k + 1 (0-based) share one value, at scattered indices, so
    the cut keeps the two lower indices of the four"""
    z = np.random.default_rng(seed).standard_normal(V).astype(np.float32) * 1.5
    order = np.lexsort((np.arange(V), -z.astype(np.float64)))
    z[order[k - 2:k + 2]] = z[order[k - 2]]
    return z


def kp_cases(V):
    return [(0, 1.0), (1, 1.0), (40, 1.0), (0, 0.5), (0, 0.9), (0, 0.95), (40, 0.9), (V, 1.0)]


def kernel_rows():
    return [("round3-390", round3_row(390)), ("round3-1384", round3_row(1384)), ("v97", row97()), ("straddle", straddle_row())]


def test_keep_set_against_brute_force_on_random_rows():
    from composer_amd.transformer import sampling_keep_set
    rng = np.random.default_rng(0)
    cases = skipped = 0
    for V in (1, 2, 63, 97, 390, 1384):
        for trial in range(6):
            z = (rng.standard_normal(V) * rng.choice([0.3, 1.5, 6.0])).astype(np.float32)
            if V > 8 and trial % 2:
                z[rng.integers(0, V, 6)] = z[0]                   # exact ties somewhere in the order
            for t in TEMPERATURES:
                for k in (0, 1, 5, V - 1, V, V + 7):
                    for p in (1e-6, 0.5, 0.9, 1.0):
                        want, margin = brute_keep_set(z, t, k, p)
                        cases += 1
                        if margin < DELTA:
                            skipped += 1
                            continue
                        got = sampling_keep_set(z, t, k, p)
                        assert got.dtype == np.int64 and got.tolist() == want, (V, trial, t, k, p)
    assert skipped <= 0.01 * cases, (skipped, cases)


def test_keep_set_ties_across_the_k_and_the_p_boundary():
    from composer_amd.transformer import sampling_keep_set
    # four equal maxima at scattered indices: top_k = 2 keeps the two lowest indices
    z = np.full(16, -3.0, np.float32)
    z[[11, 2, 7, 14]] = 1.0
    assert sampling_keep_set(z, 1.0, 2, 1.0).tolist() == [2, 7]
    assert sampling_keep_set(z, 1.0, 3, 1.0).tolist() == [2, 7, 11]
    # top_p: the four equal columns hold 4 / (4 + 12 e^-4) = 0.948 of the mass, 0.237 each: p = 0.4 needs two of them, the lowest
    assert sampling_keep_set(z, 1.0, 0, 0.4).tolist() == [2, 7]
    assert sampling_keep_set(z, 1.0, 0, 0.6).tolist() == [2, 7, 11]
    # top-k first, then top-p over the renormalised candidates: of 3 equal candidates p = 0.5 needs two
    assert sampling_keep_set(z, 1.0, 3, 0.5).tolist() == [2, 7]
    # -0 and +0 are one value: the lower index first
    z = np.array([-1.0, 0.0, -0.0, -2.0], np.float32)
    assert sampling_keep_set(z, 1.0, 1, 1.0).tolist() == [1]
    z = np.array([-1.0, -0.0, 0.0, -2.0], np.float32)
    assert sampling_keep_set(z, 1.0, 1, 1.0).tolist() == [1]
    z = straddle_row()
    order = sorted(range(390), key=lambda c: (-float(z[c]), c))
    tied = [c for c in range(390) if z[c] == z[order[39]]]
    assert len(tied) == 4
    kept = sampling_keep_set(z, 1.0, 40, 1.0).tolist()
    assert [c for c in tied if c in kept] == sorted(tied)[:2]


def test_keep_set_special_rows():
    from composer_amd.transformer import sampling_keep_set
    V = 390
    one_hot = np.full(V, -30.0, np.float32)
    one_hot[123] = 10.0
    for k, p in ((0, 0.5), (0, 0.9), (5, 0.9), (0, 1e-6)):
        assert sampling_keep_set(one_hot, 1.0, k, p).tolist() == [123]
    assert sampling_keep_set(one_hot, 1.0, 5, 1.0).tolist() == [0, 1, 2, 3, 123]      # ties below the peak: lowest indices
    z = np.random.default_rng(1).standard_normal(V).astype(np.float32)
    assert sampling_keep_set(z, 1.0, 0, 1e-6).tolist() == [int(np.argmax(z))]        # top_p so small that one column is kept
    assert sampling_keep_set(z, 1.0, 0, 1.0).tolist() == list(range(V))               # both off: every column
    assert sampling_keep_set(z, 1.0, V, 1.0).tolist() == list(range(V))
    assert sampling_keep_set(z, 1.0, V + 7, 1.0).tolist() == list(range(V))
    assert len(sampling_keep_set(z, 1.0, V - 1, 1.0)) == V - 1
    assert sampling_keep_set(z, 0.0, 40, 0.9).tolist() == [int(np.argmax(z))]         # greedy: the argmax whatever the filters
    # a lower temperature sharpens the distribution: the nucleus does not grow
    assert len(sampling_keep_set(z, 0.7, 0, 0.9)) <= len(sampling_keep_set(z, 1.6, 0, 0.9))
    # -inf columns carry no mass and are dropped by any top_p < 1
    z2 = z.copy()
    z2[:100] = -np.inf
    assert min(sampling_keep_set(z2, 1.0, 0, 0.999999)) >= 100


@pytest.mark.parametrize("k,p", [(-1, 1.0), (0, 0.0), (0, -0.5), (0, 1.5), (0, float("nan")), (2.5, 1.0), (0, float("inf"))])
def test_keep_set_refuses_invalid_arguments(k, p):
    from composer_amd.transformer import sampling_keep_set
    with pytest.raises(ValueError, match="top_k|top_p"):
        sampling_keep_set(np.zeros(8, np.float32), 1.0, k, p)


def test_keep_set_refuses_an_empty_or_nan_row():
    from composer_amd.transformer import sampling_keep_set
    with pytest.raises(ValueError):
        sampling_keep_set(np.zeros(0, np.float32), 1.0, 0, 0.9)
    with pytest.raises(ValueError):
        sampling_keep_set(np.array([0.0, np.nan], np.float32), 1.0, 0, 0.9)


def test_the_fixed_kernel_rows_are_away_from_every_top_p_boundary():
    """The GPU test compares ids bitwise on these rows and skips none of their cases: every cumulative mass must be at least
    KERNEL_MARGIN away from top_p (a row that misses is replaced by another seed here, on the CPU)."""
    from composer_amd.transformer import sampling_keep_set
    for name, z in kernel_rows():
        for t in TEMPERATURES:
            for k, p in kp_cases(len(z)):
                want, margin = brute_keep_set(z, t, k, p)
                assert margin >= KERNEL_MARGIN, (name, t, k, p, margin)
                assert sampling_keep_set(z, t, k, p).tolist() == want, (name, t, k, p)


def _restoredir(tmp_path):
    from composer_amd import cli
    cfg = yaml.safe_load(open(cli.get_default_config()))
    d = tmp_path / "run"
    d.mkdir()
    (d / "config.yml").write_text(yaml.safe_dump(cfg))           # a restoredir holding only config.yml
    return d


@pytest.mark.parametrize("args,needle", [
    (["--top-p", "0"], "--top-p"),
    (["--top-p", "1.5"], "--top-p"),
    (["--top-p", "nan"], "--top-p"),
    (["--top-k", "-1"], "--top-k"),
    (["--top-k", "40", "--top-p", "-0.1", "--num-samples", "3"], "--top-p"),
])
def test_cli_refuses_bad_filters_before_any_device_use(tmp_path, monkeypatch, args, needle):
    from composer_amd import cli

    def no_model(*a, **k):
        raise AssertionError("the model was created before --top-k / --top-p were validated")
    monkeypatch.setattr(cli, "create_model", no_model)
    res = CliRunner().invoke(cli.cli, ["generate", "transformer", str(_restoredir(tmp_path)), str(tmp_path / "o.data"),
                                       "--prompt-ids", "5,6,7"] + args)
    assert res.exit_code == 2, res.output            # click's usage-error status
    assert needle in res.output and "must be" in res.output, res.output


def test_cli_accepts_valid_filters(tmp_path, monkeypatch):
    """a valid request passes the validation and reaches the model's creation (stopped there: no device in this test)"""
    from composer_amd import cli

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(cli, "create_model", stop)
    run = _restoredir(tmp_path)
    base = ["generate", "transformer", str(run), str(tmp_path / "o.data"), "--prompt-ids", "5,6,7"]
    for extra in (["--top-k", "40"], ["--top-p", "0.9"], ["--top-k", "0", "--top-p", "1"], ["--top-k", "40", "--top-p", "0.9",
                                                                                           "--num-samples", "3"]):
        res = CliRunner().invoke(cli.cli, base + extra)
        assert isinstance(res.exception, Reached), res.output
