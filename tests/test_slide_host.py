"""CPU checks of the sliding-window decode's host surface: `slide_context_length` (the contract c(n) every layer uses) against a
step-by-step simulation of the cache, and the CLI's `--decode-mode kv-slide` / `--slide-keep` validation, which runs from the
restored config before a model (and so a device) is touched."""
import pytest
import yaml
from click.testing import CliRunner


def simulate_context_lengths(window, keep, n_max):
    """{n: tokens the draw at sequence length n sees}: the cache fills to `window`; the draw after that re-begins on `keep`"""
    out, c = {}, 0
    for n in range(1, n_max + 1):
        c = c + 1 if c < window else keep        # one more token cached, or the re-encode of the last `keep`
        out[n] = c
    return out


@pytest.mark.parametrize("window", [16, 160])
def test_slide_context_length_follows_the_simulation(window):
    from composer_amd.transformer import slide_context_length
    for keep in sorted({1, window // 2, window - 1, 7, window // 2 + 1}):
        sim = simulate_context_lengths(window, keep, 5 * window)
        for n, c in sim.items():
            assert slide_context_length(n, window, keep) == c, (window, keep, n)
        assert sim[window] == window and sim[window + 1] == keep
        period = window - keep + 1
        assert sim[window + 1 + period] == keep and (keep == window - 1 or sim[window + period] == window)


@pytest.mark.parametrize("window,keep", [(16, 0), (16, 16), (16, -1), (160, 161), (2, 2)])
def test_slide_context_length_refuses_keep_outside_the_range(window, keep):
    from composer_amd.transformer import slide_context_length
    with pytest.raises(ValueError, match="keep"):
        slide_context_length(window + 1, window, keep)


def test_slide_context_length_refuses_an_empty_sequence():
    from composer_amd.transformer import slide_context_length
    with pytest.raises(ValueError):
        slide_context_length(0, 16, 8)


def _restoredir(tmp_path, window=32):
    from composer_amd import cli
    cfg = yaml.safe_load(open(cli.get_default_config()))
    cfg["transformer"]["model"]["window_size"] = window
    d = tmp_path / "run"
    d.mkdir()
    (d / "config.yml").write_text(yaml.safe_dump(cfg))
    return d


@pytest.mark.parametrize("args,needle", [
    (["--decode-mode", "kv-slide", "--slide-keep", "0"], "window_size - 1"),
    (["--decode-mode", "kv-slide", "--slide-keep", "32"], "window_size - 1"),
    (["--decode-mode", "kv-cache", "--slide-keep", "8"], "kv-slide"),
    (["--slide-keep", "8"], "kv-slide"),
])
def test_cli_refuses_a_bad_slide_keep_before_any_device_use(tmp_path, monkeypatch, args, needle):
    from composer_amd import cli

    def no_model(*a, **k):
        raise AssertionError("the model was created before --slide-keep was validated")
    monkeypatch.setattr(cli, "create_model", no_model)
    res = CliRunner().invoke(cli.cli, ["generate", "transformer", str(_restoredir(tmp_path)), str(tmp_path / "o.data"),
                                       "--prompt-ids", "5,6,7"] + args)
    assert res.exit_code == 2, res.output            # click's usage-error status
    assert needle in res.output, res.output


def test_cli_accepts_kv_slide_as_a_decode_mode(tmp_path, monkeypatch):
    """a valid request passes the validation and reaches the model's creation (stopped there: no device in this test)"""
    from composer_amd import cli

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(cli, "create_model", stop)
    run = _restoredir(tmp_path)
    base = ["generate", "transformer", str(run), str(tmp_path / "o.data"), "--prompt-ids", "5,6,7"]
    for extra in ([], ["--slide-keep", "1"], ["--slide-keep", "31"]):
        res = CliRunner().invoke(cli.cli, base + ["--decode-mode", "kv-slide"] + extra)
        assert isinstance(res.exception, Reached), res.output
    res = CliRunner().invoke(cli.cli, base + ["--decode-mode", "kv-window"])
    assert res.exit_code == 2 and "kv-slide" in res.output      # an unknown mode: the choices listed name the new one
