"""Times the copy guard (composer_amd/csrc/copyguard.hip; include/composer_hip.h, "copy guard") between HIP events on the stream the
work runs on: median of --iters timed calls after --warmup untimed ones.

    python tools/copy_guard_bench.py [--n 33554432] [--M 32] [--B 1,16,256] [--N 0,6] [--tokens 256] [--iters 5] [--warmup 1] [--out FILE]

1. The scan alone (cmp_k_copy_bans on device pointers): one JSON line per (B, N) with the time of a step's scan -- the init kernel and
   the scan kernel --, the bytes it has to move (the corpus once, 2 n bytes, plus the B windows, the static words and the ban words)
   and the time those bytes take at the HBM rate a streaming kernel reaches on this chip (6.3 TB/s), and the share of that.  The
   corpus is the one of tools/novelty_bench.py (random over a 54-id alphabet) with the first row's window planted once; every row's
   window ends on a token of that alphabet, so at B = 256 a corpus position meets about five rows in its bucket.  If the corpus were
   read once per row, the time at B = 256 would be 256 x that at B = 1: the two are printed side by side.
2. Decode with the guard on against the same build with it off: microseconds per token of --tokens ids behind a 16-id prompt, batch 1
   and B = 16, kv mode, on the C2 model shape (6 layers, 8 heads, width 512, window 1024), guard M = --M, N = 0, the same corpus."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch                    # before the library is loaded ("Library load order")

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from composer_amd import _lib, novelty                      # noqa: E402
from composer_amd.grammar import EventGrammar              # noqa: E402

HBM_BYTES_PER_SECOND = 6.3e12
V = 390


def make_inputs(n, M, Bmax, seed=0):
    rng = np.random.default_rng(seed)
    g = EventGrammar.from_dataset_params(10, 100, 32, rules=0)
    alphabet = np.asarray([288, 297, 259, 263, 388, 389] + [g.note_on0 + p for p in range(48, 72)] + [g.note_off0 + p for p in range(48, 72)])
    corpus = rng.choice(alphabet, size=n).astype(np.uint16)
    hist = rng.choice(alphabet, size=(Bmax, M)).astype(np.int32)
    corpus[n // 3:n // 3 + M] = hist[0]                    # one true copy of row 0's window ...
    corpus[n // 3 + M] = g.note_on0 + 60                   # ... continued by a note
    return g, corpus, hist


def timed(stream, fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def scan_lines(lib, a, g, corpus, hist, Bs, Ns):
    layout = g.to_c()
    D = lambda t: C.c_void_p(t.data_ptr())
    ids_dev = torch.from_numpy(corpus.view(np.int16)).cuda()
    nw = (V + 31) // 32
    out = []
    base = {}
    for N in Ns:
        for B in Bs:
            h_dev = torch.from_numpy(np.ascontiguousarray(hist[:B])).cuda()
            lens_dev = torch.full((B,), a.M, dtype=torch.int32, device="cuda")
            words = torch.empty((B, nw), dtype=torch.int32, device="cuda")
            count = torch.empty(B, dtype=torch.int64, device="cuda")
            o = _lib.CopyGuardOpts(a.M, N, 0, 0)

            def scan():
                s = torch.cuda.current_stream()
                _lib.check(lib.cmp_k_copy_bans(C.c_void_p(s.cuda_stream), D(ids_dev), a.n, None, C.byref(layout), C.byref(o), D(h_dev),
                                               D(lens_dev), B, a.M, V, None, D(words), D(count)), "cmp_k_copy_bans")
            ms = timed(torch.cuda.current_stream(), scan, a.iters, a.warmup)
            torch.cuda.synchronize()
            want = novelty.copy_bans(corpus[a.n // 3:a.n // 3 + a.M + 1], None, hist[0], V, g, a.M, N)
            got = np.unpackbits(words[0].cpu().numpy().view(np.uint8), bitorder="little")[:V].astype(bool)
            assert (got & want).sum() == want.sum() and want.any(), "the planted copy was not banned"
            med = statistics.median(ms)
            nbytes = 2.0 * a.n + B * a.M * 4 + B * 4 + 2 * B * nw * 4 + B * 8
            bound_us = nbytes / HBM_BYTES_PER_SECOND * 1e6
            base.setdefault(N, med)
            line = {"what": "scan", "n": a.n, "M": a.M, "B": B, "N": N, "us_median": med * 1e3, "us_min_max": [min(ms) * 1e3, max(ms) * 1e3],
                    "bytes_per_step": nbytes, "us_at_6.3_TB_per_s": bound_us, "share_of_hbm_rate": bound_us / (med * 1e3),
                    "times_the_first_B_of_this_N": med / base[N], "banned_columns_row0": int(count[0].item()), "iters": a.iters,
                    "warmup": a.warmup}
            print(json.dumps(line), flush=True)
            out.append(line)
    return out


def decode_lines(a, g, corpus):
    from composer_amd.transformer import Transformer
    out = []
    m = Transformer(V, 512, 1024, 6, 8, attention_dropout_rate=0.0, residual_dropout_rate=0.0, dtype="fp32", seed=0, max_batch=1,
                    max_seq=1024)
    m._lib.cmp_ctx_stream.restype = C.c_void_p
    stream = torch.cuda.ExternalStream(m._lib.cmp_ctx_stream(m._ctx))
    cp = novelty.Corpus(corpus, None, None, g, (256, 32))
    guard = cp.guard(a.M)
    rng = np.random.default_rng(1)
    for B in (1, 16):
        prompts = [rng.integers(0, V, 16).astype(np.int32) for _ in range(B)]
        res = {}
        for name, gd in (("off", None), ("on", guard)):
            def run():
                if B == 1:
                    m.generate(prompts[0], a.tokens, mode="kv", seed=3, copy_guard=gd)
                else:
                    m.generate_batch(prompts, a.tokens, mode="kv", seed=3, copy_guard=gd)
            ms = timed(stream, run, a.iters, a.warmup)
            res[name] = [v * 1e3 / a.tokens for v in ms]
        banned = [m.decode_copy_guard_state(B > 1, b) for b in range(B)]
        line = {"what": "decode", "B": B, "tokens": a.tokens, "n": a.n, "M": a.M, "N": 0,
                "us_per_token_off_median": statistics.median(res["off"]), "us_per_token_off_min_max": [min(res["off"]), max(res["off"])],
                "us_per_token_on_median": statistics.median(res["on"]), "us_per_token_on_min_max": [min(res["on"]), max(res["on"])],
                "banned_columns": banned, "iters": a.iters, "warmup": a.warmup,
                "note": "whole generate call (prefill of a 16-id prompt included) / tokens"}
        print(json.dumps(line), flush=True)
        out.append(line)
    cp.close()
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 25)
    ap.add_argument("--M", type=int, default=32)
    ap.add_argument("--B", default="1,16,256")
    ap.add_argument("--N", default="0,6")
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Bs, Ns = [int(v) for v in a.B.split(",")], [int(v) for v in a.N.split(",")]
    lib = _lib.load()
    _lib.require_gpu()                                     # no device: fail, never a host timing
    g, corpus, hist = make_inputs(a.n, a.M, max(Bs))
    lines = scan_lines(lib, a, g, corpus, hist, Bs, Ns)
    lines += decode_lines(a, g, corpus)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
