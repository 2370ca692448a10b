#!/usr/bin/env python3
"""Batched decode throughput (Transformer.generate_batch) at the C5 geometry of bench.py:decode_bench -- 6L/8H/d512, window 2048,
a 10-id prompt per row, 1024 tokens, temperature 1.0 -- for B in {1, 8, 32, 64}, beside the batch-1 `generate` of the same
process.  One JSON line.  Each B is warmed up (the first call allocates and captures its chain); every time is the best of 3
host-clock runs around calls that end in a device sync.  Two times per B: `tokens_per_s` / `speedup_vs_batch1` over the whole call
(begin -- B per-row prefills, each followed by a sync -- plus the steps, as batch 1's `generate` is timed), and `us_per_step` over
cmp_decode_batch_steps alone (begin run outside the timed region; N ids = N - 1 chain replays).  bytes/step = the fp32 decode
weights (read once per step for all rows) + every row's K/V rows up to the mean position; GB/s and the fraction of the HBM peak
follow from the steps-only time.
    python tools/decode_batch_bench.py [--batches 1,8,32,64] [--tokens 1024]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (load order: torch before the library)

PEAK_HBM_GBS = 8000.0


def best_of(fn, reps=3):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32,64")
    ap.add_argument("--tokens", type=int, default=1024)
    a = ap.parse_args()
    from composer_amd import _lib
    from composer_amd._lib import check
    from composer_amd.transformer import Transformer
    V, E, H, L, W, P0, N = 390, 512, 8, 6, 2048, 10, a.tokens
    m = Transformer(V, E, W, L, H, attention_dropout_rate=0.0, residual_dropout_rate=0.0, dtype="fp32", seed=0, max_batch=1,
                    max_seq=64)
    rng = np.random.default_rng(0)
    nparam = sum(int(np.prod(m.parameter_shape(n))) for n in m.parameter_names)
    weight_bytes = 4 * (nparam - W * E + E)
    mean_pos = P0 + (N - 1) / 2.0
    kv_row = 4 * (2 * L * mean_pos * E + 2 * L * E)
    prompt = rng.integers(0, V, P0)
    m.generate(prompt, 32, temperature=1.0, mode="kv", seed=1)
    t1 = best_of(lambda: m.generate(prompt, N, temperature=1.0, mode="kv", seed=1))
    lib, h = m._lib, m._h
    batches = [int(b) for b in a.batches.split(",")]
    ids = np.empty(max(batches + [1]) * N, np.int32)

    def steps_only(begin, steps):
        best = None
        for _ in range(3):
            check(begin(), "begin")
            t0 = time.perf_counter()
            check(steps(), "steps")
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best / (N - 1)

    p32 = np.ascontiguousarray(prompt, np.int32)
    s1 = steps_only(lambda: lib.cmp_decode_begin(h, p32.ctypes.data_as(C.c_void_p), P0, _lib.DECODE_KV, 1.0, 1),
                    lambda: lib.cmp_decode_steps(h, N, ids.ctypes.data_as(C.c_void_p)))
    out = {"metric": "batched decode (generate_batch, C5, temp 1.0, KV cache + hipGraph)", "tokens": N, "prompt": P0,
           "batch1_generate": {"us_per_token": 1e6 * t1 / N, "tokens_per_s": N / t1, "us_per_step": 1e6 * s1}, "batched": {}}
    for B in batches:
        rows = [rng.integers(0, V, P0).tolist() for _ in range(B)]
        m.generate_batch(rows, 32, temperature=1.0, mode="kv", seed=1)
        t = best_of(lambda: m.generate_batch(rows, N, temperature=1.0, mode="kv", seed=1))
        buf = np.ascontiguousarray(rows, np.int32)
        lens = np.full(B, P0, np.int32)
        step = steps_only(lambda: lib.cmp_decode_batch_begin(h, buf.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), B,
                                                             P0, _lib.DECODE_KV, 1.0, 1),
                          lambda: lib.cmp_decode_batch_steps(h, N, ids.ctypes.data_as(C.c_void_p)))
        bps = weight_bytes + B * kv_row
        out["batched"][str(B)] = {"us_per_step": 1e6 * step, "tokens_per_s": B * N / t, "bytes_per_step": bps,
                                  "gb_per_s": bps / step / 1e9, "frac_hbm_peak": bps / step / 1e9 / PEAK_HBM_GBS,
                                  "speedup_vs_batch1": (B * N / t) / (N / t1)}
    m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
