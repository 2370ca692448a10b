#!/usr/bin/env python3
"""Sliding-window decode (`kv-slide`) cost at the C5 geometry of bench.py:decode_bench -- 6L/8H/d512, window 2048, keep 1024, a
10-id prompt per row, 4 * W ids, temperature 1.0 -- for B in {1, 64}.  One JSON line.  Per B:
  kv_us_per_step        plain kv mode, cmp_decode*_steps alone over 1024 ids (begin outside the timed region), from the same process
  slide_us_per_step     kv-slide, cmp_decode*_steps alone over all 4 * W ids, its slides included
  one_slide_ms          one slide of all B rows (gather + re-encode + cache fill + draw): a begin on full-window prompts (P = W), the
                        prefill's ids taken, then ONE timed steps(1) call, which is that slide and ends in a device sync
  row_slides / forward_calls   cmp_decode_slide_stats of the long run
Every time is the best of 3 host-clock runs around calls that end in a device sync.
    python tools/decode_slide_bench.py [--batches 1,64] [--keep 1024] [--ids 8192]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (load order: torch before the library)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--keep", type=int, default=1024)
    ap.add_argument("--ids", type=int, default=8192)
    ap.add_argument("--max-batch", type=int, default=32, help="workspace = max_batch * window tokens (rows per re-encode call = that / keep)")
    a = ap.parse_args()
    from composer_amd import _lib
    from composer_amd._lib import check
    from composer_amd.transformer import Transformer
    V, E, H, L, W, P0, N, NKV = 390, 512, 8, 6, 2048, 10, a.ids, 1024
    m = Transformer(V, E, W, L, H, attention_dropout_rate=0.0, residual_dropout_rate=0.0, dtype="fp32", seed=0, max_batch=a.max_batch,
                    max_seq=W)
    lib, h = m._lib, m._h
    rng = np.random.default_rng(0)
    out = {"metric": "sliding-window decode (C5, temp 1.0, keep %d, %d ids)" % (a.keep, N), "keep": a.keep, "ids": N, "by_batch": {}}

    def timed(begin, steps, n_steps, reps=3):
        best = None
        for _ in range(reps):
            check(begin(), "begin")
            t0 = time.perf_counter()
            check(steps(), "steps")
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best / n_steps

    for B in [int(b) for b in a.batches.split(",")]:
        buf = np.ascontiguousarray(rng.integers(0, V, (B, P0)), np.int32)
        lens = np.full(B, P0, np.int32)
        full = np.ascontiguousarray(rng.integers(0, V, (B, W)), np.int32)
        flens = np.full(B, W, np.int32)
        ids = np.empty(B * N, np.int32)
        vp = lambda x: x.ctypes.data_as(C.c_void_p)
        if B == 1:
            kv_begin = lambda: lib.cmp_decode_begin(h, vp(buf), P0, _lib.DECODE_KV, 1.0, 1)
            sl_begin = lambda: lib.cmp_decode_begin_slide(h, vp(buf), P0, a.keep, 1.0, 1)
            full_begin = lambda: lib.cmp_decode_begin_slide(h, vp(full), W, a.keep, 1.0, 1)
            steps = lambda n: lib.cmp_decode_steps(h, n, vp(ids))
        else:
            kv_begin = lambda: lib.cmp_decode_batch_begin(h, vp(buf), vp(lens), B, P0, _lib.DECODE_KV, 1.0, 1)
            sl_begin = lambda: lib.cmp_decode_batch_begin_slide(h, vp(buf), vp(lens), B, P0, a.keep, 1.0, 1)
            full_begin = lambda: lib.cmp_decode_batch_begin_slide(h, vp(full), vp(flens), B, W, a.keep, 1.0, 1)
            steps = lambda n: lib.cmp_decode_batch_steps(h, n, vp(ids))
        check(kv_begin(), "warm-up begin")
        check(steps(32), "warm-up steps")
        kv = timed(kv_begin, lambda: steps(NKV), NKV - 1)
        sl = timed(sl_begin, lambda: steps(N), N - 1)
        rs, fc = m.decode_slide_stats(batched=B > 1)

        def full_begin_and_first_id():
            rc = full_begin()
            return rc if rc else steps(1)              # the prefill's ids: no step runs
        one = timed(full_begin_and_first_id, lambda: steps(1), 1)
        out["by_batch"][str(B)] = {"kv_us_per_step": 1e6 * kv, "slide_us_per_step": 1e6 * sl, "overhead": sl / kv - 1.0,
                                   "one_slide_ms": 1e3 * one, "row_slides": rs, "forward_calls": fc}
    m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
