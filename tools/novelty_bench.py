"""Times the novelty check (composer_amd/csrc/novelty.hip) on a synthetic corpus: cmp_novelty -- the whole call, host arrays in and
out -- and cmp_k_novelty -- the kernels alone on device pointers --, both between HIP events on the stream the work runs on.

    python tools/novelty_bench.py [--n 33554432] [--L 2048] [--B 1,16] [--N 0,6] [--iters 5] [--warmup 1] [--out FILE]

Prints one JSON line per (B, N): milliseconds (median and spread over the timed calls), cell comparisons per second (cells =
n * L * B * (2 N + 1): the transpositions asked for, not the padded groups the kernel runs) and the share of the VALU bound.

The bound: the inner loop of novelty_match_kernel<1> issues 10 vector instructions per corpus cell, novelty_match_kernel<7> 37 per cell
for 7 transpositions (counted in the gfx950 assembly of this tree's source; scalar instructions and the two or three LDS reads per
cell issue beside them).  A wave64 vector instruction occupies its SIMD for 2 cycles; 256 CUs x 4 SIMDs at 2.4 GHz issue 1.2288e12 of them per
second.  The corpus, 2 bytes per id, is read from HBM once per transposition group and is not the limit.  The corpus is random over
a six-id alphabet plus notes, with one planted copy of the query's first row, so runs are short except one true copy -- the case
the kernel is built for."""
import argparse
import ctypes as C
import json
import statistics
import sys
import os

import numpy as np
import torch                    # before the library is loaded ("Library load order")

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from composer_amd import _lib                              # noqa: E402
from composer_amd.grammar import EventGrammar              # noqa: E402

VALU_PER_SECOND = 256 * 4 * 2.4e9 / 2                      # wave64 vector instructions the chip issues per second
VALU_PER_CELL = {1: 10.0, 7: 37.0}                        # per corpus cell and transposition group, novelty_match_kernel<1> / <7>
KT = 7


def bound_cells_per_second(N):
    """Requested cell comparisons per second at the VALU issue limit."""
    nrank = 2 * N + 1
    if N == 0:
        return VALU_PER_SECOND * 64 / VALU_PER_CELL[1]
    groups = -(-nrank // KT)
    return VALU_PER_SECOND * 64 / (VALU_PER_CELL[7] * groups) * nrank


def make_inputs(n, L, Bmax, seed=0):
    rng = np.random.default_rng(seed)
    g = EventGrammar.from_dataset_params(10, 100, 32, rules=0)
    alphabet = np.asarray([288, 297, 259, 263, 388, 389] + [g.note_on0 + p for p in range(48, 72)] + [g.note_off0 + p for p in range(48, 72)])
    corpus = rng.choice(alphabet, size=n).astype(np.uint16)
    x = rng.choice(alphabet, size=(Bmax, L)).astype(np.int32)
    corpus[n // 3:n // 3 + L] = x[0]                       # one true copy
    return g, corpus, x


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 25)
    ap.add_argument("--L", type=int, default=2048)
    ap.add_argument("--B", default="1,16")
    ap.add_argument("--N", default="0,6")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Bs, Ns = [int(v) for v in a.B.split(",")], [int(v) for v in a.N.split(",")]
    lib = _lib.load()
    _lib.require_gpu()                                     # no device: fail, never a host timing
    g, corpus, x = make_inputs(a.n, a.L, max(Bs))
    layout = g.to_c()
    ctx, h = C.c_void_p(), C.c_void_p()
    _lib.check(lib.cmp_ctx_create(0, C.byref(ctx)), "cmp_ctx_create")
    _lib.check(lib.cmp_dataset_create(ctx, corpus.ctypes.data_as(C.c_void_p), a.n, C.byref(layout), C.byref(h)), "cmp_dataset_create")
    lib.cmp_ctx_stream.restype = C.c_void_p
    ctx_stream = torch.cuda.ExternalStream(lib.cmp_ctx_stream(ctx))
    ids_dev = torch.from_numpy(corpus.view(np.int16)).cuda()
    lines = []
    P = lambda arr: arr.ctypes.data_as(C.c_void_p)
    D = lambda t: C.c_void_p(t.data_ptr())
    for B in Bs:
        xb = np.ascontiguousarray(x[:B])
        lens = np.full(B, a.L, np.int32)
        ln, ps, ks = np.empty((B, a.L), np.int32), np.empty((B, a.L), np.int64), np.empty((B, a.L), np.int32)
        x_dev, lens_dev = torch.from_numpy(xb).cuda(), torch.from_numpy(lens).cuda()
        ln_d = torch.empty((B, a.L), dtype=torch.int32, device="cuda")
        ps_d = torch.empty((B, a.L), dtype=torch.int64, device="cuda")
        ks_d = torch.empty((B, a.L), dtype=torch.int32, device="cuda")
        for N in Ns:
            o = _lib.NoveltyOpts(16, N, 0, 0)

            def whole():
                _lib.check(lib.cmp_novelty(h, P(xb), P(lens), B, a.L, C.byref(o), P(ln), P(ps), P(ks)), "cmp_novelty")

            def kernels():
                s = torch.cuda.current_stream()
                _lib.check(lib.cmp_k_novelty(C.c_void_p(s.cuda_stream), D(ids_dev), a.n, None, C.byref(layout), D(x_dev), D(lens_dev), B, a.L,
                                             C.byref(o), D(ln_d), D(ps_d), D(ks_d)), "cmp_k_novelty")
            ms_whole = timed(ctx_stream, whole, a.iters, a.warmup)
            ms_k = timed(torch.cuda.current_stream(), kernels, a.iters, a.warmup)
            torch.cuda.synchronize()
            assert ln[0, 0] == a.L and ps[0, 0] == a.n // 3 and ks[0, 0] == 0, "the planted copy was not found"
            assert torch.equal(ln_d.cpu(), torch.from_numpy(ln)) and torch.equal(ps_d.cpu(), torch.from_numpy(ps))
            cells = float(a.n) * a.L * B * (2 * N + 1)
            med = statistics.median(ms_k)
            rate = cells / (med * 1e-3)
            line = {"n": a.n, "L": a.L, "B": B, "N": N, "cells": cells,
                    "cmp_novelty_ms_median": statistics.median(ms_whole), "cmp_novelty_ms_min_max": [min(ms_whole), max(ms_whole)],
                    "kernels_ms_median": med, "kernels_ms_min_max": [min(ms_k), max(ms_k)], "cells_per_second": rate,
                    "valu_bound_cells_per_second": bound_cells_per_second(N), "share_of_valu_bound": rate / bound_cells_per_second(N),
                    "reported_positions": int((ln > 0).sum()), "iters": a.iters, "warmup": a.warmup}
            print(json.dumps(line), flush=True)
            lines.append(line)
    lib.cmp_dataset_destroy(h)
    lib.cmp_ctx_destroy(ctx)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
