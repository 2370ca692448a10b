#!/usr/bin/env python3
"""Whole train steps with the train options on against the default step, same process, alternating arms:
    python tools/clip_step_bench.py [--cfg c2] [--rounds 3] [--steps 15] [--arms default,clip,accum2,dp1,dp1clip]
default / clip (clip_norm 1.0) / accum2 (accumulate_steps 2: ms per MICRO-step) without a communicator; dp1 / dp1clip under a 1-rank
RCCL communicator, with cmp_dp_stats' exposed_ms (the end-of-step wait: with clipping on the whole-buffer Adam sits in it).
Every arm of every round is a fresh model; per arm the ms/step of each round and their median."""
import json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CFG = {"c2": (512, 8, 6, 1024, 128), "c2b32": (512, 8, 6, 1024, 32), "c4": (768, 12, 12, 2048, 32)}


def run(arm, cfg, steps):
    import torch
    from composer_amd.transformer import Transformer
    E, H, L, T, B = CFG[cfg]
    m = Transformer(390, E, T, L, H, attention_dropout_rate=0.1, residual_dropout_rate=0.1, dtype="bf16", seed=1000, max_batch=B, max_seq=T)
    m.initialize_parameters(0)
    if arm.startswith("dp1"):
        m.init_data_parallel(0, 1, Transformer.new_unique_id())
    if arm.endswith("clip"):
        m.set_train_options(clip_norm=1.0)
    if arm == "accum2":
        m.set_train_options(accumulate_steps=2)
    rng = np.random.default_rng(1234)
    seq = rng.integers(0, 390, size=(2, B, T + 1), dtype=np.int32)
    xs = [torch.from_numpy(np.ascontiguousarray(seq[i, :, :-1])).cuda() for i in range(2)]
    ys = [torch.from_numpy(np.ascontiguousarray(seq[i, :, 1:])).cuda() for i in range(2)]
    for i in range(4):
        m.train_step_device(xs[i % 2].data_ptr(), ys[i % 2].data_ptr(), B, T, 1e-3)
    m.synchronize()
    m.dp_stats(reset=True)
    t0 = time.perf_counter()
    for i in range(steps):
        m.train_step_device(xs[i % 2].data_ptr(), ys[i % 2].data_ptr(), B, T, 1e-3)
    m.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    out = {"ms": ms, "loss": m.last_metrics()[0], "grad_stats": m.grad_stats(), "exposed_ms": m.dp_stats()["exposed_ms"]}
    m.close()
    return out


def main():
    arg = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
    cfg, rounds, steps = arg("--cfg", "c2"), int(arg("--rounds", 3)), int(arg("--steps", 15))
    arms = arg("--arms", "default,clip,accum2,dp1,dp1clip").split(",")
    res = {a: [] for a in arms}
    for r in range(rounds):
        for a in arms:
            res[a].append(run(a, cfg, steps))
    for a in arms:
        print("%s %-8s ms/step %s (median %.3f)  exposed_ms %s  loss %.4f  grad_stats %s" % (
            cfg, a, " ".join("%.3f" % v["ms"] for v in res[a]), float(np.median([v["ms"] for v in res[a]])),
            " ".join("%.3f" % v["exposed_ms"] for v in res[a]), res[a][-1]["loss"], res[a][-1]["grad_stats"]), flush=True)
    print("CLIP_BENCH " + json.dumps(res))


if __name__ == "__main__":
    main()
