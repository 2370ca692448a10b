#!/usr/bin/env python3
"""Cost of event-grammar decoding on the per-token chain: `generate` 1024 tokens at temperature 1.0 from a 10-id prompt with the KV
cache and the captured per-token step (the geometry of bench.py's decode figure: 6L/8H/d512, window 2048), grammar off, on (all
rules) and on with a static pitch range; batch 1 and a batch of 8.  Best of three runs each, us per token."""
import sys, os, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from composer_amd.transformer import Transformer
from composer_amd.grammar import EventGrammar

V, E, H, L, W, N = 390, 512, 8, 6, 2048, 1024
m = Transformer(V, E, W, L, H, attention_dropout_rate=0.0, residual_dropout_rate=0.0, dtype="fp32", seed=0, max_batch=1, max_seq=64)
g = EventGrammar.from_dataset_params(10, 100, 32)
prompt = np.random.default_rng(0).integers(0, V, 10)
cases = {"off": {}, "constrained": {"grammar": g}, "constrained_pitch_range": {"grammar": g, "banned_ids": g.pitch_range_bans(48, 84)}}
out = {}
for name, kw in cases.items():
    for B in (1, 8):
        run = (lambda n: m.generate(prompt, n, temperature=1.0, mode="kv", seed=1, **kw)) if B == 1 else \
              (lambda n: m.generate_batch([prompt] * B, n, temperature=1.0, mode="kv", seed=1, **kw))
        run(32)                                                          # warm-up (allocations, graph instantiate)
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            ids = run(N)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        ign = [sum(i >= len(prompt) for i in g.ignored_events(np.concatenate([prompt, r]))) for r in np.atleast_2d(ids)]
        out["%s_b%d" % (name, B)] = {"us_per_token_step": 1e6 * best / N, "ignored_generated_events_per_row": float(np.mean(ign))}
print(json.dumps(out))
