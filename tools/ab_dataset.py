#!/usr/bin/env python3
"""Same-box A/B of the pipelined train step fed two ways (the cost of the device dataset, DESIGN.md "Device dataset"):
    python tools/ab_dataset.py <parent build of the library>.so composer_amd/lib/libcomposer_hip.so [--rounds 3] [--steps 30]
arm 0: the first library, host-cut windows through train_step_async (the train loop before the device dataset);
arm 1: the second library, train_step_dataset with transpose 6, stretch 0.2 and random crop all on.
Configuration C2 (6 blocks, 8 heads, E 512, 1024 tokens, B = 128, bf16).  Each arm runs in its own process (the library path is
fixed at import), arms alternate 0 1 0 1 ..., the median ms/step of every arm is printed; arm 1 also times batch_rows_kernel
alone between HIP events (cmp_k_batch_rows on the same plans)."""
import json, os, subprocess, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, H, L, T, B = 512, 8, 6, 1024, 128


def stream_and_layout(n=8 << 20):
    from composer_amd.grammar import EventGrammar
    g = EventGrammar.from_dataset_params(10, 100, 32, rules=0)
    rng = np.random.default_rng(1234)
    ids = rng.integers(0, g.time_shift0, size=n)                      # notes and velocities ...
    sh = rng.random(n) < 0.3                                          # ... and a 30 % share of time shifts
    ids[sh] = g.time_shift0 + rng.integers(0, g.time_shift_n, size=int(sh.sum()))
    return ids.astype(np.uint16), g


def child(arm, steps):
    sys.path.insert(0, ROOT)
    import time, ctypes as C, torch
    from composer_amd import dataset as D
    from composer_amd.transformer import Transformer
    ids, g = stream_and_layout()
    m = Transformer(390, E, T, L, H, attention_dropout_rate=0.1, residual_dropout_rate=0.1, dtype="bf16", seed=1000, max_batch=B, max_seq=T)
    m.initialize_parameters(0)
    out = {}
    if arm == 0:
        wd = D.WindowDataset(ids, B, T, shuffle=True, seed=1)
        it = iter(wd)
        feed = [next(it) for _ in range(steps + 3)]
        submit = lambda i: m.train_step_async(feed[i][0], feed[i][1], 1e-3)
    else:
        dd = D.DeviceDataset(ids, B, T, g, shuffle=True, seed=1, random_crop=True, transpose=6, stretch=0.2)
        feed = [dd.plan(0, i) for i in range(steps + 3)]
        submit = lambda i: m.train_step_dataset(dd, feed[i], 1e-3)
    tickets = [submit(i) for i in range(3)]
    for t in tickets:
        m.step_metrics(t)
    m.synchronize()
    t0 = time.perf_counter()
    tickets = []
    for i in range(3, steps + 3):                                     # the train loop's pipeline: read step s - 1 while s computes
        tickets.append(submit(i))
        if len(tickets) > 1:
            loss = m.step_metrics(tickets.pop(0))[0]
    loss = m.step_metrics(tickets.pop(0))[0]
    m.synchronize()
    out["ms"] = 1e3 * (time.perf_counter() - t0) / steps
    out["loss"] = loss
    if arm == 1:                                                      # the kernel alone, between HIP events on torch's stream
        lib = m._lib
        ids_d = torch.from_numpy(ids.view(np.int16)).cuda()
        x = torch.empty(B, T, dtype=torch.int32, device="cuda"); y = torch.empty_like(x)
        st = torch.empty(B, 2, dtype=torch.int32, device="cuda")
        plans = [torch.from_numpy(p.view(np.int32).copy()).cuda() for p in feed[:8]]
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        lay = g.to_c()
        run = lambda p: lib.cmp_k_batch_rows(s, C.c_void_p(ids_d.data_ptr()), len(ids), C.byref(lay), C.c_void_p(p.data_ptr()), B, T,
                                             C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(st.data_ptr()))
        for p in plans:
            assert run(p) == 0
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 40
        a.record()
        for i in range(reps):
            run(plans[i % 8])
        b.record(); b.synchronize()
        out["kernel_us"] = 1e3 * a.elapsed_time(b) / reps
        out["fallback_rows"] = int((st[:, 1] != 0).sum())
    m.close()
    print("AB_RESULT " + json.dumps(out), flush=True)


def main():
    if sys.argv[1] == "--child":
        return child(int(sys.argv[2]), int(sys.argv[3]))
    libs = [a for a in sys.argv[1:] if a.endswith(".so")]
    assert len(libs) == 2, __doc__
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 3
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 30
    res = {0: [], 1: []}
    for r in range(rounds):
        for i, l in enumerate(libs):
            env = dict(os.environ, COMPOSER_HIP_LIB=os.path.abspath(l))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(i), str(steps)], env=env, capture_output=True,
                               text=True, timeout=300)
            line = [x for x in p.stdout.splitlines() if x.startswith("AB_RESULT ")]
            if not line:
                print("arm %d failed (exit %d):\n%s\n%s" % (i, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
                return 1                                              # nothing more is started after a failed arm
            res[i].append(json.loads(line[0][10:]))
    for i, what in ((0, "train_step_async, host-cut windows"), (1, "train_step_dataset, all augmentations")):
        print("arm %d (%s, %s): %s ms/step, median %.3f, last loss %.4f" % (
            i, os.path.basename(libs[i]), what, " ".join("%.3f" % r["ms"] for r in res[i]), float(np.median([r["ms"] for r in res[i]])),
            res[i][-1]["loss"]))
    print("batch_rows_kernel alone (B=%d, W=%d): %s us, fallback rows in the last batch %d" % (
        B, T, " ".join("%.1f" % r["kernel_us"] for r in res[1]), res[1][-1]["fallback_rows"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
