"""Time BlockingAccumulator.update (aiqmc_blocking_update: two launches) and set it against one
VMC iteration.

  python tools/blocking_bench.py [--reps 30] [--bench-json FILE ...] [--out profiles/blocking_bench.json]

Four steps, K = 1 and K = 8 series at 512 and 4,096 chains (float32 samples, 24 levels), each in a
child process of its own under its own time limit (a step that fails or runs out of time ends the
run; nothing is started after it).  A step warms up 64 updates and then times `--reps` windows of
64 consecutive updates: over 64 consecutive sample numbers the cascade completes 2 levels per update
on average whatever the start, so every window does the same work.  Two figures per step:

  stream_us   HIP events around a window / 64: what the stream spends per update while the host
              does nothing else (bounded below by the host's enqueue rate)
  wall_us     a host clock around the same window ending in a synchronise / 64
  enqueue_us  a host clock around the window's update() calls alone: the host time an update costs
              a driver whose GPU is busy with other work

--bench-json: bench.py result lines (files) of the commit to compare with; their
config.walkers_per_gpu selects the matching chain count and ms_per_step is the iteration.  Each
matching step then reports stream_us and enqueue_us as a fraction of that iteration.
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ab-initio-flexible-gaussian-basis-neural-network-quantum-monte-carlo_amd")):
    sys.path.insert(0, p)

STEPS = {"K1_B512": (1, 512), "K8_B512": (8, 512), "K1_B4096": (1, 4096), "K8_B4096": (8, 4096)}
LIMIT = 240      # seconds per child, torch import included
WINDOW = 64
LEVELS = 24


def step(name, reps):
    import torch
    from aiqmc import statistics as blocking
    K, B = STEPS[name]
    x = torch.randn(K, B, device="cuda") - 100.0
    acc = blocking.make_blocking(nseries=K, max_levels=LEVELS, shift=[-100.0] * K)
    for _ in range(WINDOW):
        acc.update(x)
    torch.cuda.synchronize()
    stream_us, wall_us, enqueue_us = [], [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(WINDOW):
            acc.update(x)
        t1 = time.perf_counter()
        b.record()
        b.synchronize()
        t2 = time.perf_counter()
        stream_us.append(1e3 * a.elapsed_time(b) / WINDOW)
        wall_us.append(1e6 * (t2 - t0) / WINDOW)
        enqueue_us.append(1e6 * (t1 - t0) / WINDOW)
    r = acc.result()
    assert acc.count == WINDOW * (reps + 1) and float(r["n_blocks"][0]) == B * acc.count
    med = lambda v: {"median": statistics.median(v), "min": min(v)}
    return {"series": K, "chains": B, "levels": LEVELS, "updates": acc.count, "stream_us": med(stream_us),
            "wall_us": med(wall_us), "enqueue_us": med(enqueue_us), "mean": float(r["mean"][0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--bench-json", nargs="*", default=[], help="bench.py result lines to compare with")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blocking_bench.json"))
    ap.add_argument("--step", choices=sorted(STEPS), help="internal: run one step in this process")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step(a.step, a.reps)))
        return 0
    iteration_ms = {}
    for f in a.bench_json:
        for line in open(f):
            line = line.strip()
            if line.startswith("{") and '"ms_per_step"' in line:
                d = json.loads(line)
                iteration_ms[int(d["config"]["walkers_per_gpu"])] = {
                    "ms_per_step": d["ms_per_step"], "workload": d["config"]["workload"], "dtype": d["dtype"]}
    res = {"dtype": "fp32", "levels": LEVELS, "window": WINDOW, "reps": a.reps, "iteration": iteration_ms, "steps": {}}
    for name in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            print(f"step {name}: no result within {LIMIT} s; stopping", file=sys.stderr)
            return 2
        lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            print(f"step {name} failed ({p.returncode}); stopping\n{p.stdout}\n{p.stderr}", file=sys.stderr)
            return 2
        r = json.loads(lines[-1][7:])
        it = iteration_ms.get(r["chains"])
        if it:
            r["stream_share_of_iteration"] = 1e-3 * r["stream_us"]["median"] / it["ms_per_step"]
            r["enqueue_share_of_iteration"] = 1e-3 * r["enqueue_us"]["median"] / it["ms_per_step"]
        res["steps"][name] = r
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
