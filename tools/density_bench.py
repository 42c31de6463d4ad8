"""Time one aiqmc_density_accumulate call next to one mc_step sweep (N2, fp32, HIP events).

  python tools/density_bench.py [--walkers 4096] [--launches 50] [--out profiles/density_bench.json]

Configuration: a 64^3 grid on [-6, 6)^3, 256 radial bins over [0, 8) and 256 pair bins over [0, 8).
Three steps, each in a child process of its own under its own time limit (a step that fails or
runs out of time ends the run; nothing is started after it):

  privatised  the call as configured: radial + pair are 1,799 words, the LDS path
  fallback    the same call with the radial family stretched to 1,280 bins over [0, 40): the same
              bin width exactly (inv_h = 32), 5,895 small words > AIQMC_DENSITY_LDS_WORDS, so radial
              and pair take global atomics.  Samples beyond 8 bohr land in the extra bins instead
              of the outside word, which if anything spreads the fallback's updates more thinly.
  sweep       one mc_step sweep (Philox draws) of the same walkers

Each step equilibrates the same seeded walkers with 20 sweeps, warms up 5 launches and reports the
median and the minimum of `--launches` single launches between two events.  The two density steps
also print a digest of the words both configurations share (total, grid, pair, the first 256
radial bins) after ONE call on the same walkers; the parent requires the digests to be equal.
Prints one JSON line and writes it to --out.
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ab-initio-flexible-gaussian-basis-neural-network-quantum-monte-carlo_amd")):
    sys.path.insert(0, p)

GRID = ((-6.0, -6.0, -6.0), (6.0, 6.0, 6.0), (64, 64, 64))
RAD = (8.0, 256)
PAIR = (8.0, 256)
STRETCH = 5
LIMITS = {"privatised": 240, "fallback": 240, "sweep": 300}   # seconds per child, torch import included


def _timed(fn, warm, reps):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out)


def step(name, walkers, launches):
    import numpy as np
    import torch
    from aiqmc import _lib, systems
    s = systems.make_system("N2")
    net = s.make_network()
    ctx = net.apply._aiqmc_network.bind(net.init(5), s.atoms, torch.float32)
    N = s.nelectrons
    block = np.concatenate([np.tile(s.atoms[i], int(s.charges[i])) for i in range(s.natoms)])
    pos = torch.tensor(block[None] + np.random.default_rng(11).standard_normal((walkers, 3 * N)), dtype=torch.float32,
                       device="cuda")
    ctx.mc_step(pos, 20, 0.02, seed=1)
    torch.cuda.synchronize()
    if name == "sweep":
        k = [2]

        def sweep():
            ctx.mc_step(pos, 1, 0.02, seed=k[0])
            k[0] += 1
        med, lo = _timed(sweep, 5, launches)
        return {"ms_median": med, "ms_min": lo}
    rad = RAD if name == "privatised" else (RAD[0] * STRETCH, RAD[1] * STRETCH)
    cfg = _lib.density_cfg(grid=GRID, radial=rad, pair=PAIR)
    lay = ctx.density_layout(cfg)
    assert lay["privatised"] == (name == "privatised"), lay
    acc = torch.zeros(lay["n_words"], dtype=torch.int64, device="cuda")
    ctx.density_accumulate(pos, acc, cfg)
    torch.cuda.synchronize()
    w = acc.cpu().numpy()
    o, z = lay["offsets"], lay["sizes"]
    shared = [w[o[k]:o[k] + z[k]] for k in ("total", "skipped", "grid", "grid_out", "pair", "pair_out")]
    shared.append(np.ascontiguousarray(w[o["radial"]:o["radial"] + z["radial"]].reshape(2, 2, -1)[:, :, :RAD[1]]))
    digest = hashlib.sha256(b"".join(a.tobytes() for a in shared)).hexdigest()[:16]
    st = _lib._stream(ctx.device)
    call = lambda: _lib.check(ctx._lib.aiqmc_density_accumulate(ctx._h, ctypes.byref(cfg), _lib._ptr(pos), walkers, None,
                                                                _lib._ptr(acc), st), "aiqmc_density_accumulate")
    med, lo = _timed(call, 5, launches)
    small = lay["n_words"] - o["radial"]
    return {"ms_median": med, "ms_min": lo, "privatised": lay["privatised"], "small_words": small,
            "n_words": lay["n_words"], "shared_words_sha16": digest,
            "nonzero_small_words": int((w[o["radial"]:] != 0).sum()),
            "updates_per_call": {"grid": walkers * N, "radial": walkers * N * s.natoms,
                                 "pair": walkers * N * (N - 1) // 2}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_bench.json"))
    ap.add_argument("--step", choices=sorted(LIMITS), help="internal: run one step in this process")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step(a.step, a.walkers, a.launches)))
        return 0
    res = {"system": "N2", "dtype": "fp32", "walkers": a.walkers, "launches": a.launches,
           "config": {"grid": GRID, "radial": RAD, "pair": PAIR, "fallback_radial": (RAD[0] * STRETCH, RAD[1] * STRETCH)}}
    for name in ("privatised", "fallback", "sweep"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--walkers", str(a.walkers), "--launches",
               str(a.launches)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[name])
        except subprocess.TimeoutExpired:
            print(f"step {name}: no result within {LIMITS[name]} s; stopping", file=sys.stderr)
            return 2
        lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            print(f"step {name} failed ({p.returncode}); stopping\n{p.stdout}\n{p.stderr}", file=sys.stderr)
            return 2
        res[name] = json.loads(lines[-1][7:])
    res["words_equal"] = res["privatised"]["shared_words_sha16"] == res["fallback"]["shared_words_sha16"]
    res["privatised_over_fallback"] = res["privatised"]["ms_median"] / res["fallback"]["ms_median"]
    res["privatised_share_of_sweep"] = res["privatised"]["ms_median"] / res["sweep"]["ms_median"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if res["words_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
