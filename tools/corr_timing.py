"""Time the space-warp launch and one energy_differences call (N2, fp32, HIP events).

  python tools/corr_timing.py [--walkers 4096] [--geometries 12] [--launches 30]

Warp: the raw aiqmc_space_warp launch on preallocated buffers, 5 warm-up launches, then the median
of `--launches` single launches between two events, next to the bytes it moves (B 3N read,
M B (3N + 1) written, of the context dtype) and the bandwidth that implies.  Estimator: one
energy_differences call (warp, M + 1 local-energy batches with log|psi|, three levels, final)
against M + 1 bare local_energy batches on the same walkers, and the three levels plus the final
step alone; medians of 7 after 2 warm-ups.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ab-initio-flexible-gaussian-basis-neural-network-quantum-monte-carlo_amd")):
    sys.path.insert(0, p)

import numpy as np
import torch


def _timed(fn, warm, reps):
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
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--geometries", type=int, default=12)
    ap.add_argument("--launches", type=int, default=30)
    a = ap.parse_args()
    from aiqmc import _lib, systems
    from aiqmc.correlatedsamples import estimator
    from aiqmc.wavefunction_Ynlm import nn
    s = systems.make_system("N2")
    net = s.make_network()
    params = net.init(5)
    rng = np.random.default_rng(11)
    B, M, N = a.walkers, a.geometries, s.nelectrons
    block = np.concatenate([np.tile(s.atoms[i], int(s.charges[i])) for i in range(s.natoms)])
    pos = torch.tensor(block[None] + rng.standard_normal((B, 3 * N)), dtype=torch.float32, device="cuda")
    new = s.atoms[None] + rng.uniform(-0.05, 0.05, size=(M, s.natoms, 3))
    ain = net.apply._aiqmc_network
    ctx = ain.bind(params, s.atoms, torch.float32)
    ctx.mc_step(pos, 20, 0.02, seed=1)
    na = torch.tensor(new, device="cuda")
    newpos = torch.empty(M, B, 3 * N, dtype=torch.float32, device="cuda")
    logjac = torch.empty(M, B, dtype=torch.float32, device="cuda")
    st = _lib._stream(ctx.device)
    warp = lambda: _lib.check(ctx._lib.aiqmc_space_warp(ctx._h, _lib._ptr(pos), B, _lib._ptr(na), M, _lib._ptr(newpos),
                                                        _lib._ptr(logjac), st), "aiqmc_space_warp")
    t_warp = _timed(warp, 5, a.launches)
    nbytes = 4 * (B * 3 * N + M * B * (3 * N + 1))
    data = nn.AINetData(positions=pos, spins=s.spins, atoms=s.atoms, charges=s.charges)
    t_call = _timed(lambda: estimator.energy_differences(net.apply, params, data, new), 2, 7)
    ctxs = [ctx] + [ain.bind(params, new[m], torch.float32) for m in range(M)]
    xs = [pos] + [newpos[m] for m in range(M)]
    t_el = _timed(lambda: [c.local_energy(x) for c, x in zip(ctxs, xs)], 2, 7)
    e0, la0, _ = ctx.local_energy(pos, want_logabs=True)
    la1, e1 = la0[None].repeat(M, 1), e0[None].repeat(M, 1)
    t_lv = _timed(lambda: estimator.reduce_levels(la0, e0, la1, logjac, e1), 2, 7)
    print(json.dumps({"system": "N2", "dtype": "fp32", "walkers": B, "geometries": M,
                      "warp_ms_median": t_warp, "warp_bytes": nbytes, "warp_GBps": nbytes / t_warp / 1e6,
                      "energy_differences_ms": t_call, "local_energy_batches_ms": t_el, "levels_ms": t_lv,
                      "warp_plus_levels_fraction": (t_warp + t_lv) / t_call}))


if __name__ == "__main__":
    main()
