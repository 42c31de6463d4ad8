"""Measurements of the stochastic-reconfiguration optimizer (aiqmc.Optimizer.sr); bench.py measures
the flagship Metropolis workload and does not cover it.  One JSON document on stdout (--out FILE
also writes it):

* gram: the aiqmc_sr_gram launch on the real per-walker Jacobians (log|psi| and phase) of N2 and Be,
  fp32, 4096 walkers, against torch.matmul of the same centred fp32 product (the centred copies
  made outside the timed region).  HIP events around each launch after warm-up, the median over
  the repeats.
* step: one training iteration (mc_step of 10 sweeps + optimizer step) with SR and with Adam
  (Optimizer.adam) on Be and N2, 4096 walkers; the median wall time of synchronised iterations.
* trace: the energy of Be every 5th of --trace-steps iterations with SR and with Adam from the
  same parameters, walkers and Metropolis keys.  The reference's schedule 0.05 (1 / (1 + t))^10000
  (used for the timings) is zero after the first step, so the trace runs both optimizers with
  0.02 / (1 + t / 100) instead.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ab-initio-flexible-gaussian-basis-neural-network-quantum-monte-carlo_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)


def event_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": repeats}


def setup(name, walkers, dtype, seed):
    from aiqmc import systems
    from aiqmc.Energy import hamiltonian as H
    from aiqmc.Loss import loss as L
    from aiqmc.VMC import VMCmcstep
    from aiqmc.wavefunction_Ynlm import nn
    from aiqmc.initial_electrons_positions.init import init_electrons
    s = systems.make_system(name)
    network = s.make_network()
    params = network.init(seed)
    pos, sp = init_electrons(seed + 3, None, s.atoms, s.charges, s.spins, walkers, 1.0)
    data = nn.AINetData(positions=pos.to("cuda", dtype).contiguous(), spins=sp, atoms=s.atoms, charges=s.charges)
    mc_step = VMCmcstep.main_monte_carlo(f=network.apply, tstep=0.05, ndim=3, nelectrons=s.nelectrons, nsteps=10,
                                         batch_size=walkers)
    le = H.local_energy(f=network.apply, charges=s.charges, nspins=s.spins)
    ev = L.make_loss(network=network.apply, local_energy=le, clip_local_energy=5.0, clip_from_median=False,
                     center_at_clipped_energy=True, complex_output=True)
    return s, network, params, data, mc_step, ev


def schedule(t, rate=0.05, delay=1.0, decay=10000):
    return rate * (1.0 / (1.0 + (t / delay))) ** decay


def trace_schedule(t):
    return 0.02 / (1.0 + t / 100.0)


def make_steps(ev, schedule=schedule):
    from aiqmc.Optimizer import adam, kfac, sr, optax_like as optax
    opt = sr.Optimizer(ev, l2_reg=0.0, norm_constraint=0.001, learning_rate_schedule=schedule, curvature_ema=0.95,
                       inverse_update_period=1, min_damping=1.0e-4)
    sr_step = kfac.make_kfac_training_step(damping=0.001, optimizer=opt)
    ad = optax.chain(optax.scale_by_adam(b1=0.9, b2=0.999, eps=1e-8, eps_root=0.0),
                     optax.scale_by_schedule(schedule), optax.scale(-1.))
    adam_step = adam.make_training_step(adam.make_opt_update_step(ev, ad))
    return opt, sr_step, adam_step


def gram_bench(name, walkers, warmup, repeats):
    from aiqmc import _lib
    s, network, params, data, mc_step, ev = setup(name, walkers, torch.float32, 2)
    from aiqmc.VMC import VMCmcstep
    data = mc_step(params, data, VMCmcstep.PhiloxKey(9, 0))
    ctx = network.apply._aiqmc_network.bind(params, s.atoms, torch.float32)
    x = data.positions.reshape(walkers, -1)
    o_re, o_im = ctx.logpsi_param_grad(x), ctx.phase_param_grad(x)
    P = o_re.shape[1]
    c_re, c_im = o_re.mean(dim=0), o_im.mean(dim=0)
    out = torch.empty(P * P + 2 * P + 1, dtype=torch.float64, device="cuda")
    a, b = (o_re - c_re).contiguous(), (o_im - c_im).contiguous()
    g32 = torch.empty(P, P, dtype=torch.float32, device="cuda")
    res = {"system": name, "walkers": walkers, "P": P,
           "flop_full": 2.0 * 2 * walkers * P * P, "flop_upper": 2.0 * 2 * walkers * P * (P + 1) / 2}
    res["sr_gram"] = event_ms(lambda: _lib.sr_gram(o_re, o_im, c_re, c_im, out=out), warmup, repeats)

    def mm():
        torch.matmul(a.T, a, out=g32)
        g32.addmm_(b.T, b)
    res["torch_matmul_fp32"] = event_ms(mm, warmup, repeats)
    res["sr_gram_real_only"] = event_ms(lambda: _lib.sr_gram(o_re, None, c_re, None, out=out), warmup, repeats)
    res["ratio_sr_gram_over_matmul"] = res["sr_gram"]["median_ms"] / res["torch_matmul_fp32"]["median_ms"]
    res["sr_gram_tflops_upper"] = res["flop_upper"] / (res["sr_gram"]["median_ms"] * 1e-3) / 1e12
    _lib.sr_gram(o_re, o_im, c_re, c_im, out=out)
    mm()
    G = out[:P * P].reshape(P, P)
    res["max_abs_diff_vs_matmul_over_max"] = float((G - g32.double()).abs().max() / G.abs().max())
    return res


def step_bench(name, walkers, warmup, repeats):
    from aiqmc.VMC import VMCmcstep
    out = {"system": name, "walkers": walkers}
    for which in ("sr", "adam"):
        s, network, params, data, mc_step, ev = setup(name, walkers, torch.float32, 2)
        opt, sr_step, adam_step = make_steps(ev)
        state = opt.init(params, None, data) if which == "sr" else None
        step = sr_step if which == "sr" else adam_step
        ms, ms_opt = [], []
        for t in range(warmup + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            data = mc_step(params, data, VMCmcstep.PhiloxKey(9, 10 * t))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            data, params, state, loss, aux = step(data, params, state, VMCmcstep.PhiloxKey(23, t))
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if t >= warmup:
                ms.append(1e3 * (t2 - t0))
                ms_opt.append(1e3 * (t2 - t1))
        out[which] = {"iteration_median_ms": statistics.median(ms), "optimizer_step_median_ms": statistics.median(ms_opt),
                      "repeats": repeats, "energy": float(loss.real)}
    out["sr_over_adam_iteration"] = out["sr"]["iteration_median_ms"] / out["adam"]["iteration_median_ms"]
    return out


def trace(name, walkers, steps):
    from aiqmc.VMC import VMCmcstep
    out = {"system": name, "walkers": walkers, "steps": steps}
    for which in ("sr", "adam"):
        s, network, params, data, mc_step, ev = setup(name, walkers, torch.float32, 2)
        opt, sr_step, adam_step = make_steps(ev, trace_schedule)
        state = opt.init(params, None, data) if which == "sr" else None
        step = sr_step if which == "sr" else adam_step
        for t in range(10):   # equilibrate the walkers in the initial wavefunction
            data = mc_step(params, data, VMCmcstep.PhiloxKey(7, 10 * t))
        es = []
        for t in range(steps):
            data = mc_step(params, data, VMCmcstep.PhiloxKey(9, 10 * t))
            data, params, state, loss, aux = step(data, params, state, VMCmcstep.PhiloxKey(23, t))
            es.append(float(loss.real))
        out[which] = es[::5]
        out[which + "_mean_last_20"] = float(np.mean(es[-20:]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--trace-steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0),
           "gram": [gram_bench(n, a.walkers, a.warmup, a.repeats) for n in ("N2", "Be")],
           "step": [step_bench(n, a.walkers, a.warmup, a.repeats) for n in ("Be", "N2")],
           "trace": trace("Be", a.walkers, a.trace_steps)}
    text = json.dumps(res)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
