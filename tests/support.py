"""Scaffolding of the test suite, written once: seeded cases, the fp64 oracle's references, contexts,
host draws and rank processes.  A plain module (`import support`): no fixtures, no pytest hooks.

Nothing here has a seed default or a hidden switch: whatever differs between two test files (seed,
randomize_aux, walker count, set_proposal_reuse / set_packed_walkers) is said at the call site."""
import functools
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch


def z_name(n, a):
    """"Z5-4-4" for (13, 3): N split over the A atoms, the remainder on the first ones."""
    zs = [n // a + (1 if k < n % a else 0) for k in range(a)]
    return "Z" + "-".join(str(z) for z in zs)


def skip_unbuilt(shape_or_system):
    """Skip the calling test when the loaded library (a development build) lacks the shape."""
    from aiqmc import _lib
    s = shape_or_system
    shape = tuple(s) if isinstance(s, (tuple, list)) else (s.nelectrons, s.natoms)
    if shape not in _lib.supported_shapes():
        pytest.skip(f"{shape} not in this library's shape list")


def seeded_case(name, seed, B=None, *, randomize_aux=True, width=1.0):
    """(system, params, pos [B, 3N]): one generator of `seed` draws the parameters, then the walkers.
    B = None: four walkers for N <= 10, two above (the oracle's Laplacian)."""
    from oracle import system
    s = system.make_system(name)
    rng = np.random.default_rng(seed)
    params = system.init_params(rng, s, randomize_aux=randomize_aux)
    if B is None:
        B = 4 if s.nelectrons <= 10 else 2
    return s, params, system.init_electrons(rng, s.atoms, s.charges, B, width)


@functools.lru_cache(maxsize=None)
def oracle_case(name, seed, B=None, *, randomize_aux=True, width=1.0, phase=False):
    """seeded_case plus the fp64 oracle's (e_l, logabs, grad) there, computed once per argument set:
    (system, params, pos, e_l, logabs, grad), with phase=True (..., logabs, phase, grad)."""
    from oracle import hamiltonian, network
    s, params, pos = seeded_case(name, seed, B, randomize_aux=randomize_aux, width=width)
    net, pt = network.Network(s), network.to_torch(params)
    e, l, g = hamiltonian.batch_local_energy(net, pt, torch.tensor(pos))
    if not phase:
        return s, params, pos, e.numpy(), l.numpy(), g.numpy()
    ph = np.array([float(net.apply(pt, r)[0]) for r in torch.tensor(pos)])
    return s, params, pos, e.numpy(), l.numpy(), ph, g.numpy()


def make_ctx(system, dtype, params=None, *, ecp=None, atoms=None):
    """A context of `system`: ECP tables when given, then the parameters (a tree or a flat vector)."""
    from oracle import system as osystem
    from aiqmc import _lib
    ctx = _lib.Context.for_system(system, dtype, atoms=atoms)
    if ecp is not None:
        ctx.set_ecp_tables(ecp)
    if params is not None:
        ctx.set_params(osystem.flatten_params(params) if isinstance(params, dict) else params)
    return ctx


def host_draws(seed, B, N, nsweeps=1):
    """(gauss1 [S, B, 3N], gauss2 [S, B, N, 3N], u [S, B, N]) of one generator, in the oracle's layout."""
    rng = np.random.default_rng(seed)
    g1 = torch.tensor(rng.standard_normal((nsweeps, B, 3 * N)))
    g2 = torch.tensor(rng.standard_normal((nsweeps, B, N, 3 * N)))
    u = torch.tensor(rng.uniform(size=(nsweeps, B, N)))
    return g1, g2, u


def oracle_sweep(system, params, pos, draws, tstep):
    """(new positions, acceptance ratios [B, N]) of one fp64 oracle sweep with the draws' first sweep."""
    from oracle import mcstep, network
    g1, g2, u = draws
    x, acc = mcstep.walkers_update(network.Network(system), network.to_torch(params), torch.tensor(pos), g1[0], g2[0],
                                   u[0], tstep)
    return x.numpy(), acc.numpy()


def to_np(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def dev(a, dtype=None):
    return None if a is None else torch.tensor(a, device="cuda", dtype=dtype)


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_ranks(script, world, argv, *, timeout, env=None):
    """Run `script` (program text) as `world` fresh child processes, ranks 0..world-1 of one group on
    127.0.0.1, and return their exit codes.  Every child has `timeout` seconds from the start; at the
    first failure or time-out the remaining children are ended (their codes are the signal's), and
    nothing further is started."""
    port = free_port()
    procs = []
    for r in range(world):
        e = dict(os.environ, **(env or {}), RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r),
                 MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, "-c", script, *argv], env=e))
    deadline = time.monotonic() + timeout
    try:
        while True:
            codes = [p.poll() for p in procs]
            if None not in codes or any(c not in (None, 0) for c in codes) or time.monotonic() > deadline:
                break
            time.sleep(0.02)
    finally:
        for p in procs:
            if p.poll() is None:
                p.terminate()
        for p in procs:
            try:
                p.wait(timeout=10)
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
    return [p.returncode for p in procs]
