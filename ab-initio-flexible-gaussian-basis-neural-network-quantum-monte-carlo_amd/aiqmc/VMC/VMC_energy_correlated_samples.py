"""Correlated-sampling VMC driver (drop-in for AIQMCrelease3/VMC/VMC_energy_correlated_samples.py).

``main(atoms, new_atoms, charges, spins, tstep, nelectrons, nsteps, natoms, ndim, batch_size,
iterations, list_l, nspins, save_path, restore_path, Rn_local, Local_coes, Local_exps,
Rn_non_local, Non_local_coes, Non_local_exps, save_frequency, structure)`` with the reference's
flow (:28-192): restore the VMC checkpoint (a run without one raises, :72-73), one ``mc_step`` call
of ``nsteps`` sweeps at the primary geometry (:140), then the ccECP energies of the geometries
``new_atoms [M, A, 3]`` on those walkers.  The energies come from
``correlatedsamples.estimator.energy_differences`` -- the space warp with its Jacobian and the
probability-ratio weights -- and not from the reference's unfinished weights (:160-185, see the
estimator's docstring); the result object (e0, e, delta, err, ess, each [M]) is logged and returned.

One process per GPU (torchrun); ``batch_size`` is the global walker count, each rank owns
batch_size / world walkers and the estimator's three all-reduces pool them.  Every rank evaluates
all M geometries (the reference spreads them over its devices, :76-81, which its pmap shapes tie
to M = the device count).  ``iterations``, ``save_path`` beyond the checkpoint search,
``save_frequency`` and ``structure`` are accepted and unused, as in the reference.
"""
from __future__ import annotations

import logging
import time
from typing import Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist

from .. import checkpoint
from ..correlatedsamples import estimator
from ..spin_indices import jastrow_indices_ee, spin_indices_h
from ..systems import EcpTables
from ..wavefunction_Ynlm import nn
from . import VMCmcstep


def main(atoms, new_atoms, charges, spins, tstep: float, nelectrons: int, nsteps: int, natoms: int, ndim: int,
         batch_size: int, iterations: int, list_l: int, nspins: Tuple[int, int], save_path: Optional[str],
         restore_path: Optional[str], Rn_local, Local_coes, Local_exps, Rn_non_local, Non_local_coes,
         Non_local_exps, save_frequency: float, structure=None, seed: Optional[int] = None):
    del iterations, save_frequency, structure
    logging.info('Quantum Monte Carlo Start running')
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank() if world > 1 else 0
    if batch_size % world:
        raise ValueError('Batch size must be divisible by number of devices!')
    device_batch_size = batch_size // world
    seed = int(1e6 * time.time()) % (1 << 62) if seed is None else int(seed)
    ckpt_save_path = checkpoint.create_save_path(save_path=save_path)
    ckpt_restore_path = checkpoint.get_restore_path(restore_path=restore_path)
    fname = checkpoint.find_last_checkpoint(ckpt_save_path) or checkpoint.find_last_checkpoint(ckpt_restore_path)
    if not fname:
        raise ValueError('correlated samples VMC must use the wave function from VMC!')
    _, data, params, _ = checkpoint.restore(fname, batch_size)

    new_atoms = np.asarray(new_atoms.detach().cpu() if isinstance(new_atoms, torch.Tensor) else new_atoms,
                           dtype=np.float64).reshape(-1, natoms, ndim)
    logging.info('number_structures: %d', new_atoms.shape[0])
    par, anti, npar, nanti = jastrow_indices_ee(spins=spins, nelectrons=nelectrons)
    up, dn = spin_indices_h(spins)
    network = nn.make_ai_net(ndim=ndim, nelectrons=nelectrons, natoms=natoms, nspins=nspins, determinants=1,
                             charges=charges, parallel_indices=par, antiparallel_indices=anti, n_parallel=npar,
                             n_antiparallel=nanti, spin_up_indices=up, spin_down_indices=dn)
    signed_network = network.apply
    mc_step = VMCmcstep.main_monte_carlo(f=signed_network, tstep=tstep, ndim=ndim, nelectrons=nelectrons,
                                         nsteps=nsteps, batch_size=device_batch_size)
    dev = torch.device("cuda", torch.cuda.current_device())
    pos = torch.as_tensor(np.asarray(data.positions)).reshape(-1, nelectrons * ndim)
    if pos.shape[0] == batch_size and world > 1:
        pos = pos[rank * device_batch_size:(rank + 1) * device_batch_size]
    if pos.shape[0] != device_batch_size:
        raise ValueError(f"checkpoint holds {pos.shape[0]} walkers, expected {device_batch_size} per device")
    dtype = nn.kernel_dtype(pos)
    data = nn.AINetData(positions=pos.to(dev, dtype).contiguous(), spins=spins, atoms=atoms, charges=charges)
    key = VMCmcstep.PhiloxKey(seed + 7919 * rank, 0)
    data = mc_step(params, data, key)
    logging.info("calculate the new positions and the new energy for the new configurations.")
    ecp = EcpTables(Rn_local, Local_coes, Local_exps, Rn_non_local, Non_local_coes, Non_local_exps, int(list_l))
    # the rotations of the pp quadrature: one (seed, offset) for every geometry, beyond the sweeps' draws
    res = estimator.energy_differences(signed_network, params, data, new_atoms, ecp=ecp, seed=key.seed,
                                       offset=nsteps)
    for m in range(new_atoms.shape[0]):
        logging.info('structure %d: E = %.6f, E - E0 = %.6f +- %.6f (E0 = %.6f, ESS = %.1f of %d)', m,
                     float(res.e[m]), float(res.delta[m]), float(res.err[m]), float(res.e0[m]), float(res.ess[m]),
                     batch_size)
    return res
