"""The second-order training step (drop-in for AIQMCrelease3/Optimizer/kfac.py:45-81).

``make_kfac_training_step(damping, optimizer, reset_if_nan=False)`` -> ``step(data, params,
state, key) -> (data, params, state, loss, aux)``, the reference's signature, so that
main/main_pp.py:160-206 ports by building ``aiqmc.Optimizer.sr.Optimizer`` where the reference
builds ``kfac_jax.Optimizer``.

The curvature is NOT KFAC's Kronecker-factored block approximation: ``optimizer`` is the
stochastic-reconfiguration optimizer of Optimizer.sr, whose curvature is the EXACT Fisher matrix
of the wavefunction (the real part of the quantum geometric tensor), damped and inverted as a
whole.  The name of this module and of the factory follow the reference's driver only.

As in the reference the step runs with zero momentum and the damping given here.  With
``reset_if_nan`` a NaN loss returns the parameters and the optimizer state of before the step
(kfac.py:63-78); the optimizer never writes into either, so they are kept by reference instead of
being copied.
"""
from __future__ import annotations

import math

import torch

from ..Loss.loss import check_real_energies


def make_kfac_training_step(damping: float, optimizer, reset_if_nan: bool = False):
    shared_mom = 0.0
    shared_damping = float(damping)

    def step(data, params, state, key):
        """A full update iteration: the optimization step on the walkers of `data`."""
        new_params, new_state, stats = optimizer.step(params=params, state=state, rng=key, batch=data,
                                                      momentum=shared_mom, damping=shared_damping)
        loss = stats["loss"]
        if reset_if_nan and math.isnan(float(loss.real if torch.is_complex(loss) else loss)):
            new_params, new_state = params, state
        check_real_energies(stats["aux"])
        return data, new_params, new_state, loss, stats["aux"]

    return step
