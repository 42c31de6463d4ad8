"""Observables other than the energy (names and signatures of ferminet/observables.py, which the
reference tree vendors: ``make_s2`` :98-227, ``make_dipole`` :230-272).

``make_s2(signed_network, nspins, assign_spin=True, states=0)`` returns
``s2_estimator(params, data, state=None)``: for every walker of ``data.positions [B, 3N]`` the
spin-squared estimator of the fixed spin assignment,

    S2_L(x) = (na - nb)/2 ((na - nb)/2 + 1) + nb - sum_{i in up} sum_{j in down} psi(x_{i<->j}) / psi(x),

na = max(nspins), nb = min(nspins), x_{i<->j} = x with the coordinates of electron slots i and j
exchanged (the spin labels stay on the slots; i over the up slots ascending in the outer loop, j
over the down slots in the inner one).  psi is complex here, so the result is a COMPLEX tensor
[B] (complex64 for float32 positions) -- the package's convention for complex per-walker
quantities (``local_energy(..., complex_output=True)``); its imaginary part averages to zero.
Nothing is clamped: a walker on a node of psi gives an infinite or NaN value.

``make_dipole(signed_network, states=0)`` returns ``dipole_estimator(params, data, state=None)``
-> [B, 3], mu = sum_a Z_a R_a - sum_i r_i in atomic units (Z_a = ``data.charges`` for a generic
callable, the network's charges -- Z_eff under an ECP -- for an aiqmc network).

If ``signed_network`` is the ``apply`` of an aiqmc ``make_ai_net`` Network (the detection
``Energy.hamiltonian.local_energy`` uses), the estimators run in the HIP kernels of
csrc/observables.hip (``Context.spin_squared`` / ``Context.dipole``): n_up n_down + 1 value
forwards per walker.  Any other callable takes a batched torch path that builds the exchanged
positions and calls it once on the walkers and once on all B n_up n_down exchanged
configurations.  Such a callable follows this package's ``apply`` convention
``signed_network(params, positions [M, 3N], spins, atoms, charges) -> (phase [M], log|psi| [M])``
with the phase an angle in radians; a complex first output is taken as the unit-modulus sign
factor psi / |psi| instead.  Its spin slots come from ``data.spins`` (> 0 up, < 0 down, as
``spin_indices.spin_indices_h``), or are the first nspins[0] slots up when ``data.spins`` is None.

Batch means over several ranks go through ``constants.pmean`` / ``constants.pmean_stats``
(``batch_mean``, ``s2_stats``); no other collective is involved.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import torch

from . import constants


def _positions(data) -> torch.Tensor:
    pos = data.positions
    return pos if isinstance(pos, torch.Tensor) else torch.as_tensor(np.asarray(pos))


def _kernel_dtype(pos: torch.Tensor):
    return pos.dtype if pos.dtype in (torch.float32, torch.float64) else torch.float32


def _spin_slots(spins, nspins: Tuple[int, int], nelectrons: int):
    """(up slots, down slots) of the generic path."""
    if spins is None:
        up, dn = np.arange(nspins[0]), np.arange(nspins[0], nspins[0] + nspins[1])
    else:
        s = spins.detach().cpu().numpy() if isinstance(spins, torch.Tensor) else np.asarray(spins)
        s = np.asarray(s, dtype=np.float64)
        s = s.reshape(-1, s.shape[-1])[0]
        up, dn = np.nonzero(s > 0)[0], np.nonzero(s < 0)[0]
    if len(up) != nspins[0] or len(dn) != nspins[1] or len(up) + len(dn) != nelectrons:
        raise ValueError(f"spin slots ({len(up)} up, {len(dn)} down of {nelectrons} electrons) do not match "
                         f"nspins={tuple(nspins)}")
    return up, dn


def exchanged_positions(pos: torch.Tensor, up: Sequence[int], dn: Sequence[int]) -> torch.Tensor:
    """[B, n_up n_down, 3N]: pos [B, 3N] with the coordinates of slots up[ia] and dn[ib] exchanged,
    pair index ia * n_down + ib."""
    B, n3 = pos.shape
    N = n3 // 3
    perm = np.tile(np.arange(N), (len(up) * len(dn), 1))
    for ia, i in enumerate(up):
        for ib, j in enumerate(dn):
            perm[ia * len(dn) + ib, [i, j]] = [j, i]
    x = pos.reshape(B, N, 3)[:, torch.as_tensor(perm, device=pos.device), :]
    return x.reshape(B, perm.shape[0], n3)


def _s2_diagonal(nspins: Tuple[int, int]) -> float:
    na, nb = max(nspins), min(nspins)
    sz = 0.5 * (na - nb)
    return sz * (sz + 1.0) + nb


def make_s2(signed_network, nspins: Sequence[int], assign_spin: bool = True, states: int = 0):
    """See the module docstring.  The returned estimator also carries
    ``s2_estimator.pair_ratios(params, data)`` -> the complex ratios psi(x_{i<->j}) / psi(x),
    [B, n_up, n_down]."""
    if not assign_spin:
        raise NotImplementedError("make_s2: assign_spin=False (sampled spin configurations) is not built; the "
                                  "network's spin assignment is fixed by its spin tables")
    if states:
        raise NotImplementedError("make_s2: states != 0 (the excited-state machinery) is not built")
    nspins = (int(nspins[0]), int(nspins[1]))
    diag = _s2_diagonal(nspins)
    net = getattr(signed_network, "_aiqmc_network", None)

    if net is not None:
        if tuple(net.nspins) != nspins:
            raise ValueError(f"make_s2: nspins={nspins} differ from the network's {tuple(net.nspins)}")

        def _pairs(params, data):
            pos = _positions(data)
            ctx = net.bind(params, data.atoms, _kernel_dtype(pos))
            return pos, ctx.spin_squared(pos, want_pairs=True)

        def s2_estimator(params, data, state=None):
            del state
            pos = _positions(data)
            ctx = net.bind(params, data.atoms, _kernel_dtype(pos))
            return ctx.spin_squared(pos).reshape(pos.shape[:-1])

        def pair_ratios(params, data):
            pos, (_, dl, dp) = _pairs(params, data)
            r = torch.exp(dl) * torch.complex(torch.cos(dp), torch.sin(dp))
            return r.reshape(*pos.shape[:-1], *nspins)
    else:
        def pair_ratios(params, data):
            pos = _positions(data)
            n3 = pos.shape[-1]
            flat = pos.reshape(-1, n3)
            up, dn = _spin_slots(data.spins, nspins, n3 // 3)
            x = exchanged_positions(flat, up, dn)
            K = x.shape[1]
            s0, l0 = signed_network(params, flat, data.spins, data.atoms, data.charges)
            s1, l1 = signed_network(params, x.reshape(-1, n3), data.spins, data.atoms, data.charges)
            s0, l0, s1, l1 = (torch.as_tensor(t) for t in (s0, l0, s1, l1))
            s1, l1 = s1.reshape(-1, K), l1.reshape(-1, K)
            mag = torch.exp(l1 - l0[:, None])
            if torch.is_complex(s0) or torch.is_complex(s1):
                unit = s1 / s0[:, None]
            else:
                d = s1 - s0[:, None]
                unit = torch.complex(torch.cos(d), torch.sin(d))
            return (mag * unit).reshape(*pos.shape[:-1], *nspins)

        def s2_estimator(params, data, state=None):
            del state
            r = pair_ratios(params, data)
            return diag - r.sum(dim=(-2, -1))

    s2_estimator.pair_ratios = pair_ratios
    return s2_estimator


def make_dipole(signed_network, states: int = 0):
    """See the module docstring."""
    if states:
        raise NotImplementedError("make_dipole: states != 0 (the excited-state machinery) is not built")
    net = getattr(signed_network, "_aiqmc_network", None)

    def dipole_estimator(params, data, state=None):
        del params, state
        pos = _positions(data)
        if net is not None:
            ctx = net.context(data.atoms, _kernel_dtype(pos))
            return ctx.dipole(pos).reshape(*pos.shape[:-1], 3)
        atoms = torch.as_tensor(np.asarray(data.atoms), dtype=pos.dtype, device=pos.device).reshape(-1, 3)
        charges = torch.as_tensor(np.asarray(data.charges), dtype=pos.dtype, device=pos.device).reshape(-1)
        nuc = (charges[:, None] * atoms).sum(0)
        return nuc - pos.reshape(*pos.shape[:-1], -1, 3).sum(-2)

    return dipole_estimator


def batch_mean(values: torch.Tensor) -> torch.Tensor:
    """Mean over the walkers (dim 0) of all ranks: constants.pmean of the rank mean (equal
    per-rank batches, as the drivers require)."""
    return constants.pmean(values.mean(dim=0))


def s2_stats(s2: torch.Tensor):
    """(<S^2>, variance of Re S2_L) over the walkers of all ranks, one all-reduce
    (constants.pmean_stats on the real part)."""
    re = s2.real if torch.is_complex(s2) else s2
    return constants.pmean_stats(re.reshape(-1).contiguous())
