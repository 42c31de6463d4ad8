"""Correlated-sampling estimator: energies of nearby nuclear geometries on the walkers of one run.

The walkers x_b are drawn from |psi_R|^2 at the primary geometry R (``data.atoms``).  For every
secondary geometry R'_m (``new_atoms [M, A, 3]``), with T_m the space warp of
``corrsamples.correlated_samples`` and log|det J| its Jacobian (``jacobianWeights``),

    lw[m][b] = 2 (log|psi_R'm(T_m x_b)| - log|psi_R(x_b)|) + logjac[m][b],   w = exp(lw - max_b lw),
    E_m = sum w e1 / sum w,   E_0 = sum e0 / n,   dE_m = E_m - E_0,   ESS_m = (sum w)^2 / sum w^2,
    err_m = sqrt((sum d^2 - (sum d)^2 / n) / (n (n - 1))),  d_b = (w_b n / sum w)(e1_b - E_m) - (e0_b - E_0)

with e1 = Re E_L at (T_m x_b; R'_m) and e0 = Re E_L at (x_b; R).  The same parameters are used at
every geometry; the statistical noise of E_m and E_0 is correlated and largely cancels in dE_m.
The sums are the three levels of ``_lib.corr_level`` with one all-reduce each between them (MAX,
SUM, SUM over the default process group; none in a single process) and ``_lib.corr_final``.

Departure from the reference's driver (VMC/VMC_energy_correlated_samples.py:160-192): it weights
with |log psi_R(x) - log psi_R'(x)|^2, which is not a probability ratio, evaluates psi_R' at the
un-warped positions, and multiplies by jacobianWeights.weights_jacobian, which is not the
transform's Jacobian.  The estimator above is the standard one those lines aim at.

``network`` is the ``apply`` of an aiqmc ``make_ai_net`` Network (or the Network): the warp, the
wavefunction, the local energies and the levels run in the HIP kernels, one context per geometry
(``AINet.bind(params, atoms_m, dtype)``).  Any other callable
``network(params, positions [K, 3N], spins, atoms, charges) -> (phase [K], log|psi| [K])`` takes the
torch host path throughout; its local energy is ``network.local_energy(params, positions, atoms,
charges) -> [K]`` when the callable has that attribute, and otherwise the all-electron
V - 1/2 (lap log|psi| + |grad log|psi||^2) by automatic differentiation.
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from .. import _lib, constants
from ..utils.utils import np64
from ..wavefunction_Ynlm.nn import as_positions, network_of
from . import corrsamples, jacobianWeights


@dataclasses.dataclass
class EnergyDifferences:
    """Each field [M] (float64): primary energy, secondary energies, differences, their
    delta-method errors and the effective sample sizes of the weights."""
    e0: torch.Tensor
    e: torch.Tensor
    delta: torch.Tensor
    err: torch.Tensor
    ess: torch.Tensor


def _primary_atoms(atoms) -> np.ndarray:
    a = np64(atoms)
    return a.reshape(-1, a.shape[-2], a.shape[-1])[0] if a.ndim == 3 else a


def _all_reduce(x: torch.Tensor, op) -> torch.Tensor:
    if op == dist.ReduceOp.SUM:
        return constants.all_reduce_(x)
    if constants._active():
        dist.all_reduce(x, op=op)
    return x


def reduce_levels(logabs0, e0, logabs1, logjac, e1) -> EnergyDifferences:
    """The three levels and the final step on this rank's walkers (device or host tensors:
    logabs0 / e0 [n], logabs1 / logjac / e1 [M, n]), with the all-reduces between them."""
    L1 = _all_reduce(_lib.corr_level(1, logabs0, e0, logabs1, logjac, e1), dist.ReduceOp.MAX)
    L2 = _all_reduce(_lib.corr_level(2, logabs0, e0, logabs1, logjac, e1, L1=L1), dist.ReduceOp.SUM)
    L3 = _all_reduce(_lib.corr_level(3, logabs0, e0, logabs1, logjac, e1, L1=L1, L2=L2), dist.ReduceOp.SUM)
    res = _lib.corr_final(L2, L3)
    return EnergyDifferences(e0=res[:, 0], e=res[:, 1], delta=res[:, 2], err=res[:, 3], ess=res[:, 4])


def _autograd_local_energy(network, params, pos, spins, atoms, charges):
    """All-electron E_L of a generic callable by double backward, walkers [K, 3N]."""
    x = pos.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        la = torch.as_tensor(network(params, x, spins, atoms, charges)[1])
        (g,) = torch.autograd.grad(la.sum(), x, create_graph=True)
        lap = torch.zeros_like(la)
        for k in range(x.shape[1]):
            lap = lap + torch.autograd.grad(g[:, k].sum(), x, retain_graph=True)[0][:, k]
    g, lap = g.detach(), lap.detach()
    K, N = x.shape[0], x.shape[1] // 3
    p = pos.reshape(K, N, 3)
    r_ae = torch.linalg.norm(p[:, :, None] - atoms[None, None], dim=-1)
    iu = torch.triu_indices(N, N, 1)
    r_ee = torch.linalg.norm(p[:, iu[0]] - p[:, iu[1]], dim=-1)
    A = atoms.shape[0]
    ia = torch.triu_indices(A, A, 1)
    v_nn = (charges[ia[0]] * charges[ia[1]] / torch.linalg.norm(atoms[ia[0]] - atoms[ia[1]], dim=-1)).sum()
    v = (1.0 / r_ee).sum(-1) - (charges[None, None] / r_ae).sum((-2, -1)) + v_nn
    return v - 0.5 * (lap + (g * g).sum(-1))


def energy_differences(network, params, data, new_atoms, *, ecp=None, seed=0, offset=0) -> EnergyDifferences:
    """E(R'_m) - E(R) for the geometries new_atoms [M, A, 3] on the walkers data.positions [B, 3N]
    sampled at data.atoms (see the module docstring).  The local energy is the all-electron one;
    with ``ecp`` (an ``aiqmc.systems.EcpTables`` or any object with its fields) it is the ccECP
    local energy, the same tables attached to every geometry's context and the same Philox
    (seed, offset) passed to every geometry, so that the quadrature rotations are correlated as
    well.  ``seed`` may instead be an ``Energy.pphamiltonian.HostRotations`` (injected rotations,
    the parity mode of the pp local energy)."""
    f = getattr(network, "apply", network)
    net = network_of(f, None)
    atoms = _primary_atoms(data.atoms)
    na = np64(new_atoms)
    if na.ndim == 2:
        na = na[None]
    if na.ndim != 3 or na.shape[1:] != atoms.shape:
        raise ValueError(f"new_atoms must be [M, {atoms.shape[0]}, 3], got {na.shape}")
    M = na.shape[0]
    if M == 0:
        raise ValueError("energy_differences needs at least one secondary geometry")

    if net is None:
        if ecp is not None:
            raise NotImplementedError("energy_differences: the ccECP local energy needs an aiqmc network")
        pos = as_positions(data.positions)
        p = pos.reshape(-1, pos.shape[-1]).to(torch.float64)
        at, nat = torch.as_tensor(atoms).to(p.device), torch.as_tensor(na).to(p.device)
        ch = torch.as_tensor(np64(data.charges)).reshape(-1)[:atoms.shape[0]].to(p.device)
        el = getattr(f, "local_energy", None)
        e_l = (lambda x, a: torch.as_tensor(el(params, x, a, ch))) if el is not None else (
            lambda x, a: _autograd_local_energy(f, params, x, data.spins, a, ch))
        la = lambda x, a: torch.as_tensor(f(params, x, data.spins, a, ch)[1])
        newpos = corrsamples.correlated_samples(at, nat, p)
        logjac = jacobianWeights.log_weights_jacobian(p, at, nat)
        la1 = torch.stack([la(newpos[m], nat[m]) for m in range(M)])
        e1 = torch.stack([e_l(newpos[m], nat[m]) for m in range(M)])
        real = lambda t: (t.real if torch.is_complex(t) else t).to(torch.float64)
        return reduce_levels(real(la(p, at)), real(e_l(p, at)), real(la1), logjac, real(e1))

    ctx0, pos = net.bind_positions(params, data.positions, atoms)
    dtype = ctx0.dtype
    ctxs = [net.bind(params, na[m], dtype) for m in range(M)]
    p = ctx0._pos(pos)
    B = p.shape[0]
    newpos, logjac = ctx0.space_warp(p, na)
    la1 = torch.empty(M, B, dtype=dtype, device=ctx0.device)
    e1 = torch.empty(M, B, dtype=dtype, device=ctx0.device)
    if ecp is None:
        e0, la0, _ = ctx0.local_energy(p, want_logabs=True)
        for m, c in enumerate(ctxs):
            _, la_m, _ = c.local_energy(newpos[m], want_logabs=True, out=e1[m])
            la1[m].copy_(la_m)
    else:
        from ..Energy.pphamiltonian import HostRotations
        tables = tuple(np64(getattr(ecp, k)) for k in _lib.ECP_TABLE_NAMES)
        kw = dict(rot=torch.as_tensor(seed.rot)) if isinstance(seed, HostRotations) else dict(
            seed=int(getattr(seed, "seed", seed)), offset=int(getattr(seed, "offset", offset)))

        def pp(c, x):
            c.ensure_ecp(*tables, list_l=int(ecp.list_l))
            return c.local_energy_ecp(x, **kw).real, c.logpsi(x, with_phase=False)[0]

        e0, la0 = pp(ctx0, p)
        for m, c in enumerate(ctxs):
            e_m, la_m = pp(c, newpos[m])
            e1[m].copy_(e_m)
            la1[m].copy_(la_m)
    return reduce_levels(la0, e0.contiguous(), la1, logjac, e1)


def displaced_geometries(atoms, delta: float) -> np.ndarray:
    """[6A, A, 3]: geometry 2 (3 a + c) moves coordinate c of atom a by +delta, the next one by
    -delta."""
    a = _primary_atoms(atoms)
    out = np.tile(a[None], (6 * a.shape[0], 1, 1))
    for k in range(3 * a.shape[0]):
        out[2 * k, k // 3, k % 3] += delta
        out[2 * k + 1, k // 3, k % 3] -= delta
    return out


def forces_by_differences(network, params, data, *, delta: float = 1e-2, ecp=None, seed=0, offset=0):
    """Central-difference forces from one ``energy_differences`` call over the 6A geometries of
    ``displaced_geometries``: (F [A, 3], err [A, 3]) with F = -(dE_+ - dE_-) / (2 delta) and
    err = sqrt(err_+^2 + err_-^2) / (2 delta).  The two differences share their walkers, so their
    errors are correlated and err is an upper bound of the force's statistical error, not an
    estimate of it.  The finite-difference error is O(delta^2)."""
    a = _primary_atoms(data.atoms)
    res = energy_differences(network, params, data, displaced_geometries(a, delta), ecp=ecp, seed=seed,
                             offset=offset)
    d, e = res.delta.reshape(-1, 3, 2), res.err.reshape(-1, 3, 2)
    force = -(d[..., 0] - d[..., 1]) / (2.0 * delta)
    err = torch.sqrt(e[..., 0] ** 2 + e[..., 1] ** 2) / (2.0 * delta)
    return force, err
