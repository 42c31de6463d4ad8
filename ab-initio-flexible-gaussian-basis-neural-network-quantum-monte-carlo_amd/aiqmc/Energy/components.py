"""What the local energy is made of: kinetic, electron-electron, electron-nucleus, nucleus-nucleus
and pseudopotential terms per walker (aiqmc_energy_components, csrc/components.hip).

    comps = components.make_energy_components(net.apply, charges, nspins)        # all-electron
    comps = components.make_energy_components(net.apply, charges, nspins, rn_local=..., ...,
                                              list_l=2)                          # pseudopotential
    acc = statistics.make_blocking(nseries=8, names=components.COMPONENT_NAMES)
    for it in range(iterations):
        ...                                        # sweeps
        acc.update(comps(params, key, data))       # [8, B], one blocking sample
    s = components.summarize(acc)
    print(s["kinetic"], s["virial_ratio"], s["kinetic_gap"])

Rows (COMPONENT_NAMES, the AIQMC_COMP_* macros of include/aiqmc.h):
  total          Re E_L, the bits of hamiltonian.local_energy / pphamiltonian.local_energy
  kinetic        T_L = all-electron E_L - (v_ee + v_en + v_nn) = -1/2 (lap log|psi| + |grad log|psi||^2),
                 with complex_output plus 1/2 |grad theta|^2
  kinetic_grad   T_G = 1/2 |grad log|psi||^2.  <T_G> = <T_L> over |psi|^2 for a wavefunction of
                 piecewise-constant phase; ``summarize`` reports the gap <T_L - T_G>, the standard
                 check that the sample is equilibrated and the Laplacian right
  v_ee, v_en, v_nn, v_pp_local   the potentials of ``potential_terms``
  v_pp_nonlocal  total - (kinetic + v_ee + v_en + v_nn + v_pp_local); 0 without an ECP
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import numpy as np
import torch

from .. import statistics
from .._lib import COMPONENT_NAMES, ECP_TABLE_NAMES
from ..VMC.VMCmcstep import PhiloxKey, philox_key
from ..utils.utils import np64
from ..wavefunction_Ynlm.nn import as_positions, network_of
from .pphamiltonian import HostRotations

__all__ = ["COMPONENT_NAMES", "make_energy_components", "potential_terms", "summarize"]

_POTENTIAL = ("v_ee", "v_en", "v_nn", "v_pp_local", "v_pp_nonlocal")


def make_energy_components(f, charges, nspins: Sequence[int], complex_output: bool = False, **pp_tables):
    """``components(params, key, data) -> [8, B]`` for an aiqmc network ``f`` (the signature and the
    charge check of hamiltonian.local_energy).  The pseudopotential keywords are those of
    pphamiltonian.local_energy (rn_local, local_coes, local_exps, rn_non_local, non_local_coes,
    non_local_exps, list_l; natoms / nelectrons / ndim / lognetwork / use_scan are accepted): give
    all seven or none.  With them ``key`` selects the grid rotations as there -- a
    ``HostRotations``, a ``PhiloxKey`` or an int seed; without, it is ignored."""
    del nspins
    net = network_of(f, "make_energy_components")
    c = np64(charges)
    if c.shape != net.charges.shape or not np.allclose(c, net.charges):
        raise ValueError("make_energy_components charges differ from the network's charges")
    for k, want in (("natoms", net.natoms), ("nelectrons", net.nelectrons), ("ndim", 3)):
        if k in pp_tables and int(pp_tables.pop(k)) != want:
            raise ValueError(f"{k} does not match the network")
    pp_tables.pop("lognetwork", None)
    pp_tables.pop("use_scan", None)
    unknown = set(pp_tables) - set(ECP_TABLE_NAMES) - {"list_l"}
    if unknown:
        raise TypeError(f"make_energy_components: unknown keyword(s) {sorted(unknown)}")
    tables = None
    if pp_tables:
        missing = [k for k in ECP_TABLE_NAMES + ("list_l",) if k not in pp_tables]
        if missing:
            raise ValueError(f"make_energy_components: pseudopotential tables need {missing} as well")
        list_l = int(pp_tables["list_l"])
        tables = tuple(np64(pp_tables[k]) for k in ECP_TABLE_NAMES)
        if tables[3].reshape(net.natoms, -1).shape[1] % (list_l + 1):
            raise ValueError("non-local tables must have list_l + 1 angular channels per atom")

    def components(params, key: Union[int, PhiloxKey, HostRotations, None], data) -> torch.Tensor:
        ctx, pos = net.bind_positions(params, data.positions, data.atoms)
        if tables is None:
            if ctx.ecp is not None:
                raise ValueError("this network's context carries pseudopotential tables: pass them to "
                                 "make_energy_components")
            return ctx.energy_components(pos, complex_output=complex_output)
        ctx.ensure_ecp(*tables, list_l=list_l)
        if isinstance(key, HostRotations):
            return ctx.energy_components(pos, complex_output=complex_output, rot=torch.as_tensor(key.rot))
        k = philox_key(key or 0)
        return ctx.energy_components(pos, complex_output=complex_output, seed=k.seed, offset=k.offset)

    components._aiqmc_network = net
    return components


def potential_terms(pos, atoms, charges, ecp_local=None) -> torch.Tensor:
    """Rows v_ee, v_en, v_nn, v_pp_local ([4, B]) of positions ``pos`` [..., 3N] with the kernel's
    formulas in plain torch, in the dtype of ``pos`` (the documented replica of
    k_energy_components; works on any device, sums in torch's order rather than the kernel's):
      r = sqrt(dx^2 + dy^2 + dz^2);  v_ee = sum_{i<j} 1 / r_ij;  v_en = sum_{i,a} -Z_a / r_ia;
      v_nn = sum_{a<b} Z_a Z_b / R_ab in float64, rounded to the dtype once;
      v_pp_local = sum_{i,a,k} c_ak r^(n_ak - 2) exp(-alpha_ak r^2), r^2 the sum of squares.
    ``ecp_local`` = (rn_local, local_coes, local_exps), each [A, KL]; None: v_pp_local = 0.
    Nothing is clamped: coincident particles give inf."""
    x = as_positions(pos)
    dt, dev = x.dtype, x.device
    a64 = torch.as_tensor(np64(atoms)).reshape(-1, 3)
    z64 = torch.as_tensor(np64(charges)).reshape(-1)
    A = a64.shape[0]
    x = x.reshape(-1, x.shape[-1] // 3, 3)
    N = x.shape[1]
    d = x[:, None, :, :] - x[:, :, None, :]
    iu = torch.triu_indices(N, N, 1, device=dev)
    r_ee = torch.sqrt((d * d).sum(-1))[:, iu[0], iu[1]]
    v_ee = (1.0 / r_ee).sum(-1)
    dae = x[:, :, None, :] - a64.to(dev, dt)[None, None]
    r2 = (dae * dae).sum(-1)                                   # [B, N, A]
    r = torch.sqrt(r2)
    v_en = (-z64.to(dev, dt)[None, None] / r).sum((-2, -1))
    vnn = 0.0
    for i in range(A):
        for j in range(i + 1, A):
            vnn += float(z64[i] * z64[j] / torch.sqrt(((a64[i] - a64[j]) ** 2).sum()))
    v_nn = torch.full_like(v_ee, vnn)
    if ecp_local is None:
        v_pp = torch.zeros_like(v_ee)
    else:
        rn, co, ex = (torch.as_tensor(np64(t)).reshape(A, -1) for t in ecp_local)
        n2 = (rn - 2.0).to(dev, dt)
        v_pp = (co.to(dev, dt) * r[..., None] ** n2 * torch.exp(-ex.to(dev, dt) * r2[..., None])).sum((-3, -2, -1))
    return torch.stack([v_ee, v_en, v_nn, v_pp])


def _column(acc: statistics.BlockingAccumulator, k: int) -> dict:
    r = acc.result(k)
    lvl = r["optimal_level"]
    err = r["stderr_opt"]
    if lvl is None and r["naive_stderr"] == 0.0:   # a constant row (v_nn; the ECP rows without an ECP)
        lvl, err = 0, 0.0
    return {"mean": float(r["mean"][0]), "stderr": err, "level": lvl}


def summarize(acc: statistics.BlockingAccumulator) -> dict:
    """The blocked summary of a ``statistics.make_blocking(nseries=8)`` accumulator fed with
    ``components(...)`` samples.  Per row name: ``{"mean", "stderr", "level"}`` -- the level-0 mean
    and the standard error at the row's optimal blocking level (``BlockingAccumulator.result``;
    NaN / None while no level qualifies; 0 for a constant row).  Also
      ``virial_ratio``  -(v_ee + v_en + v_nn + v_pp_local + v_pp_nonlocal) / kinetic of the means,
      ``kinetic_gap``   <T_L - T_G>,
    each ``{"value", "stderr", "level"}`` with the delta-method error sqrt(g^T C g / n) from the
    accumulator's ``covariance(level)`` (g the gradient of the quantity in the row means), at the
    highest optimal level of the rows involved -- the same expression ``ratio`` evaluates for a pair."""
    if acc.K != len(COMPONENT_NAMES):
        raise ValueError(f"summarize: the accumulator holds {acc.K} series, the components are {len(COMPONENT_NAMES)}")
    out = {name: _column(acc, k) for k, name in enumerate(COMPONENT_NAMES)}
    idx = {name: k for k, name in enumerate(COMPONENT_NAMES)}
    mean = np.array([out[n]["mean"] for n in COMPONENT_NAMES])
    levels_reached = acc.result(0)["n_blocks"]

    def derived(value: float, g: np.ndarray) -> dict:
        rows = [COMPONENT_NAMES[k] for k in np.nonzero(g)[0]]
        lvl = max([out[n]["level"] for n in rows if out[n]["level"] is not None], default=0)
        cov = acc.covariance(lvl).numpy()
        q = float(g @ cov @ g)
        return {"value": value, "stderr": float(np.sqrt(max(q, 0.0) / float(levels_reached[lvl]))), "level": lvl}

    t = mean[idx["kinetic"]]
    v = sum(mean[idx[n]] for n in _POTENTIAL)
    g = np.zeros(len(COMPONENT_NAMES))
    for n in _POTENTIAL:
        g[idx[n]] = -1.0 / t
    g[idx["kinetic"]] = v / (t * t)
    out["virial_ratio"] = derived(-v / t, g)
    g = np.zeros(len(COMPONENT_NAMES))
    g[idx["kinetic"]], g[idx["kinetic_grad"]] = 1.0, -1.0
    out["kinetic_gap"] = derived(mean[idx["kinetic"]] - mean[idx["kinetic_grad"]], g)
    return out
