"""Generate tests/golden/components.npz: the float64 oracle's slow pieces for the energy-components
tests (tests/test_gpu_components.py), computed once.

Run from the repo root:  python tests/golden/make_golden_components.py
Cases (name, walkers): H2 5, Be 7, N2 7, C_ecp 5 (carbon ccECP), CO2_ecp 3 (C, O, O ccECP, a full
16-lane group).  Per case, seeded (alternating spins, randomised auxiliary parameters, walkers from
init_electrons rounded to float32 so that both dtypes and the oracle see the same positions):
  <name>_params  canonical parameter vector;  <name>_pos [B, 3N]
  <name>_ke      [B] oracle.hamiltonian.kinetic_jvp_of_grad of log|psi|
  <name>_grad    [B, 3N] grad log|psi|
  Be_ke_complex  [B] the real part of kinetic_complex_jvp_of_grad (complex_output=True)
  <name>_rot [B, 3, 3], <name>_nl_re [B]   (ECP cases) the injected grid rotations and the real part
                 of oracle.pphamiltonian.nonlocal_pp_energy
The potentials are cheap and are taken from the oracle live by the tests.
Oracle outputs, not reference outputs (JAX is absent here).
"""
import os
import sys

import numpy as np
import torch
from torch.func import grad, vmap

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import hamiltonian, network, pphamiltonian, system  # noqa: E402

torch.set_default_dtype(torch.float64)

CASES = {"H2": (5, 41, None), "Be": (7, 42, None), "N2": (7, 43, None),
         "C_ecp": (5, 44, pphamiltonian.c_atom_ccecp), "CO2_ecp": (3, 45, pphamiltonian.co2_ccecp)}


def case(name: str) -> dict:
    B, seed, tables = CASES[name]
    s = system.make_system(name)
    rng = np.random.default_rng(seed)
    params = system.init_params(rng, s, randomize_aux=True)
    pos = system.init_electrons(rng, s.atoms, s.charges, B, 1.0).astype(np.float32).astype(np.float64)
    net, pt = network.Network(s), network.to_torch(params)
    x = torch.tensor(pos)
    f = lambda y: net.logabs(pt, y)
    out = {"params": system.flatten_params(params), "pos": pos,
           "ke": vmap(hamiltonian.kinetic_jvp_of_grad(f))(x).detach().numpy(),
           "grad": vmap(grad(f))(x).detach().numpy()}
    if name == "Be":
        kc = hamiltonian.kinetic_complex_jvp_of_grad(f, lambda y: net.apply(pt, y)[0])
        out["ke_complex"] = vmap(kc)(x)[:, 0].detach().numpy()
    if tables is not None:
        rots = pphamiltonian.haar_rotations(rng, B)
        nl = [pphamiltonian.nonlocal_pp_energy(net, pt, tables(), x[b], rots[b])[0] for b in range(B)]
        out["rot"] = rots
        out["nl_re"] = np.array([complex(v.detach()).real for v in nl])
    print(name, "ke", out["ke"])
    return {f"{name}_{k}": v for k, v in out.items()}


if __name__ == "__main__":
    arrays = {}
    for n in CASES:
        arrays.update(case(n))
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "components.npz"), **arrays)
