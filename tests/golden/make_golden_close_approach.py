"""Generate tests/golden/close_approach_<name>.npz: float64 (and float32) oracle references on
walkers with an electron close to a nucleus or to another electron, for
tests/test_close_approach_host.py (the reference's own soundness) and
tests/test_gpu_close_approach.py (the kernels).

Run from the repo root:  python tests/golden/make_golden_close_approach.py [names] [--check]
(--check regenerates and compares every array bit for bit with the committed file; a few minutes
on one core.)  The oracle only; Oracle outputs, not reference outputs (JAX is absent here).

Systems, the smallest shape of each kernel family: Be (4,1) four configurations per wave, C (6,1)
two per wave, Z5-4 (9,2) one wave per walker with odd N and both atoms off the origin, C_ecp (4,1)
with the carbon ccECP tables.  Parameters init_params(rng, s, randomize_aux=True), seeded.

Walkers (row order; B = 19, odd, so the packed launches end in a partial wave that holds close
walkers): row 0 the ordinary base walker, row 1 a second ordinary walker (the pad that keeps B odd;
Z5-4 carries the bond-midpoint walker in its place), then for d in D = (1e-1, 1e-2, 1e-3, 1e-4) bohr
  en       electron 0 at R_0 + d u                 u  = (0.48, -0.6, 0.64)  (an exact unit vector)
  ee_anti  electron 1 at x_0 + d u                 (spins alternate: 0 and 1 antiparallel)
  ee_par   electron 2 at x_0 + d u                 (0 and 2 parallel)
  en2      electron 0 at R_0 + d u, electron 1 at R_0 + 2 d u'     u' = (-0.36, 0.48, 0.8)
and last  en_ax  electron 0 at R_0 + 1e-3 (1, 0, 0): two exact-zero components in the unit-vector
features.  (Not the z axis: there the 1/r^2 terms of the kinetic energy, 1e6 Ha each, cancel down to
|E_L| ~ 1e4 Ha, a cancellation inside the kinetic energy that S does not measure, and the oracle run
in float32 misses tol32 by a factor 2 (Be) to 21 (C); along x E_L keeps its 1/r^2 size and the
float32 oracle is within 0.15 tol32 on all four systems.)  Z5-4 row 1, mid: electron 0 exactly on the bond midpoint (the origin).
A displaced coordinate is base + d u rounded to float64; among the neighbouring float64 lattice
points (+-3 ulp per component) the one whose distance from the base is closest to d is taken, so
that every stored distance equals its target to 1e-12 relative even at d = 1e-4 next to
coordinates of order one.

Arrays (float64 unless noted):
  params_flat [P]; pos [B,3N]; pos32 [B,3N] float32 (pos rounded); kind [B] int8 (KINDS index);
  d [B] (0 for ordinary walkers); target, dist [B,2] the close distances (0 where unused): column 0
  r(electron 0, nucleus 0) for en / en2 / en_ax or r(x_0, x_j) for ee_*, column 1 r(electron 1,
  nucleus 0) of en2;
  logabs, phase [B], grad [B,3N], e_l [B] (batch_local_energy), e_re, e_im [B]
  (batch_local_energy_complex), v_ee, v_en, v_nn [B], S [B] = |E_L - V| + V_ee + |V_en| + V_nn (the
  cancellation scale), pgrad [B,P] (logabs_param_grad), delta_ref [B] the largest change of e_l over
  8 random one-ulp perturbations of the walker's coordinates;
  r32_{logabs,grad,e_l,S,v_ee,v_en}: the same float64 oracle at pos32 (what the fp32 kernels are compared
  with), o32_{e_l,logabs}: the oracle run in float32 / complex64 at pos32;
  start_* / land_*: one oracle.mcstep.walkers_update sweep each (tstep 0.05): x0 [B,3N], g1 [B,3N],
  g2d [B,N,3] (the diagonal blocks of gauss2 [B,N,3N], all that enters), u [B,N], cond [B,N] bool,
  acc [B,N] the acceptance values, x1 [B,3N], v2 [2] the two limdrift sums.  start: x0 = pos, random
  draws.  land: x0 = B copies of the base walker (row 1 the pad), and in every row of a close kind
  gauss1 of electron 0 solved as (target - x_0 - tstep grad_eff_0) / sqrt(tstep), grad_eff the
  oracle's limdrift over this batch, so that electron 0's proposal lands at distance d from nucleus
  0 (en, en2 along u', en_ax, mid) or from electron 1 / 2 (ee_anti / ee_par); land_dist [B] is the
  distance the oracle's own proposal ends at (equal to d up to the rounding of x_0 + g);
  dd_{x1,go,gn} [B,3N], dd_tdamp: oracle.dmc.drift_diffusion from pos with the start sweep's draws;
  C_ecp only: rot [B,3,3] Haar rotations, pp_e_re, pp_e_im, pp_loc [B] (batch_local_energy_pp),
  pp_S [B] = |Re E - V| + V_ee + |V_en| + V_nn with V = V_ee + V_nn + pp_loc and V_en the -Z/r part
  of pp_loc; r32_pp_e_re, r32_pp_e_im, r32_pp_S: the same at pos32.
"""
import itertools
import math
import os
import sys

import numpy as np
import torch
from torch.func import vmap

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import dmc, hamiltonian, loss, mcstep, network, pphamiltonian, system  # noqa: E402

torch.set_default_dtype(torch.float64)

HERE = os.path.dirname(os.path.abspath(__file__))
SYSTEMS = {"Be": 501, "C": 502, "Z5-4": 503, "C_ecp": 504}
D = (1e-1, 1e-2, 1e-3, 1e-4)
KINDS = ("base", "pad", "en", "ee_anti", "ee_par", "en2", "en_ax", "mid")
U = np.array([0.48, -0.6, 0.64])
U2 = np.array([-0.36, 0.48, 0.8])
TSTEP = 0.05


def place(base: np.ndarray, d: float, u: np.ndarray) -> np.ndarray:
    """The float64 point near base + d u whose distance from base is closest to d."""
    c0 = base + d * u
    sp = np.spacing(np.abs(c0))
    best, err = c0, abs(np.linalg.norm(c0 - base) - d)
    for off in itertools.product(range(-3, 4), repeat=3):
        c = c0 + np.array(off) * sp
        e = abs(np.linalg.norm(c - base) - d)
        if e < err:
            best, err = c, e
    return best


def walkers(s, rng):
    """pos [B,3N], kind [B], d [B], target [B,2], per-row landing target (point, reference point)."""
    N = s.nelectrons
    two = system.init_electrons(rng, s.atoms, s.charges, 2, 1.0).reshape(2, N, 3)
    base, R0 = two[0], s.atoms[0]
    rows, kinds, ds, tg, land = [base.copy()], ["base"], [0.0], [(0.0, 0.0)], [None]
    if s.natoms == 2:
        mid = base.copy()
        mid[0] = 0.5 * (s.atoms[0] + s.atoms[1])
        rows.append(mid), kinds.append("mid"), ds.append(0.0), tg.append((0.0, 0.0))
        land.append((mid[0].copy(), None))
    else:
        rows.append(two[1].copy()), kinds.append("pad"), ds.append(0.0), tg.append((0.0, 0.0)), land.append(None)
    for d in D:
        x = base.copy()
        x[0] = place(R0, d, U)
        rows.append(x), kinds.append("en"), ds.append(d), tg.append((d, 0.0)), land.append((x[0].copy(), R0))
        for kind, j in (("ee_anti", 1), ("ee_par", 2)):
            x = base.copy()
            x[j] = place(base[0], d, U)
            rows.append(x), kinds.append(kind), ds.append(d), tg.append((d, 0.0))
            land.append((place(base[j], d, U), base[j]))      # the landing sweep moves electron 0 next to j
        x = base.copy()
        x[0] = place(R0, d, U)
        x[1] = place(R0, 2 * d, U2)
        rows.append(x), kinds.append("en2"), ds.append(d), tg.append((d, 2 * d)), land.append((place(R0, d, U2), R0))
    x = base.copy()
    x[0] = place(R0, 1e-3, np.array([1.0, 0.0, 0.0]))
    assert x[0][1] == R0[1] and x[0][2] == R0[2]
    rows.append(x), kinds.append("en_ax"), ds.append(1e-3), tg.append((1e-3, 0.0)), land.append((x[0].copy(), R0))
    pos = np.stack(rows).reshape(len(rows), 3 * N)
    assert pos.shape[0] % 2 == 1
    return pos, np.array([KINDS.index(k) for k in kinds], np.int8), np.array(ds), np.array(tg), land, two


def distances(s, pos, kind):
    """[B,2]: the close distances of each row as the docstring lists them, recomputed from pos."""
    B = pos.shape[0]
    x = pos.reshape(B, -1, 3)
    R0 = s.atoms[0]
    out = np.zeros((B, 2))
    for b in range(B):
        k = KINDS[kind[b]]
        if k in ("en", "en2", "en_ax"):
            out[b, 0] = np.linalg.norm(x[b, 0] - R0)
        if k == "en2":
            out[b, 1] = np.linalg.norm(x[b, 1] - R0)
        if k == "ee_anti":
            out[b, 0] = np.linalg.norm(x[b, 1] - x[b, 0])
        if k == "ee_par":
            out[b, 0] = np.linalg.norm(x[b, 2] - x[b, 0])
    return out


def potentials(s, pos):
    atoms, charges = torch.tensor(s.atoms), torch.tensor(s.charges)
    v = np.zeros((3, pos.shape[0]))
    for b, x in enumerate(torch.tensor(pos)):
        r_ae, r_ee = hamiltonian.construct_r(x, atoms)
        v[0, b] = hamiltonian.potential_electron_electron(r_ee)
        v[1, b] = hamiltonian.potential_electron_nuclear(charges, r_ae)
        v[2, b] = hamiltonian.potential_nuclear_nuclear(charges, atoms)
    return v


def scale(e_l, v):
    return np.abs(e_l - v.sum(0)) + v[0] + np.abs(v[1]) + v[2]


def sweep(net, pt, x0, g1, g2, u):
    info = {}
    x1, acc = mcstep.walkers_update(net, pt, torch.tensor(x0), torch.tensor(g1), torch.tensor(g2), torch.tensor(u),
                                    TSTEP, info=info)
    B, n3 = x0.shape
    N = n3 // 3
    idx = np.arange(N)
    gx = info["grad_x"]
    te = info["taueff_proposals"]
    v2w = float(torch.sum(gx ** 2))
    # the proposals (walkers_update's x2) and their limdrift sum, which info does not carry
    g = (mcstep.limdrift(gx, TSTEP, 0.25) * TSTEP + math.sqrt(TSTEP) * torch.tensor(g1)).reshape(B, N, 3)
    xp = torch.tensor(x0).reshape(B, 1, N, 3).repeat(1, N, 1, 1)
    xp[:, idx, idx, :] += g
    f = lambda p: net.logabs(pt, p)
    gp = vmap(torch.func.grad(f))(xp.reshape(B * N, n3))
    v2p = float(torch.sum(gp ** 2))
    assert abs(float(mcstep.taueff(gp, TSTEP, 0.25)) - float(te)) <= 1e-12 * float(te)
    return dict(x0=x0, g1=g1, g2d=g2.reshape(B, N, N, 3)[:, idx, idx, :].copy(), u=u,
                cond=info["cond"].numpy(), acc=acc.numpy(), x1=x1.numpy(), v2=np.array([v2w, v2p])), xp.numpy()


def make(name: str) -> dict:
    torch.set_num_threads(1)
    s = system.make_system(name)
    rng = np.random.default_rng(SYSTEMS[name])
    params = system.init_params(rng, s, randomize_aux=True)
    net, pt = network.Network(s), network.to_torch(params)
    N = s.nelectrons
    pos, kind, d, target, land, two = walkers(s, rng)
    B = pos.shape[0]
    pos32 = pos.astype(np.float32)
    out = dict(params_flat=system.flatten_params(params), pos=pos, pos32=pos32, kind=kind, d=d, target=target,
               dist=distances(s, pos, kind))
    # float64 oracle at pos
    e, l, g = hamiltonian.batch_local_energy(net, pt, torch.tensor(pos))
    ph = vmap(lambda x: net.apply(pt, x)[0])(torch.tensor(pos))
    ec = hamiltonian.batch_local_energy_complex(net, pt, torch.tensor(pos))
    v = potentials(s, pos)
    out.update(logabs=l.numpy(), phase=ph.numpy(), grad=g.numpy(), e_l=e.numpy(), e_re=ec.real.numpy(),
               e_im=ec.imag.numpy(), v_ee=v[0], v_en=v[1], v_nn=v[2], S=scale(e.numpy(), v),
               pgrad=loss.logabs_param_grad(net, params, torch.tensor(pos)))
    # delta_ref
    delta = np.zeros(B)
    for _ in range(8):
        sign = rng.integers(0, 2, size=pos.shape) * 2 - 1
        p = np.nextafter(pos, np.where(sign > 0, np.inf, -np.inf))
        ep = hamiltonian.batch_local_energy(net, pt, torch.tensor(p))[0].numpy()
        delta = np.maximum(delta, np.abs(ep - out["e_l"]))
    out["delta_ref"] = delta
    # the rounded positions: float64 and float32 oracle
    p32 = pos32.astype(np.float64)
    e, l, g = hamiltonian.batch_local_energy(net, pt, torch.tensor(p32))
    v32 = potentials(s, p32)
    out.update(r32_logabs=l.numpy(), r32_grad=g.numpy(), r32_e_l=e.numpy(), r32_S=scale(e.numpy(), v32),
               r32_v_ee=v32[0], r32_v_en=v32[1])
    e, l, _ = hamiltonian.batch_local_energy(net, network.to_torch(params, torch.float32), torch.tensor(pos32))
    assert e.dtype == torch.float32
    out.update(o32_e_l=e.double().numpy(), o32_logabs=l.double().numpy())
    # the two sweeps
    g1 = rng.standard_normal((B, 3 * N))
    g2 = rng.standard_normal((B, N, 3 * N))
    u = rng.uniform(size=(B, N))
    st, _ = sweep(net, pt, pos, g1, g2, u)
    out.update({f"start_{k}": a for k, a in st.items()})
    x0 = np.repeat(two[0].reshape(1, 3 * N), B, axis=0)
    x0[1] = two[1].reshape(3 * N)
    gl1 = rng.standard_normal((B, 3 * N))
    gl2 = rng.standard_normal((B, N, 3 * N))
    ul = rng.uniform(size=(B, N))
    gx = vmap(torch.func.grad(lambda p: net.logabs(pt, p)))(torch.tensor(x0))
    ge = mcstep.limdrift(gx, TSTEP, 0.25).numpy()
    for b in range(B):
        if land[b] is not None:
            gl1[b, 0:3] = (land[b][0] - x0[b, 0:3] - TSTEP * ge[b, 0:3]) / math.sqrt(TSTEP)
    ld, xp = sweep(net, pt, x0, gl1, gl2, ul)
    out.update({f"land_{k}": a for k, a in ld.items()})
    out["land_dist"] = np.array([0.0 if land[b] is None or land[b][1] is None
                                 else np.linalg.norm(xp[b, 0, 0] - land[b][1]) for b in range(B)])
    # DMC drift-diffusion from the close walkers
    xn, td, go, gn = dmc.drift_diffusion(net, pt, torch.tensor(pos), torch.tensor(g1), torch.tensor(g2), torch.tensor(u), TSTEP)
    out.update(dd_x1=xn.numpy(), dd_tdamp=np.array(float(td)), dd_go=go.numpy(), dd_gn=gn.numpy())
    if name == "C_ecp":
        ecp = pphamiltonian.c_atom_ccecp()
        rots = pphamiltonian.haar_rotations(rng, B)
        out["rot"] = rots
        for tag, p in (("", pos), ("r32_", p32)):
            ee, _, loc, _ = pphamiltonian.batch_local_energy_pp(net, pt, ecp, torch.tensor(p), rots)
            ee, loc = ee.detach().numpy(), loc.detach().numpy()
            vv = potentials(s, p)
            S = np.abs(ee.real - (vv[0] + vv[2] + loc)) + vv[0] + np.abs(vv[1]) + vv[2]
            out.update({f"{tag}pp_e_re": ee.real.copy(), f"{tag}pp_e_im": ee.imag.copy(), f"{tag}pp_S": S})
            if not tag:
                out["pp_loc"] = loc
    for b in range(B):
        print(f"{name:6s} {b:2d} {KINDS[kind[b]]:8s} d={d[b]:.0e} E_L={out['e_l'][b]: .6e} S={out['S'][b]:.3e} "
              f"delta_ref={delta[b]:.1e} |grad|max={np.abs(out['grad'][b]).max():.2e}", flush=True)
    return out


def path(name: str) -> str:
    return os.path.join(HERE, f"close_approach_{name}.npz")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--check"]
    for n in args or list(SYSTEMS):
        arrays = make(n)
        if "--check" in sys.argv:
            old = np.load(path(n))
            assert sorted(old.files) == sorted(arrays), (sorted(old.files), sorted(arrays))
            for k, a in arrays.items():
                assert old[k].dtype == np.asarray(a).dtype and old[k].tobytes() == np.asarray(a).tobytes(), (n, k)
            print(n, "reproduced bit for bit")
        else:
            np.savez_compressed(path(n), **arrays)
            print(n, os.path.getsize(path(n)), "bytes")
