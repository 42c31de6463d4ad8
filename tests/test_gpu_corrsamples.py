"""Correlated sampling on the GPU: aiqmc_space_warp, aiqmc_corr_level / aiqmc_corr_final and
aiqmc.correlatedsamples.estimator against the float64 host path and the float64 oracle.

Warp shapes, the smallest that take each path: (2,2) H2 four rows per wave, (4,1) Be the
translation case A = 1, (3,3) A = 3 and odd N, (10,5) the largest A, (16,3) every lane of a row
busy, (14,2) N2.  B in {1, 5, 8}, M in {1, 3}, |dR| <= 0.2 bohr, walkers rounded to float32 so that
both dtypes and the host see the same positions.

Warp tolerances (absolute; positions and log-determinants are O(1)): measured on an MI355X as the
largest error over all of these cases against the float64 host path, then 8 x that, rounded up to
one digit (few inputs are measured; the margin covers another machine's rounding of the same
kernels):
    fp64  newpos 4.44e-16 -> 4e-15,  logjac 2.44e-15 -> 2e-14
    fp32  newpos 2.27e-07 -> 2e-6,   logjac 6.80e-07 -> 6e-6
The estimator levels accumulate in float64 in a fixed tree order that is not torch's: each sum is
held to 1e-12 of the sum of the magnitudes of its terms (the scale of a sum's rounding error; for
the sums of positive terms that is rtol 1e-12).  sum d is zero but for rounding, so rtol on the
sum itself would have no meaning there.

End to end the bounds are composed from the per-value bounds of tests/test_gpu_shapes.py and
tests/test_gpu_parity.py (none new): fp64 log|psi| 1e-10 + 1e-10 |l| and |dE_L| <= 1e-6 (also the
ccECP bound of tests/test_ecp.py); fp32 log|psi| 2e-4 + 1e-5 |l| and E_L 2e-3 + 2e-4 |e|.  With
dl the bound of lw = 2 (l1 - l0) + logjac (twice the two log|psi| bounds plus the warp's logjac
bound), each weight is off by at most the factor exp(+-dl) against the normalisation, so to first
order |dE_m| <= de + 2 dl max_b |e1_b - E_m|, |dE_0| <= de, the ESS by 4 dl relative, and the
error bar by ||dd|| / sqrt(n (n - 1)) with dd_b the bound of d_b (the mean subtraction is a
projection).  The oracle is evaluated at the GPU's own warped positions (the warp is held to the
host path above).
"""
import dataclasses

import numpy as np
import pytest
import torch

import support

pytestmark = pytest.mark.gpu

SHAPES = {"H2": (2, 2), "Be": (4, 1), "Z1-1-1": (3, 3), "Z2-2-2-2-2": (10, 5), "CO2_ecp": (16, 3), "N2": (14, 2)}
BMAX = 8
# (newpos, logjac) absolute bounds
WARP_TOL = {torch.float64: (4e-15, 2e-14), torch.float32: (2e-6, 6e-6)}
LOGPSI_TOL = {torch.float64: (1e-10, 1e-10), torch.float32: (1e-5, 2e-4)}     # rtol, atol (test_gpu_shapes.py)
EL_TOL = {torch.float64: (0.0, 1e-6), torch.float32: (2e-4, 2e-3)}             # rtol, atol

_REF = {}


def _warp_case(name):
    """(system, pos [8, 3N] float32-representable, new_atoms [3, A, 3], host newpos [3, 8, 3N],
    host logjac [3, 8]) in float64, computed once per system."""
    if name not in _REF:
        from oracle import system
        from aiqmc.correlatedsamples import corrsamples, jacobianWeights
        s = system.make_system(name)
        assert (s.nelectrons, s.natoms) == SHAPES[name]
        rng = np.random.default_rng(500 + 7 * s.nelectrons + s.natoms)
        pos = system.init_electrons(rng, s.atoms, s.charges, BMAX, 1.0).astype(np.float32).astype(np.float64)
        new = s.atoms[None] + rng.uniform(-0.2, 0.2, size=(3, s.natoms, 3)) / np.sqrt(3.0)
        t = torch.tensor
        ref_pos = corrsamples.correlated_samples(t(s.atoms), t(new), t(pos)).numpy()
        ref_lj = jacobianWeights.log_weights_jacobian(t(pos), t(s.atoms), t(new)).numpy()
        _REF[name] = (s, pos, new, ref_pos, ref_lj)
    return _REF[name]


def _ctx(s, dtype, params=None, atoms=None):
    support.skip_unbuilt(s)
    return support.make_ctx(s, dtype, params, atoms=atoms)


def warp_errors(dtype, name, B, M):
    """Largest |newpos - host| and |logjac - host| of one case."""
    s, pos, new, ref_pos, ref_lj = _warp_case(name)
    ctx = _ctx(s, dtype)
    x = torch.tensor(pos[:B], device="cuda", dtype=dtype)
    newpos, logjac = ctx.space_warp(x, new[:M])
    torch.cuda.synchronize()
    assert newpos.shape == (M, B, pos.shape[1]) and logjac.shape == (M, B) and newpos.dtype == dtype
    return (float(np.abs(newpos.double().cpu().numpy() - ref_pos[:M, :B]).max()),
            float(np.abs(logjac.double().cpu().numpy() - ref_lj[:M, :B]).max()))


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("B", [1, 5, 8])
@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_space_warp_matches_host(dtype, name, B, M):
    e_pos, e_lj = warp_errors(dtype, name, B, M)
    print(f"{name} {dtype} B={B} M={M}: newpos {e_pos:.3g} logjac {e_lj:.3g}")
    assert e_pos <= WARP_TOL[dtype][0] and e_lj <= WARP_TOL[dtype][1]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_near_nucleus(dtype):
    """One electron of H2 at 0, 1e-12 and 1e-6 bohr from a nucleus: finite, and on the nucleus the
    electron moves with it and its block determinant is 1."""
    from aiqmc.correlatedsamples import jacobianWeights
    s, pos, new, _, _ = _warp_case("H2")
    x = pos[:4].copy()
    u = np.array([0.6, -0.64, 0.48])
    for b, eps in enumerate((0.0, 1e-12, 1e-6)):
        x[b, 3:] = s.atoms[1] + eps * u
    x = torch.tensor(x, dtype=dtype)          # rounded to the context dtype: what the kernel sees
    ctx = _ctx(s, dtype)
    newpos, logjac = ctx.space_warp(x.cuda(), new[:2])
    torch.cuda.synchronize()
    assert torch.isfinite(newpos).all() and torch.isfinite(logjac).all()
    newpos, logjac = newpos.double().cpu().numpy(), logjac.double().cpu().numpy()
    xd = x.double().numpy()
    # exactly on the nucleus as the kernel sees it (the atom rounded to the context dtype)
    assert np.all(xd[0, 3:] == torch.tensor(s.atoms[1], dtype=dtype).double().numpy())
    tol_pos, tol_lj = WARP_TOL[dtype]
    for m in range(2):
        assert np.abs(newpos[m, 0, 3:] - (xd[0, 3:] + new[m, 1] - s.atoms[1])).max() <= tol_pos
        # the other electron's block alone makes up the walker's log-determinant
        other = jacobianWeights.log_weights_jacobian(torch.tensor(xd[0, :3]), torch.tensor(s.atoms), torch.tensor(new[m]))
        assert abs(logjac[m, 0] - float(other)) <= tol_lj


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_translation_known_answer(dtype):
    """H2 with positions and one common dR on a 2^-10 grid: x + dR is exact, the Jacobian is the
    identity, and the translated context sees the same wavefunction."""
    from oracle import system
    s, pos, _, _, _ = _warp_case("H2")
    grid = lambda v: np.round(np.asarray(v) * 1024.0) / 1024.0
    x = grid(pos)
    dR = grid([0.123, -0.077, 0.051])
    new = (s.atoms + dR)[None]
    params = system.init_params(np.random.default_rng(41), s, randomize_aux=True)
    c0, c1 = _ctx(s, dtype, params), _ctx(s, dtype, params, atoms=new[0])
    xt = torch.tensor(x, device="cuda", dtype=dtype)
    newpos, logjac = c0.space_warp(xt, new)
    assert torch.equal(newpos[0], torch.tensor(x + np.tile(dR, 2), device="cuda", dtype=dtype))
    assert torch.equal(logjac, torch.zeros_like(logjac))
    l0, _ = c0.logpsi(xt)
    l1, _ = c1.logpsi(newpos[0])
    rtol, atol = LOGPSI_TOL[dtype]
    np.testing.assert_allclose(l1.double().cpu().numpy(), l0.double().cpu().numpy(), rtol=rtol, atol=atol)


@pytest.mark.parametrize("name", ["H2", "Z1-1-1", "N2"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_warp_is_deterministic_and_chunk_independent(dtype, name):
    s, pos, new, _, _ = _warp_case(name)
    ctx = _ctx(s, dtype)
    x = torch.tensor(pos, device="cuda", dtype=dtype)
    ws = ctx.workspace_bytes()
    a = ctx.space_warp(x, new)
    b = ctx.space_warp(x, new)
    lo, hi = ctx.space_warp(x[:4], new), ctx.space_warp(x[4:], new)
    one = [ctx.space_warp(x, new[m]) for m in range(3)]
    torch.cuda.synchronize()
    assert ctx.workspace_bytes() == ws
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], torch.cat([lo[0], hi[0]], dim=1)) and torch.equal(a[1], torch.cat([lo[1], hi[1]], dim=1))
    assert torch.equal(a[0], torch.cat([o[0] for o in one])) and torch.equal(a[1], torch.cat([o[1] for o in one]))
    empty = ctx.space_warp(x[:0], new)
    assert empty[0].shape == (3, 0, pos.shape[1]) and empty[1].shape == (3, 0)


def _level_inputs(n, M, kind, seed=5):
    rng = np.random.default_rng(seed + n + M)
    la0 = rng.normal(-3.0, 1.0, size=n)
    e0 = rng.normal(-14.6, 0.5, size=n)
    la1 = la0[None] + rng.normal(0.0, 0.3, size=(M, n))
    lj = rng.normal(0.0, 0.05, size=(M, n))
    e1 = e0[None] + 0.3 + rng.normal(0.0, 0.1, size=(M, n))
    if kind == "up":
        la1 += 400.0
    elif kind == "down":
        la1 -= 400.0
    elif kind == "nan":
        la1[M - 1, n // 2] = np.nan
    return la0, e0, la1, lj, e1


@pytest.mark.parametrize("kind", ["plain", "up", "down", "nan"])
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("n", [1, 5, 257])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_levels_match_host(dtype, n, M, kind):
    """Each level on the device against the host float64 level on the same inputs of `dtype` (and
    the same host L1 / L2), lw shifted by +-800 and with one NaN walker among the cases."""
    from aiqmc import _lib
    host = [torch.tensor(v, dtype=dtype) for v in _level_inputs(n, M, kind)]
    dev = [v.cuda() for v in host]
    la0, e0, la1, lj, e1 = (v.double().numpy() for v in host)
    h1 = _lib.corr_level(1, *host)
    d1 = _lib.corr_level(1, *dev)
    np.testing.assert_allclose(d1.cpu().numpy(), h1.numpy(), rtol=1e-12, atol=0)
    h2 = _lib.corr_level(2, *host, L1=h1)
    d2 = _lib.corr_level(2, *dev, L1=h1.cuda())
    w = np.exp(2 * (la1 - la0[None]) + lj - h1.numpy()[:, None])
    scale2 = np.stack([np.full(M, n), np.full(M, np.abs(e0).sum()), w.sum(1), (w * np.abs(e1)).sum(1), (w * w).sum(1)], 1)
    h3 = _lib.corr_level(3, *host, L1=h1, L2=h2)
    d3 = _lib.corr_level(3, *dev, L1=h1.cuda(), L2=h2.cuda())
    l2 = h2.numpy()
    E0, Em = l2[:, 1] / l2[:, 0], l2[:, 3] / l2[:, 2]
    d = (w * (l2[:, 0] / l2[:, 2])[:, None]) * (e1 - Em[:, None]) - (e0[None] - E0[:, None])
    scale3 = np.stack([np.abs(d).sum(1), (d * d).sum(1)], 1)
    hf, df = _lib.corr_final(h2, h3), _lib.corr_final(h2.cuda(), h3.cuda())
    again = (_lib.corr_level(1, *dev), _lib.corr_level(2, *dev, L1=h1.cuda()),
             _lib.corr_level(3, *dev, L1=h1.cuda(), L2=h2.cuda()), _lib.corr_final(h2.cuda(), h3.cuda()))
    torch.cuda.synchronize()
    for got, want, scale in ((d2, h2, scale2), (d3, h3, scale3)):
        got, want = got.cpu().numpy(), want.numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.all(np.abs(got - want)[ok] <= 1e-12 * scale[ok]), (got, want)
    np.testing.assert_allclose(df.cpu().numpy(), hf.numpy(), rtol=1e-12, atol=0)
    if kind == "nan":
        assert np.isnan(hf.numpy()[M - 1, 1:]).all() and np.isnan(df.cpu().numpy()[M - 1, 1:]).all()
    if n == 1 and kind != "nan":
        assert np.isnan(df.cpu().numpy()[:, 3]).all() and np.all(df.cpu().numpy()[:, 4] == 1.0)
    for a, b in zip((d1, d2, d3, df), again):       # equal bits from run to run
        assert torch.equal(a.cpu().view(torch.int64), b.cpu().view(torch.int64))


def _estimator_ref(la0, e0, la1, lj, e1):
    lw = 2 * (la1 - la0[None]) + lj
    w = np.exp(lw - lw.max(1, keepdims=True))
    n = la0.size
    E0, Em = e0.mean(), (w * e1).sum(1) / w.sum(1)
    rel = w * n / w.sum(1, keepdims=True)
    d = rel * (e1 - Em[:, None]) - (e0 - E0)[None]
    err = np.sqrt(((d * d).sum(1) - d.sum(1) ** 2 / n) / (n * (n - 1)))
    return E0, Em, err, w.sum(1) ** 2 / (w * w).sum(1), rel


def _check_estimator(res, la0, e0, la1, lj, e1, dtype, tol_lj):
    """energy_differences' result against the estimator formed in numpy from the oracle's values,
    with the bounds of the module docstring."""
    n = la0.size
    E0, Em, err, ess, rel = _estimator_ref(la0, e0, la1, lj, e1)
    lr, la = LOGPSI_TOL[dtype]
    er, ea = EL_TOL[dtype]
    dl = (2 * ((la + lr * np.abs(la1)) + (la + lr * np.abs(la0))[None]) + tol_lj).max(1)
    de0, de1 = (ea + er * np.abs(e0)).max(), (ea + er * np.abs(e1)).max(1)
    spread = np.abs(e1 - Em[:, None])
    dEm = de1 + 2 * dl * spread.max(1)
    dd = rel * (2 * dl[:, None] * spread + de1[:, None] + dEm[:, None]) + 2 * de0
    derr = np.sqrt((dd * dd).sum(1) / (n * (n - 1)))
    got = {k: getattr(res, k).cpu().numpy() for k in ("e0", "e", "delta", "err", "ess")}
    print(f"{dtype}: |dE0| {np.abs(got['e0'] - E0).max():.3g} (bound {de0:.3g}) |dEm| {np.abs(got['e'] - Em).max():.3g} "
          f"(bound {dEm.min():.3g}) |derr| {np.abs(got['err'] - err).max():.3g} (bound {derr.min():.3g}) "
          f"ESS rel {np.abs(got['ess'] / ess - 1).max():.3g} (bound {4 * dl.min():.3g})")
    assert np.all(np.abs(got["e0"] - E0) <= de0)
    assert np.all(np.abs(got["e"] - Em) <= dEm)
    assert np.all(np.abs(got["delta"] - (Em - E0)) <= dEm + de0)
    assert np.all(np.abs(got["err"] - err) <= derr)
    assert np.all(np.abs(got["ess"] - ess) <= 4 * dl * ess)


@pytest.mark.parametrize("name", ["H2", "Be"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_energy_differences_match_oracle(dtype, name):
    from oracle import hamiltonian, network, system
    from aiqmc.correlatedsamples import estimator, jacobianWeights
    from aiqmc.wavefunction_Ynlm import nn
    from aiqmc import systems
    s, pos, new, _, _ = _warp_case(name)
    new = new[:2]
    net = systems.make_system(name).make_network()
    params = system.init_params(np.random.default_rng(43), s, randomize_aux=True)
    x = torch.tensor(pos, device="cuda", dtype=dtype)
    data = nn.AINetData(positions=x, spins=s.spins, atoms=s.atoms, charges=s.charges)
    res = estimator.energy_differences(net.apply, params, data, new)
    assert all(getattr(res, k).shape == (2,) for k in ("e0", "e", "delta", "err", "ess"))
    again = estimator.energy_differences(net, params, data, new)       # the Network itself is accepted too
    assert torch.equal(res.delta, again.delta) and torch.equal(res.err, again.err)
    ain = net.apply._aiqmc_network
    newpos, _ = ain.context(s.atoms, dtype).space_warp(x, new)
    newpos = newpos.double().cpu()
    pt = network.to_torch(params)
    e0, la0, _ = hamiltonian.batch_local_energy(network.Network(s), pt, torch.tensor(pos))
    la1, e1 = [], []
    for m in range(2):
        e_m, l_m, _ = hamiltonian.batch_local_energy(network.Network(dataclasses.replace(s, atoms=new[m])), pt, newpos[m])
        la1.append(l_m.numpy())
        e1.append(e_m.numpy())
    lj = jacobianWeights.log_weights_jacobian(torch.tensor(pos), torch.tensor(s.atoms), torch.tensor(new)).numpy()
    _check_estimator(res, la0.numpy(), e0.numpy(), np.stack(la1), lj, np.stack(e1), dtype, WARP_TOL[dtype][1])


def test_energy_differences_ccecp_match_oracle():
    """C_ecp, one displaced geometry, injected rotations shared by both geometries."""
    from oracle import network, pphamiltonian as pp, system
    from aiqmc.Energy.pphamiltonian import HostRotations
    from aiqmc.correlatedsamples import estimator, jacobianWeights
    from aiqmc.wavefunction_Ynlm import nn
    from aiqmc import systems
    s = system.make_system("C_ecp")
    rng = np.random.default_rng(47)
    B = 4
    pos = system.init_electrons(rng, s.atoms, s.charges, B, 1.0).astype(np.float32).astype(np.float64)
    new = s.atoms[None] + np.array([[[0.05, -0.08, 0.11]]])
    rots = pp.haar_rotations(rng, B)
    params = system.init_params(rng, s, randomize_aux=True)
    net = systems.make_system("C_ecp").make_network()
    x = torch.tensor(pos, device="cuda")
    data = nn.AINetData(positions=x, spins=s.spins, atoms=s.atoms, charges=s.charges)
    res = estimator.energy_differences(net.apply, params, data, new, ecp=systems.ccecp_tables("C_ecp"),
                                       seed=HostRotations(torch.tensor(rots)))
    newpos, _ = net.apply._aiqmc_network.context(s.atoms, torch.float64).space_warp(x, new)
    newpos = newpos.cpu()
    pt, ecp = network.to_torch(params), pp.c_atom_ccecp()
    n0, n1 = network.Network(s), network.Network(dataclasses.replace(s, atoms=new[0]))
    logabs = lambda n, xs: np.array([float(n.apply(pt, r)[1]) for r in xs])
    e0 = pp.batch_local_energy_pp(n0, pt, ecp, torch.tensor(pos), rots)[0].real.numpy()
    e1 = pp.batch_local_energy_pp(n1, pt, ecp, newpos[0], rots)[0].real.numpy()
    lj = jacobianWeights.log_weights_jacobian(torch.tensor(pos), torch.tensor(s.atoms), torch.tensor(new)).numpy()
    _check_estimator(res, logabs(n0, torch.tensor(pos)), e0, logabs(n1, newpos[0])[None], lj, e1[None], torch.float64,
                     WARP_TOL[torch.float64][1])
    # Philox rotations from (seed, offset): reproducible, and another offset draws other rotations
    ph = [estimator.energy_differences(net.apply, params, data, new, ecp=systems.ccecp_tables("C_ecp"), seed=3, offset=o)
          for o in (5, 5, 6)]
    assert torch.isfinite(ph[0].delta).all() and torch.isfinite(ph[0].err).all()
    assert torch.equal(ph[0].e, ph[1].e) and torch.equal(ph[0].e0, ph[1].e0)
    assert not torch.equal(ph[0].e0, ph[2].e0)


def test_forces_are_differences_of_one_call():
    from oracle import system
    from aiqmc.correlatedsamples import estimator
    from aiqmc.wavefunction_Ynlm import nn
    from aiqmc import systems
    s, pos, _, _, _ = _warp_case("H2")
    net = systems.make_system("H2").make_network()
    params = system.init_params(np.random.default_rng(43), s, randomize_aux=True)
    data = nn.AINetData(positions=torch.tensor(pos, device="cuda"), spins=s.spins, atoms=s.atoms, charges=s.charges)
    F, err = estimator.forces_by_differences(net.apply, params, data, delta=1e-2)
    res = estimator.energy_differences(net.apply, params, data, estimator.displaced_geometries(s.atoms, 1e-2))
    assert F.shape == (2, 3) and err.shape == (2, 3) and res.delta.shape == (12,)
    d, e = res.delta.reshape(2, 3, 2), res.err.reshape(2, 3, 2)
    assert torch.equal(F, -(d[..., 0] - d[..., 1]) / 2e-2)
    assert torch.equal(err, torch.sqrt(e[..., 0] ** 2 + e[..., 1] ** 2) / 2e-2)
    assert torch.isfinite(F).all() and (err > 0).all()
