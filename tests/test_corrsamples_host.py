"""Correlated sampling on the host (float64): the space warp, its Jacobian, the estimator levels.

aiqmc.correlatedsamples.corrsamples / jacobianWeights are pure torch; the estimator's three levels
(_lib.corr_level / corr_final) have a torch float64 path for host tensors, which a generic callable
network takes throughout.  Bounds: the Jacobian against autograd to rtol 1e-10 (the repository's
float64 log|psi| bound); the reference's r^-4 / sum r^-4 formula to 1e-13 relative on walkers at
least 0.1 bohr from every nucleus; two gloo ranks against one process to 1e-12 relative.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import support

SITES = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [1.2, 0.7, 0.3], [-0.9, 1.1, -0.4], [0.3, -1.3, 0.8]])


def _case(A, N, seed, B=3):
    rng = np.random.default_rng(seed)
    atoms = SITES[:A].copy()
    new = atoms + rng.uniform(-0.2, 0.2, size=(A, 3)) / np.sqrt(3.0)
    pos = (atoms[rng.integers(0, A, size=(B, N))] + rng.standard_normal((B, N, 3))).reshape(B, 3 * N)
    return torch.tensor(atoms), torch.tensor(new), torch.tensor(pos)


@pytest.mark.parametrize("A,N", [(2, 2), (3, 3), (3, 10), (5, 3), (5, 10)])
def test_jacobian_matches_autograd(A, N):
    """det of the full 3N x 3N autograd Jacobian of correlated_samples == prod_i det J_i."""
    from aiqmc.correlatedsamples import corrsamples, jacobianWeights
    atoms, new, pos = _case(A, N, 10 * A + N)
    wj = jacobianWeights.weights_jacobian(pos, atoms, new)
    lj = jacobianWeights.log_weights_jacobian(pos, atoms, new)
    assert wj.shape == (pos.shape[0],)
    for b in range(pos.shape[0]):
        jac = torch.autograd.functional.jacobian(lambda x: corrsamples.correlated_samples(atoms, new, x), pos[b])
        blocks = jac.reshape(N, 3, N, 3)
        off = blocks.clone()
        off[torch.arange(N), :, torch.arange(N), :] = 0.0
        assert float(off.abs().max()) == 0.0           # electrons move independently
        det = float(torch.linalg.det(jac))
        assert abs(float(wj[b]) - det) <= 1e-10 * abs(det), (float(wj[b]), det)
        assert abs(float(lj[b]) - np.log(abs(det))) <= 1e-10 * max(1.0, abs(np.log(abs(det))))
        one = jacobianWeights.weights_jacobian(pos[b], atoms, new)      # the reference's single-configuration call
        assert one.shape == () and float(one) == float(wj[b])


def test_single_atom_is_a_translation():
    from aiqmc.correlatedsamples import corrsamples, jacobianWeights
    atoms, _, pos = _case(1, 4, 3)
    new = atoms + torch.tensor([[0.11, -0.07, 0.05]], dtype=torch.float64)
    out = corrsamples.correlated_samples(atoms, new, pos)
    assert torch.equal(out, pos + (new - atoms).repeat(1, 4))
    assert torch.equal(jacobianWeights.weights_jacobian(pos, atoms, new), torch.ones(3, dtype=torch.float64))
    assert torch.equal(jacobianWeights.log_weights_jacobian(pos, atoms, new), torch.zeros(3, dtype=torch.float64))


def test_common_displacement_and_identity():
    from aiqmc.correlatedsamples import corrsamples, jacobianWeights
    atoms, new, pos = _case(3, 5, 4)
    shift = torch.tensor([0.13, -0.02, 0.09], dtype=torch.float64)
    out = corrsamples.correlated_samples(atoms, atoms + shift, pos)
    np.testing.assert_allclose(out.numpy(), (pos + shift.repeat(5)).numpy(), rtol=0, atol=4 * 2.0 ** -52 * 4.0)
    lj = jacobianWeights.log_weights_jacobian(pos, atoms, atoms + shift)
    assert float(lj.abs().max()) <= 5 * 4 * 2.0 ** -52      # 4 ulp of 1 per electron
    assert torch.equal(corrsamples.correlated_samples(atoms, atoms.clone(), pos), pos)     # dR = 0: bitwise
    assert torch.equal(jacobianWeights.log_weights_jacobian(pos, atoms, atoms.clone()), torch.zeros(3, dtype=torch.float64))
    # batched geometries and the shapes of the results
    both = torch.stack([new, atoms + shift])
    ob = corrsamples.correlated_samples(atoms, both, pos)
    assert ob.shape == (2, 3, 15) and torch.equal(ob[1], out)
    assert torch.equal(ob[0], corrsamples.correlated_samples(atoms, new, pos))
    assert corrsamples.correlated_samples(atoms, new, pos[0]).shape == (15,)
    assert jacobianWeights.log_weights_jacobian(pos, atoms, both).shape == (2, 3)


def test_near_and_on_nucleus():
    """On a nucleus the electron moves with it and the block determinant is 1; at 1e-3, 1e-6 and
    1e-12 bohr everything is finite and tends monotonically to that limit."""
    from aiqmc.correlatedsamples import corrsamples, jacobianWeights
    atoms, new, _ = _case(3, 1, 5)
    u = torch.tensor([0.6, -0.64, 0.48], dtype=torch.float64)
    dist_pos, dist_det = [], []
    for eps in (1e-3, 1e-6, 1e-12, 0.0):
        x = atoms[1] + eps * u
        y = corrsamples.correlated_samples(atoms, new, x)
        det = jacobianWeights.weights_jacobian(x, atoms, new)
        lj = jacobianWeights.log_weights_jacobian(x, atoms, new)
        assert torch.isfinite(y).all() and torch.isfinite(det) and torch.isfinite(lj)
        dist_pos.append(float((y - (x + new[1] - atoms[1])).abs().max()))
        dist_det.append(abs(float(det) - 1.0))
    assert dist_pos[3] == 0.0 and dist_det[3] == 0.0
    assert dist_pos[0] >= dist_pos[1] >= dist_pos[2] >= dist_pos[3] and dist_pos[0] > 0.0
    assert dist_det[0] >= dist_det[1] >= dist_det[2] >= dist_det[3] and dist_det[0] > 0.0
    # float32 at the same distances: finite as well (r^-4 itself would overflow)
    for eps in (1e-3, 1e-6, 1e-12, 0.0):
        x = (atoms[1] + eps * u).float()
        assert torch.isfinite(corrsamples.correlated_samples(atoms, new, x)).all()
        assert torch.isfinite(jacobianWeights.log_weights_jacobian(x, atoms, new))


@pytest.mark.parametrize("A,N", [(2, 2), (3, 10), (5, 3)])
def test_reference_formula(A, N):
    """r' = r + sum_a (r_a^-4 / sum_b r_b^-4) dR_a, written out in numpy float64."""
    from aiqmc.correlatedsamples import corrsamples
    atoms, new, pos = _case(A, N, 77 + A, B=16)
    a, n, p = atoms.numpy(), new.numpy(), pos.numpy().reshape(16, N, 3)
    r_ae = np.linalg.norm(p[:, :, None, :] - a[None, None], axis=-1)
    keep = r_ae.min(axis=(1, 2)) >= 0.1
    assert keep.sum() >= 4
    k = 1.0 / r_ae ** 4
    wts = k / k.sum(-1, keepdims=True)
    ref = (p + np.einsum("bna,ac->bnc", wts, n - a)).reshape(16, 3 * N)[keep]
    out = corrsamples.correlated_samples(atoms, new, pos).numpy()[keep]
    np.testing.assert_allclose(out, ref, rtol=1e-13, atol=0)


# ----------------------------------------------------------------------------- estimator
class ToyNetwork:
    """psi = exp(-alpha sum_{i,a} r_ia) with its local energy written out."""

    def __init__(self, alpha, with_energy=True):
        self.alpha = alpha
        if with_energy:
            self.local_energy = self._local_energy

    def __call__(self, params, pos, spins, atoms, charges):
        r = torch.linalg.norm(pos.reshape(pos.shape[0], -1, 1, 3) - atoms[None, None], dim=-1)
        return torch.zeros(pos.shape[0], dtype=pos.dtype), -self.alpha * r.sum((-2, -1))

    def _local_energy(self, params, pos, atoms, charges):
        K, N = pos.shape[0], pos.shape[1] // 3
        p = pos.reshape(K, N, 3)
        d = p[:, :, None] - atoms[None, None]
        r = torch.linalg.norm(d, dim=-1)
        grad = -self.alpha * (d / r[..., None]).sum(2)
        lap = -self.alpha * (2.0 / r).sum((-2, -1))
        iu = torch.triu_indices(N, N, 1)
        v = (1.0 / torch.linalg.norm(p[:, iu[0]] - p[:, iu[1]], dim=-1)).sum(-1) - (charges / r).sum((-2, -1))
        ia = torch.triu_indices(atoms.shape[0], atoms.shape[0], 1)
        v = v + (charges[ia[0]] * charges[ia[1]] / torch.linalg.norm(atoms[ia[0]] - atoms[ia[1]], dim=-1)).sum()
        return v - 0.5 * (lap + (grad * grad).sum((-2, -1)))


def _toy_data(B=12, seed=8):
    from aiqmc.wavefunction_Ynlm import nn
    atoms, new, pos = _case(2, 2, seed, B=B)
    return nn.AINetData(positions=pos, spins=None, atoms=atoms, charges=torch.tensor([1.0, 1.0], dtype=torch.float64)), new


def _numpy_estimator(la0, e0, la1, lj, e1):
    lw = 2 * (la1 - la0[None]) + lj
    w = np.exp(lw - lw.max(1, keepdims=True))
    n = la0.size
    E0, Em = e0.mean(), (w * e1).sum(1) / w.sum(1)
    d = (w * n / w.sum(1, keepdims=True)) * (e1 - Em[:, None]) - (e0 - E0)[None]
    err = np.sqrt(((d * d).sum(1) - d.sum(1) ** 2 / n) / (n * (n - 1)))
    return np.full(len(Em), E0), Em, Em - E0, err, w.sum(1) ** 2 / (w * w).sum(1)


def test_generic_network_takes_the_host_path():
    from aiqmc.correlatedsamples import corrsamples, estimator, jacobianWeights
    data, new = _toy_data()
    net = ToyNetwork(0.9)
    geoms = torch.stack([new, data.atoms.clone()])
    res = estimator.energy_differences(net, None, data, geoms)
    # geometry 1 is the primary one: w = 1 and e1 = e0
    assert float(res.delta[1]) == 0.0 and float(res.ess[1]) == 12.0 and float(res.e[1]) == float(res.e0[1])
    # geometry 0 against the estimator written out in numpy
    x1 = corrsamples.correlated_samples(data.atoms, new, data.positions)
    ch = data.charges
    ref = _numpy_estimator(net(None, data.positions, None, data.atoms, ch)[1].numpy(),
                           net.local_energy(None, data.positions, data.atoms, ch).numpy(),
                           net(None, x1, None, new, ch)[1].numpy()[None],
                           jacobianWeights.log_weights_jacobian(data.positions, data.atoms, new).numpy()[None],
                           net.local_energy(None, x1, new, ch).numpy()[None])
    for got, want in zip((res.e0, res.e, res.delta, res.err, res.ess), ref):
        np.testing.assert_allclose(float(got[0]), want[0], rtol=1e-12)
    assert 1.0 < float(res.ess[0]) <= 12.0 and float(res.err[0]) > 0.0
    # without a hand-coded local energy the generic path differentiates log|psi| itself
    auto = estimator.energy_differences(ToyNetwork(0.9, with_energy=False), None, data, geoms)
    np.testing.assert_allclose(auto.e.numpy(), res.e.numpy(), rtol=1e-10)
    np.testing.assert_allclose(auto.e0.numpy(), res.e0.numpy(), rtol=1e-10)


def _level_inputs(n, M, seed=5):
    rng = np.random.default_rng(seed)
    la0 = rng.normal(-3.0, 1.0, size=n)
    e0 = rng.normal(-14.6, 0.5, size=n)
    la1 = la0[None] + rng.normal(0.0, 0.3, size=(M, n))
    lj = rng.normal(0.0, 0.05, size=(M, n))
    e1 = e0[None] + 0.3 + rng.normal(0.0, 0.1, size=(M, n))
    return la0, e0, la1, lj, e1


@pytest.mark.parametrize("shift", [0.0, 400.0, -400.0])
def test_levels_equal_numpy_and_are_shift_invariant(shift):
    """lw shifted by +-800: exp(lw) itself overflows / underflows float64; the max-shift of level 1
    makes the result the unshifted one."""
    from aiqmc.correlatedsamples import estimator
    la0, e0, la1, lj, e1 = _level_inputs(40, 3)
    ref = _numpy_estimator(la0, e0, la1, lj, e1)
    t = torch.tensor
    res = estimator.reduce_levels(t(la0), t(e0), t(la1 + shift), t(lj), t(e1))
    for got, want in zip((res.e0, res.e, res.delta, res.err, res.ess), ref):
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-10)
    assert np.all(np.isfinite(res.err.numpy()))


def test_single_walker_and_nan_walker():
    from aiqmc.correlatedsamples import estimator
    t = torch.tensor
    la0, e0, la1, lj, e1 = _level_inputs(1, 2)
    res = estimator.reduce_levels(t(la0), t(e0), t(la1), t(lj), t(e1))
    assert torch.isnan(res.err).all() and torch.isfinite(res.e).all() and torch.equal(res.ess, torch.ones(2, dtype=torch.float64))
    la0, e0, la1, lj, e1 = _level_inputs(9, 2)
    la1[1, 4] = np.nan
    res = estimator.reduce_levels(t(la0), t(e0), t(la1), t(lj), t(e1))
    assert torch.isnan(res.e[1]) and torch.isnan(res.delta[1]) and torch.isnan(res.err[1]) and torch.isnan(res.ess[1])
    assert torch.isfinite(res.e[0]) and torch.isfinite(res.err[0])


def test_forces_are_differences_of_one_call():
    from aiqmc.correlatedsamples import estimator
    data, _ = _toy_data()
    net = ToyNetwork(0.9)
    F, err = estimator.forces_by_differences(net, None, data, delta=1e-2)
    geoms = estimator.displaced_geometries(data.atoms, 1e-2)
    assert geoms.shape == (12, 2, 3) and F.shape == (2, 3) and err.shape == (2, 3)
    res = estimator.energy_differences(net, None, data, geoms)
    d, e = res.delta.numpy(), res.err.numpy()
    for a in range(2):
        for c in range(3):
            k = 2 * (3 * a + c)
            assert geoms[k, a, c] - float(data.atoms[a, c]) == pytest.approx(1e-2)
            assert float(F[a, c]) == -(d[k] - d[k + 1]) / 2e-2
            assert float(err[a, c]) == pytest.approx(np.sqrt(e[k] ** 2 + e[k + 1] ** 2) / 2e-2, rel=1e-14)
    assert np.all(np.isfinite(F.numpy())) and np.all(err.numpy() > 0.0)


# ----------------------------------------------------------------------------- C-ABI, arguments
def test_symbols_declared_exported_and_refusing():
    from aiqmc import _lib
    from conftest import ROOT
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "aiqmc.h")).read()
    for s in ("aiqmc_space_warp", "aiqmc_corr_level", "aiqmc_corr_final"):
        assert f"int {s}(" in hdr and s in _lib.EXPORTED_SYMBOLS
        getattr(lib, s)
    assert lib.aiqmc_space_warp(None, None, 0, None, 0, None, None, None) < 0
    assert "null context" in _lib.last_error()
    assert lib.aiqmc_corr_level(1, _lib.AIQMC_F64, 0, 1, None, None, None, None, None, None, None, None, None) < 0
    assert lib.aiqmc_corr_level(4, _lib.AIQMC_F64, 3, 1, None, None, None, None, None, None, None, None, None) < 0
    assert lib.aiqmc_corr_level(1, 7, 3, 1, None, None, None, None, None, None, None, None, None) < 0
    assert lib.aiqmc_corr_level(1, _lib.AIQMC_F64, 3, 1, None, None, None, None, None, None, None, None, None) < 0
    assert lib.aiqmc_corr_final(None, None, 1, None, None) < 0


def test_python_argument_checks():
    from aiqmc import _lib
    from aiqmc.correlatedsamples import corrsamples, estimator
    la0, e0, la1, lj, e1 = (torch.tensor(v) for v in _level_inputs(5, 2))
    with pytest.raises(ValueError):
        _lib.corr_level(0, la0, e0, la1, lj, e1)
    with pytest.raises(ValueError):
        _lib.corr_level(2, la0, e0, la1, lj, e1)            # no L1
    with pytest.raises(ValueError):
        _lib.corr_level(3, la0, e0, la1, lj, e1, L1=torch.zeros(2, dtype=torch.float64))   # no L2
    data, new = _toy_data()
    with pytest.raises(ValueError):
        estimator.energy_differences(ToyNetwork(0.9), None, data, torch.zeros(1, 3, 3))
    with pytest.raises(ValueError):
        corrsamples.correlated_samples(data.atoms, new, torch.zeros(4, dtype=torch.float64))


def test_driver_needs_a_checkpoint(tmp_path):
    from aiqmc.VMC import VMC_energy_correlated_samples as drv
    from aiqmc import systems
    s, t = systems.make_system("C_ecp"), systems.ccecp_tables("C_ecp")
    with pytest.raises(ValueError, match="correlated samples VMC must use the wave function from VMC"):
        drv.main(s.atoms, s.atoms[None] + 0.01, s.charges, s.spins, 0.05, 4, 2, 1, 3, 4, 1, 2, s.nspins,
                 str(tmp_path / "save"), str(tmp_path / "restore"), t.rn_local, t.local_coes, t.local_exps,
                 t.rn_non_local, t.non_local_coes, t.non_local_exps, 10.0, None)


# ----------------------------------------------------------------------------- two ranks
def _worker(rank, world, port, q):
    import sys
    from conftest import PKG
    sys.path.insert(0, PKG)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from aiqmc.correlatedsamples import estimator
    la0, e0, la1, lj, e1 = _level_inputs(6 * world, 3)
    sl = slice(6 * rank, 6 * (rank + 1))
    t = torch.tensor
    res = estimator.reduce_levels(t(la0[sl]), t(e0[sl]), t(la1[:, sl]), t(lj[:, sl]), t(e1[:, sl]))
    q.put((rank, [v.numpy() for v in (res.e0, res.e, res.delta, res.err, res.ess)]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_one_process():
    """2 x 6 walkers through the host levels with gloo all-reduces (MAX, SUM, SUM) == 12 walkers
    in one process."""
    from aiqmc.correlatedsamples import estimator
    world = 2
    port = support.free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(world)], key=lambda v: v[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    t = torch.tensor
    one = estimator.reduce_levels(*(t(v) for v in _level_inputs(6 * world, 3)))
    for _, vals in res:
        for got, want in zip(vals, (one.e0, one.e, one.delta, one.err, one.ess)):
            np.testing.assert_allclose(got, want.numpy(), rtol=1e-12, atol=0)
