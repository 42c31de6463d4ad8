"""aiqmc.observables without a GPU: known answers of the S^2 estimator through the generic
(batched torch) path, the pair order, the dipole's closed form, option handling and the C-ABI's
host-side behaviour.

The known answers are properties of the wavefunctions, not of the code: a restricted
closed-shell determinant product is a singlet (S^2 psi = 0 as a function, so the estimator is 0
at EVERY configuration), a spatially antisymmetric two-electron function a triplet (2), a
restricted high-spin determinant with one unpaired electron a doublet (0.75).  float64 throughout;
the pointwise bound 1e-10 is rounding of the 2x2 determinants and exp/log round trips."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

from aiqmc import observables
from aiqmc.wavefunction_Ynlm.nn import AINetData

C1 = np.array([0.3, -0.2, 0.5])
C2 = np.array([-0.4, 0.1, 0.2])


def _phi(k, r):
    """Four arbitrary non-orthogonal orbitals on r [..., 3] (torch or numpy)."""
    lib = torch if isinstance(r, torch.Tensor) else np
    c1 = torch.tensor(C1) if lib is torch else C1
    c2 = torch.tensor(C2) if lib is torch else C2
    nrm = lambda v: (v * v).sum(-1) ** 0.5
    if k == 0:
        return lib.exp(-1.0 * nrm(r))
    if k == 1:
        return (r[..., 0] + 0.3) * lib.exp(-0.7 * nrm(r - c1))
    if k == 2:
        return lib.exp(-0.5 * nrm(r - c2)) + 0.2 * lib.exp(-1.3 * nrm(r))
    return (r[..., 2] - 0.1 * r[..., 1] + 0.4) * lib.exp(-0.9 * nrm(r - c2))


def _angle(sign):
    """The phase of a real psi (0 or pi) in the dtype of `sign`."""
    return torch.where(sign > 0, torch.zeros_like(sign), torch.full_like(sign, np.pi))


def _det_network(up, dn, up_orbs, dn_orbs):
    """psi = det[phi_a(r_up)] det[phi_a(r_dn)] in the package's apply convention (phase, log|psi|)."""
    def net(params, pos, spins, atoms, charges):
        x = pos.reshape(pos.shape[0], -1, 3)
        sign, logabs = 1.0, 0.0
        for slots, orbs in ((up, up_orbs), (dn, dn_orbs)):
            m = torch.stack([torch.stack([_phi(a, x[:, e]) for a in orbs], -1) for e in slots], -2)
            s, l = torch.linalg.slogdet(m)
            sign, logabs = sign * s, logabs + l
        return _angle(sign), logabs
    return net


def _det_psi_numpy(x, up, dn, up_orbs, dn_orbs):
    """The same determinant product for ONE configuration x [N, 3], plain numpy."""
    v = 1.0
    for slots, orbs in ((up, up_orbs), (dn, dn_orbs)):
        v *= np.linalg.det(np.array([[_phi(a, x[e]) for a in orbs] for e in slots]))
    return v


def _data(pos, spins):
    return AINetData(positions=torch.tensor(pos), spins=None if spins is None else np.asarray(spins, dtype=float),
                     atoms=np.zeros((1, 3)), charges=np.ones(1))


def _walkers(n, B=7, seed=0):
    return np.random.default_rng(seed).normal(size=(B, 3 * n))


def test_two_electron_singlet_is_zero():
    def net(params, pos, spins, atoms, charges):
        x = pos.reshape(-1, 2, 3)
        return torch.zeros(pos.shape[0], dtype=pos.dtype), -0.8 * x.norm(dim=-1).sum(-1)
    s2 = observables.make_s2(net, (1, 1))(None, _data(_walkers(2), [1, -1]))
    assert s2.shape == (7,) and torch.is_complex(s2)
    np.testing.assert_allclose(s2.real.numpy(), 0.0, atol=1e-10)
    np.testing.assert_allclose(s2.imag.numpy(), 0.0, atol=1e-10)


def test_two_electron_triplet_is_two():
    def net(params, pos, spins, atoms, charges):
        x = pos.reshape(-1, 2, 3)
        d = x[:, 0, 0] - x[:, 1, 0]
        return _angle(d), torch.log(d.abs()) - 0.8 * x.norm(dim=-1).sum(-1)
    s2 = observables.make_s2(net, (1, 1))(None, _data(_walkers(2, seed=1), [1, -1]))
    np.testing.assert_allclose(s2.real.numpy(), 2.0, atol=1e-10)
    np.testing.assert_allclose(s2.imag.numpy(), 0.0, atol=1e-10)


@pytest.mark.parametrize("spins", [[1, -1, 1, -1], [1, 1, -1, -1], None])
def test_restricted_closed_shell_determinant_is_a_singlet_pointwise(spins):
    s = np.array([1, 1, -1, -1] if spins is None else spins)
    up, dn = np.nonzero(s > 0)[0], np.nonzero(s < 0)[0]
    net = _det_network(up, dn, (0, 1), (0, 1))
    s2 = observables.make_s2(net, (2, 2))(None, _data(_walkers(4, seed=2), spins))
    np.testing.assert_allclose(s2.real.numpy(), 0.0, atol=1e-10)
    np.testing.assert_allclose(s2.imag.numpy(), 0.0, atol=1e-10)


def test_unrestricted_determinant_equals_the_formula_in_numpy():
    up, dn = (0, 2), (1, 3)
    net = _det_network(up, dn, (0, 1), (2, 3))
    pos = _walkers(4, seed=3)
    s2 = observables.make_s2(net, (2, 2))(None, _data(pos, [1, -1, 1, -1]))
    ref = np.zeros(len(pos))
    for b, x in enumerate(pos.reshape(-1, 4, 3)):
        psi0 = _det_psi_numpy(x, up, dn, (0, 1), (2, 3))
        acc = 0.0 * 1.0 + 2.0   # (na - nb)/2 ((na - nb)/2 + 1) + nb
        for i in up:
            for j in dn:
                y = x.copy()
                y[[i, j]] = x[[j, i]]
                acc -= _det_psi_numpy(y, up, dn, (0, 1), (2, 3)) / psi0
        ref[b] = acc
    assert np.abs(ref).min() > 1e-3            # spin contaminated at every walker
    np.testing.assert_allclose(s2.real.numpy(), ref, rtol=1e-10, atol=1e-10)
    assert np.all(np.abs(s2.imag.numpy()) <= 1e-10 * (1.0 + np.abs(ref))), s2.imag


def test_high_spin_restricted_determinant_is_a_doublet_pointwise():
    up, dn = (0, 2), (1,)
    net = _det_network(up, dn, (0, 1), (0,))
    s2 = observables.make_s2(net, (2, 1))(None, _data(_walkers(3, seed=4), [1, -1, 1]))
    np.testing.assert_allclose(s2.real.numpy(), 0.75, atol=1e-10)
    # the minority channel may be the first one: nspins (1, 2)
    net = _det_network((1,), (0, 2), (0,), (0, 1))
    s2 = observables.make_s2(net, (1, 2))(None, _data(_walkers(3, seed=5), [-1, 1, -1]))
    np.testing.assert_allclose(s2.real.numpy(), 0.75, atol=1e-10)


def test_pair_order_follows_the_spin_tables():
    """log psi = sum_e w_e x_e with distinct weights: exchanging slots i and j multiplies psi by
    exp((w_i - w_j)(x_j - x_i)), a different number for every pair of slots.  Up slots 0, 2 and
    down slots 1, 3: the ratios are those of (0,1), (0,3), (2,1), (2,3) in that order; the
    parallel pairs (0,2) and (1,3) do not appear."""
    w = np.array([0.1, 0.23, 0.37, 0.52])

    def net(params, pos, spins, atoms, charges):
        x = pos.reshape(-1, 4, 3)[:, :, 0]
        return torch.zeros(pos.shape[0], dtype=pos.dtype), (x * torch.tensor(w)).sum(-1)
    pos = _walkers(4, B=3, seed=6)
    est = observables.make_s2(net, (2, 2))
    data = _data(pos, [1, -1, 1, -1])
    r = est.pair_ratios(None, data)
    assert r.shape == (3, 2, 2)
    x = pos.reshape(3, 4, 3)[:, :, 0]
    ratio = lambda i, j: np.exp((w[i] - w[j]) * (x[:, j] - x[:, i]))
    expect = np.stack([np.stack([ratio(0, 1), ratio(0, 3)], -1), np.stack([ratio(2, 1), ratio(2, 3)], -1)], -2)
    np.testing.assert_allclose(r.real.numpy(), expect, rtol=1e-12)
    for par in ((0, 2), (1, 3)):
        assert np.abs(r.real.numpy() - ratio(*par)[:, None, None]).min() > 1e-6
    np.testing.assert_allclose(est(None, data).real.numpy(), 2.0 - expect.sum((1, 2)), rtol=1e-12)
    # the positions handed to the network: pair k = ia * n_down + ib
    xp = observables.exchanged_positions(torch.tensor(pos), (0, 2), (1, 3)).numpy().reshape(3, 4, 4, 3)
    for k, (i, j) in enumerate(((0, 1), (0, 3), (2, 1), (2, 3))):
        y = pos.reshape(3, 4, 3).copy()
        y[:, [i, j]] = y[:, [j, i]]
        np.testing.assert_array_equal(xp[:, k], y)


def test_spin_slots_must_match_nspins():
    net = lambda params, pos, spins, atoms, charges: (torch.zeros(len(pos)), torch.zeros(len(pos)))
    with pytest.raises(ValueError):
        observables.make_s2(net, (2, 2))(None, _data(_walkers(4), [1, 1, 1, -1]))


def test_dipole_closed_form():
    atoms = np.array([[0.0, 0.0, 1.5], [0.5, -2.0, 0.0], [-1.0, 0.25, 0.0]])
    charges = np.array([1.0, 2.0, 4.0])
    data = AINetData(positions=torch.zeros(1, 3, dtype=torch.float64), spins=None, atoms=atoms, charges=charges)
    mu = observables.make_dipole(lambda *a: None)(None, data)
    assert mu.shape == (1, 3)
    np.testing.assert_allclose(mu.numpy()[0], [1.0 - 4.0, -4.0 + 1.0, 1.5], rtol=0, atol=1e-15)
    # two electrons: minus the sum of their positions is added
    data.positions = torch.tensor([[0.5, 0.0, 0.0, 0.0, 1.0, -2.0]], dtype=torch.float64)
    mu = observables.make_dipole(lambda *a: None)(None, data)
    np.testing.assert_allclose(mu.numpy()[0], [-3.5, -4.0, 3.5], rtol=0, atol=1e-15)


def test_unbuilt_options_raise():
    net = lambda *a: None
    with pytest.raises(NotImplementedError, match="assign_spin"):
        observables.make_s2(net, (1, 1), assign_spin=False)
    with pytest.raises(NotImplementedError, match="states"):
        observables.make_s2(net, (1, 1), states=1)
    with pytest.raises(NotImplementedError, match="states"):
        observables.make_dipole(net, states=1)


def test_symbols_are_declared_exported_and_resolve():
    from aiqmc import _lib
    hdr = open(os.path.join(ROOT, "include", "aiqmc.h")).read()
    lib = _lib.load()
    for name in ("aiqmc_spin_squared", "aiqmc_dipole"):
        assert re.search(r"^int\s+" + name + r"\s*\(", hdr, re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None


def test_null_context_is_refused_without_a_gpu():
    from aiqmc import _lib
    lib = _lib.load()
    assert lib.aiqmc_spin_squared(None, None, 4, None, None, None, None, None) < 0
    assert "context" in _lib.last_error()
    assert lib.aiqmc_dipole(None, None, 4, None, None) < 0
    assert lib.aiqmc_debug_set_obs_chunk(None, 16) < 0
