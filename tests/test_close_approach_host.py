"""The close-approach fixtures (tests/golden/close_approach_<name>.npz, make_golden_close_approach.py)
checked on the CPU, the reference alone: the preconditions under which tests/test_gpu_close_approach.py
keeps every walker.

Per system (Be, C, Z5-4, C_ecp; 19 walkers with an electron 1e-1 ... 1e-4 bohr from a nucleus or from
another electron):
  * two walkers per file (one en at d = 1e-3, one ee_par at d = 1e-4) recomputed by the oracle equal
    the stored log|psi|, gradient and E_L (1e-13 of the walker's cancellation scale S: the rounding
    of a different vmap batch);
  * every close distance recomputed from the stored float64 positions equals its target to 1e-12
    relative (and the stored one exactly); the landing sweep's proposals end at their distance to
    1e-10 (they are the oracle's x_0 + g, rounded at coordinates of order one);
  * every reference is finite;
  * delta_ref, the change of the fp64 E_L under one-ulp perturbations of the coordinates, is at most
    tol64 / 10, tol64 = 1e-9 max(S, 1e3) Ha;
  * the oracle run in float32 is within tol32 = 2e-4 max(S, 10) of the float64 oracle at the same
    float32-rounded positions, every walker;
  * every Metropolis acceptance value of the two sweeps differs from its uniform by at least 1e-6
    relative, so no decision the GPU test compares is marginal.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

NAMES = ["Be", "C", "Z5-4", "C_ecp"]
KINDS = ("base", "pad", "en", "ee_anti", "ee_par", "en2", "en_ax", "mid")


def tol64(S):
    return 1e-9 * np.maximum(S, 1e3)


def tol32(S):
    return 2e-4 * np.maximum(S, 10.0)


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, f"close_approach_{name}.npz")))


@pytest.mark.parametrize("name", NAMES)
def test_fixture_equals_a_fresh_oracle_evaluation(name):
    from oracle import hamiltonian, network, system
    g = _load(name)
    s = system.make_system(name)
    params = system.unflatten_params(system.init_params(np.random.default_rng(0), s), g["params_flat"])
    kind, d = g["kind"], g["d"]
    rows = [int(np.flatnonzero((kind == KINDS.index("en")) & (d == 1e-3))[0]),
            int(np.flatnonzero((kind == KINDS.index("ee_par")) & (d == 1e-4))[0])]
    e, l, gr = hamiltonian.batch_local_energy(network.Network(s), network.to_torch(params), torch.tensor(g["pos"][rows]))
    S = g["S"][rows]
    assert np.all(np.abs(e.numpy() - g["e_l"][rows]) <= 1e-13 * S), (e.numpy(), g["e_l"][rows])
    np.testing.assert_allclose(l.numpy(), g["logabs"][rows], rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(gr.numpy(), g["grad"][rows], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_layout_and_distances(name):
    from oracle import system
    g = _load(name)
    s = system.make_system(name)
    pos, kind, d, target = g["pos"], g["kind"], g["d"], g["target"]
    B, N = pos.shape[0], s.nelectrons
    assert B % 2 == 1 and pos.shape == (B, 3 * N)
    assert g["pos32"].dtype == np.float32 and np.array_equal(g["pos32"], pos.astype(np.float32))
    names = [KINDS[k] for k in kind]
    for k in ("en", "ee_anti", "ee_par", "en2"):
        assert sorted(d[[i for i, n in enumerate(names) if n == k]]) == [1e-4, 1e-3, 1e-2, 1e-1], k
    assert names.count("base") == 1 and names.count("en_ax") == 1 and names[-1] != "pad"
    assert ("mid" in names) == (s.natoms == 2)
    x, R0 = pos.reshape(B, N, 3), s.atoms[0]
    for b, n in enumerate(names):
        got = np.zeros(2)
        if n in ("en", "en2", "en_ax"):
            got[0] = np.linalg.norm(x[b, 0] - R0)
        if n == "en2":
            got[1] = np.linalg.norm(x[b, 1] - R0)
        if n in ("ee_anti", "ee_par"):
            got[0] = np.linalg.norm(x[b, 1 if n == "ee_anti" else 2] - x[b, 0])
        assert np.array_equal(got, g["dist"][b]), (b, n)
        assert np.all(np.abs(got - target[b]) <= 1e-12 * target[b]), (b, n, got, target[b])
        if n == "en_ax":
            assert x[b, 0, 1] == R0[1] and x[b, 0, 2] == R0[2]
        if n == "mid":
            assert np.array_equal(x[b, 0], 0.5 * (s.atoms[0] + s.atoms[1]))
    ld = g["land_dist"]
    close = ld > 0
    assert close.sum() == 17
    assert np.all(np.abs(ld[close] - d[close]) <= 1e-10 * d[close]), (ld, d)


@pytest.mark.parametrize("name", NAMES)
def test_references_are_finite_and_well_conditioned(name):
    g = _load(name)
    for k, a in g.items():
        if a.dtype.kind == "f":
            assert np.isfinite(a).all(), k
    S = g["S"]
    print(name, "delta_ref / tol64", (g["delta_ref"] / tol64(S)).max())
    assert np.all(g["delta_ref"] <= tol64(S) / 10), (g["delta_ref"], tol64(S))
    err = np.abs(g["o32_e_l"] - g["r32_e_l"])
    print(name, "fp32 oracle |dE| / tol32", (err / tol32(g["r32_S"])).max())
    assert np.all(err <= tol32(g["r32_S"])), (err, tol32(g["r32_S"]))
    np.testing.assert_allclose(g["o32_logabs"], g["r32_logabs"], rtol=1e-5, atol=2e-4)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("sweep", ["start", "land"])
def test_no_metropolis_decision_is_marginal(name, sweep):
    g = _load(name)
    acc, u, cond = g[f"{sweep}_acc"], g[f"{sweep}_u"], g[f"{sweep}_cond"]
    assert np.array_equal(cond, acc > u)
    gap = np.abs(acc - u) / np.maximum(np.abs(acc), u)
    assert gap.min() >= 1e-6, (gap.min(), np.unravel_index(gap.argmin(), gap.shape))
    moved = np.any(g[f"{sweep}_x1"].reshape(*cond.shape, 3) != g[f"{sweep}_x0"].reshape(*cond.shape, 3), axis=2)
    assert np.array_equal(moved, cond)
    assert cond.sum() > 0
