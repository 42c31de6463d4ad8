"""aiqmc_energy_components without a GPU: the export and its argument checks, the torch replica of
the kernel's potential formulas (aiqmc.Energy.components.potential_terms) against the float64
oracle, the row names against the header, ``summarize`` on a synthetic series, the factory's
argument checks, and the golden fixture of tests/test_gpu_components.py against the oracle."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

HEADER = os.path.join(ROOT, "include", "aiqmc.h")
NOECP = ["H2", "Be", "N2"]
ECP = {"C_ecp": "c_atom_ccecp", "C2_ecp": "c2_ccecp"}


def test_symbol_exported_and_arguments_checked_before_the_gpu():
    from aiqmc import _lib
    lib = _lib.load()
    src = open(HEADER).read()
    assert re.search(r"^int\s+aiqmc_energy_components\s*\(", src, re.M)
    assert "aiqmc_energy_components" in _lib.EXPORTED_SYMBOLS
    fn = lib.aiqmc_energy_components
    buf = (8 * 8 * 4) * b"\0"
    for args in ((None, buf, 4, 0, 1, None, 0, 0, buf, None),      # null context
                 (None, buf, 4, 0, 1, None, 0, 0, None, None),     # null out as well
                 (None, buf, -1, 0, 1, None, 0, 0, buf, None)):    # negative B
        assert fn(*args) != 0
        msg = _lib.last_error()
        assert isinstance(msg, str) and msg


def test_component_names_match_the_header_macros():
    from aiqmc import _lib
    from aiqmc.Energy import components
    src = open(HEADER).read()
    n = int(re.search(r"^#define AIQMC_NCOMPONENTS (\d+)", src, re.M).group(1))
    macros = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"^#define AIQMC_COMP_(\w+) (\d+)", src, re.M)}
    assert n == 8 and len(_lib.COMPONENT_NAMES) == 8 == len(macros)
    assert components.COMPONENT_NAMES is _lib.COMPONENT_NAMES
    for k, name in enumerate(_lib.COMPONENT_NAMES):
        assert macros[name] == k, (name, macros)
    assert n == _lib.BLOCKING_MAX_SERIES


def _oracle_terms(s, pos, ecp):
    """[4, B] float64: the oracle's v_ee, v_en, v_nn and local pp part without part1."""
    from oracle import hamiltonian as ham, pphamiltonian as pp
    atoms, charges = torch.tensor(s.atoms), torch.tensor(s.charges)
    out = []
    for x in torch.tensor(pos):
        r_ae, r_ee = ham.construct_r(x, atoms)
        # part1 = -Z / r (pseudopotential.py:111) vanishes identically for zero charges: what is
        # left of local_pp_energy is its Gaussian part, with no cancellation
        loc = pp.local_pp_energy(ecp, x, atoms, torch.zeros_like(charges)) if ecp is not None else torch.zeros(())
        out.append(torch.stack([ham.potential_electron_electron(r_ee), ham.potential_electron_nuclear(charges, r_ae),
                                ham.potential_nuclear_nuclear(charges, atoms), loc.to(torch.float64)]))
    return torch.stack(out).T.numpy()


@pytest.mark.parametrize("name", NOECP + list(ECP))
def test_potential_terms_match_the_oracle(name):
    from oracle import pphamiltonian as pp, system
    from aiqmc.Energy import components
    s = system.make_system(name)
    ecp = getattr(pp, ECP[name])() if name in ECP else None
    pos = system.init_electrons(np.random.default_rng(500 + len(name) + s.nelectrons), s.atoms, s.charges, 5, 1.0)
    loc = None if ecp is None else (ecp.rn_local, ecp.local_coes, ecp.local_exps)
    got = components.potential_terms(torch.tensor(pos), s.atoms, s.charges, loc)
    assert got.shape == (4, 5) and got.dtype == torch.float64
    ref = _oracle_terms(s, pos, ecp)
    print(name, "max relative difference per row:",
          np.max(np.abs(got.numpy() - ref) / np.maximum(np.abs(ref), 1e-300), axis=1))
    np.testing.assert_allclose(got.numpy(), ref, rtol=1e-13, atol=0)
    if ecp is None:
        assert (got[3] == 0).all()
    else:   # and with its part1: the whole local_pp_energy is v_en + v_pp_local
        full = [float(pp.local_pp_energy(ecp, x, torch.tensor(s.atoms), torch.tensor(s.charges))) for x in torch.tensor(pos)]
        np.testing.assert_allclose((got[1] + got[3]).numpy(), full, rtol=1e-13, atol=0)


def test_potential_terms_coincident_electrons_stay_in_their_walker():
    from oracle import system
    from aiqmc.Energy import components
    s = system.make_system("H2")
    pos = system.init_electrons(np.random.default_rng(3), s.atoms, s.charges, 4, 1.0).astype(np.float32)
    bad = pos.copy()
    bad[2, 3:6] = bad[2, 0:3]
    a = components.potential_terms(torch.tensor(pos), s.atoms, s.charges)
    b = components.potential_terms(torch.tensor(bad), s.atoms, s.charges)
    assert a.dtype == torch.float32 and b[0, 2] == float("inf")
    keep = [0, 1, 3]
    assert torch.equal(a[:, keep], b[:, keep])


def test_summarize_synthetic_series():
    from aiqmc import statistics
    from aiqmc.Energy import components
    names = components.COMPONENT_NAMES
    rng = np.random.default_rng(77)
    means = np.array([-9.0, 7.0, 6.5, 5.0, -20.0, 3.0, -1.5, 0.75])
    T, B = 64, 6
    x = means[None, :, None] + rng.standard_normal((T, 8, B))
    acc = statistics.make_blocking(nseries=8, names=names)
    for row in x:
        acc.update(torch.tensor(row))            # CPU tensors: the torch path
    s = components.summarize(acc)
    m = x.mean(axis=(0, 2))
    for k, n in enumerate(names):
        assert abs(s[n]["mean"] - m[k]) <= 1e-12 * abs(m[k]), (n, s[n], m[k])
        r = acc.result(k)
        assert s[n]["level"] == r["optimal_level"] and s[n]["stderr"] == r["stderr_opt"]
    pot = [names.index(n) for n in ("v_ee", "v_en", "v_nn", "v_pp_local", "v_pp_nonlocal")]
    want = -m[pot].sum() / m[1]
    assert abs(s["virial_ratio"]["value"] - want) <= 1e-12 * abs(want)
    assert abs(s["kinetic_gap"]["value"] - (m[1] - m[2])) <= 1e-12 * abs(m[1] - m[2])
    # the error bars are what the accumulator's `ratio` gives for the pair (sum of the potential
    # rows, kinetic), and for the pair (kinetic - kinetic_grad, 1), at the same level
    two = statistics.make_blocking(nseries=2)
    gap = statistics.make_blocking(nseries=2)
    for row in x:
        two.update(torch.tensor(np.stack([row[pot].sum(0), row[1]])))
        gap.update(torch.tensor(np.stack([row[1] - row[2], np.ones(B)])))
    lv = s["virial_ratio"]["level"]
    r = two.ratio(0, 1)
    assert abs(-float(r["ratio"][lv]) - s["virial_ratio"]["value"]) <= 1e-12 * abs(want)
    np.testing.assert_allclose(s["virial_ratio"]["stderr"], float(r["stderr"][lv]), rtol=1e-10)
    lg = s["kinetic_gap"]["level"]
    np.testing.assert_allclose(s["kinetic_gap"]["stderr"], float(gap.ratio(0, 1)["stderr"][lg]), rtol=1e-10)
    assert s["virial_ratio"]["stderr"] > 0 and s["kinetic_gap"]["stderr"] > 0
    with pytest.raises(ValueError):
        components.summarize(two)


def test_summarize_constant_rows_have_zero_error():
    from aiqmc import statistics
    from aiqmc.Energy import components
    rng = np.random.default_rng(5)
    x = rng.standard_normal((16, 8, 4))
    x[:, 5] = 23.5          # v_nn
    x[:, 6:] = 0.0          # no ECP
    acc = statistics.make_blocking(nseries=8)
    for row in x:
        acc.update(torch.tensor(row))
    s = components.summarize(acc)
    assert s["v_nn"] == {"mean": 23.5, "stderr": 0.0, "level": 0}
    assert s["v_pp_nonlocal"]["mean"] == 0.0 and s["v_pp_nonlocal"]["stderr"] == 0.0


def test_factory_argument_checks():
    from oracle import system
    from aiqmc import systems
    from aiqmc.Energy import components
    with pytest.raises(TypeError):
        components.make_energy_components(lambda *a: (0, 0), np.ones(1), (1, 0))
    s = systems.make_system("H2")
    net = s.make_network()
    with pytest.raises(ValueError):
        components.make_energy_components(net.apply, s.charges + 1.0, s.nspins)
    with pytest.raises(ValueError):       # some pseudopotential tables, not all
        components.make_energy_components(net.apply, s.charges, s.nspins, rn_local=[[1.0]] * 2)
    with pytest.raises(TypeError):
        components.make_energy_components(net.apply, s.charges, s.nspins, bogus=1)
    f = components.make_energy_components(net.apply, s.charges, s.nspins)
    assert callable(f) and f._aiqmc_network is net.apply._aiqmc_network
    assert system.make_system("H2").nelectrons == s.nelectrons


@pytest.mark.parametrize("name", ["H2", "C_ecp"])
def test_golden_fixture_is_the_oracle(name):
    """The cheap cases of tests/golden/components.npz (make_golden_components.py) recomputed."""
    from torch.func import grad, vmap
    from oracle import hamiltonian as ham, network, pphamiltonian as pp, system
    g = np.load(os.path.join(GOLDEN, "components.npz"))
    s = system.make_system(name)
    x = torch.tensor(g[f"{name}_pos"])
    assert np.array_equal(g[f"{name}_pos"], g[f"{name}_pos"].astype(np.float32).astype(np.float64))
    net = network.Network(s)
    template = system.init_params(np.random.default_rng(0), s)
    pt = network.to_torch(system.unflatten_params(template, g[f"{name}_params"]))
    f = lambda y: net.logabs(pt, y)
    np.testing.assert_allclose(vmap(ham.kinetic_jvp_of_grad(f))(x).detach().numpy(), g[f"{name}_ke"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(vmap(grad(f))(x).detach().numpy(), g[f"{name}_grad"], rtol=1e-10, atol=1e-10)
    if name == "C_ecp":
        nl = pp.nonlocal_pp_energy(net, pt, pp.c_atom_ccecp(), x[1], g[f"{name}_rot"][1])[0]
        np.testing.assert_allclose(complex(nl.detach()).real, g[f"{name}_nl_re"][1], rtol=1e-10, atol=1e-12)
