"""oracle.system.make_system names with an explicit spin pattern, "<system>@<u/d per slot>": the
spins, nspins and every table follow from the pattern (spin-polarised systems, minority-first
orderings, n_down > n_up); names without "@" resolve exactly as before."""
import numpy as np
import pytest

from oracle import system


@pytest.mark.parametrize("name,spins", [
    ("Z4@uuud", [1, 1, 1, -1]),
    ("Z3@ddu", [-1, -1, 1]),                       # minority first, n_down > n_up
    ("C_ecp@dudd", [-1, 1, -1, -1]),
    ("Z4-3@duddudd", [-1, 1, -1, -1, 1, -1, -1]),  # (2, 5) on two atoms
    ("Z8-8@" + "u" * 9 + "d" * 7, [1] * 9 + [-1] * 7),
])
def test_pattern_sets_spins_and_tables(name, spins):
    s = system.make_system(name)
    base = system.make_system(name.split("@")[0])
    spins = np.array(spins, dtype=np.float64)
    N = len(spins)
    up, dn = np.nonzero(spins > 0)[0], np.nonzero(spins < 0)[0]
    assert s.name == name and s.nelectrons == N
    np.testing.assert_array_equal(s.spins, spins)
    np.testing.assert_array_equal(s.atoms, base.atoms)
    np.testing.assert_array_equal(s.charges, base.charges)
    assert s.nspins == (len(up), len(dn))
    t = s.tables()
    np.testing.assert_array_equal(t["spin_up_indices"], up)
    np.testing.assert_array_equal(t["spin_down_indices"], dn)
    assert t["n_antiparallel"] == len(up) * len(dn)
    assert t["n_parallel"] + t["n_antiparallel"] == N * (N - 1) // 2
    assert t["parallel_indices"].shape == (2, t["n_parallel"])
    assert t["antiparallel_indices"].shape == (2, t["n_antiparallel"])
    # every pair (i < j) once, in the table of its spin product, row-major
    pairs = [(i, j) for i in range(N) for j in range(i + 1, N)]
    assert [tuple(p) for p in t["parallel_indices"].T] == [p for p in pairs if spins[p[0]] == spins[p[1]]]
    assert [tuple(p) for p in t["antiparallel_indices"].T] == [p for p in pairs if spins[p[0]] != spins[p[1]]]
    # init_params sizes the two Jastrow vectors from the tables
    params = system.init_params(np.random.default_rng(0), s)
    assert params["jastrow_ee"]["ee_par"].shape == (t["n_parallel"],)
    assert params["jastrow_ee"]["ee_anti"].shape == (t["n_antiparallel"],)


@pytest.mark.parametrize("name", ["Z4@uud", "Z4@uuudd", "Z4@uuuu", "Z4@dddd", "Z4@uuxd", "Z4@", "Z4@UUUD", "C_ecp@ud"])
def test_bad_patterns_are_refused(name):
    with pytest.raises((KeyError, ValueError)):
        system.make_system(name)
    with pytest.raises(KeyError):
        system.make_system("Nope@ud")


@pytest.mark.parametrize("name", ["H2", "Be", "C", "C_ecp", "Ne", "C2", "C2_ecp", "N2", "CO2_ecp", "O2", "Z5", "Z4-3",
                                  "Z5-4-4"])
def test_names_without_a_pattern_are_unchanged(name):
    s = system.make_system(name)
    n = s.nelectrons
    want = np.array([1.0] * 4 + [-1.0] * 4) if name == "C2_ecp" else system.alternating_spins(n)
    assert s.name == name
    np.testing.assert_array_equal(s.spins, want)
    assert s.nspins == (int((want > 0).sum()), int((want < 0).sum()))
    # the alternating pattern written out is the same system
    if name != "C2_ecp":
        p = system.make_system(name + "@" + "".join("u" if v > 0 else "d" for v in want)) if n > 1 else None
        np.testing.assert_array_equal(p.spins, s.spins)
        assert p.tables()["n_parallel"] == s.tables()["n_parallel"]
