"""aiqmc.observables.make_density without a GPU: the torch host path against a float64 numpy
replica of the bin rule, configuration checks, normalisation, a 2-rank gloo reduction and the
checkpoint round trip.

The replica (`replica`, also the reference of tests/test_gpu_density.py) uses nothing from the
package: f = (x - lo) * n / (hi - lo) in float64 (distances: f = r * n / r_max), inside iff
0 <= f < n, bin floor(f), everything else in the channel's outside word; a walker of weight w adds
rint(w 2^32) per sample.  It also counts the EDGE samples, |f - rint(f)| <= tol, whose bin a float32
(or float64) evaluation of the same rule may place differently: tol = 1e-4 for float32 inputs (f <= 64
here, a few float32 ulps of 64 are about 3e-5), 1e-10 for float64.  Every comparison first asserts
that its seeded input has NO edge sample and then demands exact integer equality.
"""
import os

import numpy as np
import pytest
import torch

import support
from conftest import ROOT
from replicas import (BMAX, GRID, ONE, PAIR, RADIAL, SYSTEMS, TOL, assert_counts_equal, geometry, replica,  # noqa: F401
                      walkers)


def _data(pos, name, dtype):
    from aiqmc.wavefunction_Ynlm.nn import AINetData
    atoms, per, spins = geometry(name)
    return AINetData(positions=torch.tensor(pos, dtype=dtype), spins=spins, atoms=atoms,
                     charges=np.asarray(per, dtype=np.float64))


def _nspins(name):
    s = geometry(name)[2]
    return int((s > 0).sum()), int((s < 0).sum())


_NET = lambda *a: None   # a generic callable: the host path (never evaluated)


@pytest.mark.parametrize("fam", ["all", "grid", "radial", "pair"])
@pytest.mark.parametrize("name", list(SYSTEMS))
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_host_path_equals_replica(dtype, name, fam):
    from aiqmc import observables
    atoms, _, spins = geometry(name)
    kw = {k: v for k, v in (("grid", GRID), ("radial", RADIAL), ("pair", PAIR)) if fam in ("all", k)}
    pos = walkers(name)
    ref, edges = replica(pos, atoms, spins, tol=TOL[dtype], **kw)
    assert edges == 0
    acc = observables.make_density(_NET, _nspins(name), **kw)
    acc.update(None, _data(pos, name, dtype))
    assert_counts_equal(acc.counts, ref)
    # conservation: inside + outside = total x electrons (pairs) of the channel
    c = {k: v.numpy() for k, v in acc.counts.items()}
    nup, ndn = _nspins(name)
    tot = int(c["total"][0])
    assert tot == BMAX * ONE
    if "grid" in kw:
        np.testing.assert_array_equal(c["grid"].sum((1, 2, 3)) + c["grid_out"], [tot * nup, tot * ndn])
    if "radial" in kw:
        np.testing.assert_array_equal(c["radial"].sum(2) + c["radial_out"],
                                      np.array([[tot * nup], [tot * ndn]]).repeat(len(atoms), 1))
    if "pair" in kw:
        np.testing.assert_array_equal(c["pair"].sum(1) + c["pair_out"],
                                      [tot * (nup * (nup - 1) // 2), tot * (ndn * (ndn - 1) // 2), tot * nup * ndn])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_weights_skips_and_non_finite_coordinates(dtype):
    from aiqmc import observables
    name = "Z5"
    atoms, _, spins = geometry(name)
    pos = walkers(name)[:12].copy()
    w = np.random.default_rng(5).uniform(0.0, 2.0, 12).astype(np.float32).astype(np.float64)
    w[3], w[7], w[9] = np.nan, -0.5, np.inf
    pos[1, 4], pos[2, 0], pos[3, 2] = np.nan, np.inf, np.nan   # walker 3 is skipped anyway
    ref, edges = replica(pos, atoms, spins, GRID, RADIAL, PAIR, weights=w, tol=TOL[dtype])
    assert edges == 0 and ref["skipped"][0] == 3
    acc = observables.make_density(_NET, _nspins(name), grid=GRID, radial=RADIAL, pair=PAIR)
    acc.update(None, _data(pos, name, dtype), weights=torch.tensor(w))
    assert_counts_equal(acc.counts, ref)
    # electron 1 of walker 1 (NaN y) and electron 0 of walker 2 (infinite x) are outside everywhere
    assert int(acc.counts["grid_out"].sum()) >= int(np.rint(w[1] * 2.0 ** 32) + np.rint(w[2] * 2.0 ** 32))
    # two updates on the halves, and a permuted order, give the same words
    acc2 = observables.make_density(_NET, _nspins(name), grid=GRID, radial=RADIAL, pair=PAIR)
    acc2.update(None, _data(pos[:5], name, dtype), weights=torch.tensor(w[:5]))
    acc2.update(None, _data(pos[5:], name, dtype), weights=torch.tensor(w[5:]))
    assert torch.equal(acc2.words, acc.words)
    p = np.random.default_rng(6).permutation(12)
    acc2.reset()
    acc2.update(None, _data(pos[p], name, dtype), weights=torch.tensor(w[p]))
    assert torch.equal(acc2.words, acc.words)


def test_spin_slots_come_from_data_spins():
    """Block spins [+, +, -, -] instead of alternating: the channels follow data.spins."""
    from aiqmc import observables
    atoms, per, _ = geometry("Be")
    spins = np.array([1.0, 1.0, -1.0, -1.0])
    pos = walkers("Be")[:9]
    ref, edges = replica(pos, atoms, spins, GRID, RADIAL, PAIR)
    assert edges == 0
    acc = observables.make_density(_NET, (2, 2), grid=GRID, radial=RADIAL, pair=PAIR)
    d = _data(pos, "Be", torch.float64)
    d.spins = spins
    acc.update(None, d)
    assert_counts_equal(acc.counts, ref)
    alt, _ = replica(pos, atoms, geometry("Be")[2], GRID, RADIAL, PAIR)
    assert not np.array_equal(alt["pair"], ref["pair"])


def test_config_validation_messages():
    from aiqmc import observables
    mk = lambda **kw: observables.make_density(_NET, (1, 1), **kw)
    with pytest.raises(ValueError, match=r"grid_hi\[1\] <= grid_lo\[1\]"):
        mk(grid=((0, 0, 0), (1, 0, 1), (4, 4, 4)))
    with pytest.raises(ValueError, match=r"grid_hi\[2\]"):
        mk(grid=((0, 0, 0), (1, 1, float("nan")), (4, 4, 4)))
    with pytest.raises(ValueError, match=r"negative grid_n\[0\]"):
        mk(grid=((0, 0, 0), (1, 1, 1), (-1, 4, 4)))
    with pytest.raises(ValueError, match="negative rad_n"):
        mk(radial=(1.0, -2))
    with pytest.raises(ValueError, match="negative pair_n"):
        mk(pair=(1.0, -2))
    with pytest.raises(ValueError, match="rad_max"):
        mk(radial=(0.0, 8))
    with pytest.raises(ValueError, match="pair_max"):
        mk(pair=(-1.0, 8))
    with pytest.raises(ValueError, match="pair_n above"):
        mk(pair=(1.0, (1 << 20) + 1))
    acc = mk(grid=((0, 0, 0), (1, 1, 1), (1 << 10, 1 << 10, 1 << 10)))
    with pytest.raises(ValueError, match="words"):
        acc.update(None, _data(walkers("H2")[:1], "H2", torch.float64))
    # a zero count leaves the family out, whatever its range says
    acc = mk(grid=((0, 0, 0), (0, 0, 0), (4, 0, 4)), radial=(0.0, 0), pair=(2.0, 4))
    acc.update(None, _data(walkers("H2")[:3], "H2", torch.float64))
    assert acc.counts["grid"].numel() == 0 and acc.counts["radial_out"].numel() == 0
    assert acc.layout["n_words"] == 2 + 3 * 4 + 3
    with pytest.raises(ValueError, match="nspins"):
        observables.make_density(_NET, (2, 1), pair=(2.0, 4)).update(None, _data(walkers("H2")[:3], "H2", torch.float64))
    with pytest.raises(RuntimeError, match="update"):
        mk(pair=(2.0, 4)).counts


def test_header_names_are_exported_and_refuse_a_null_context():
    import ctypes
    import re
    from aiqmc import _lib
    hdr = open(os.path.join(ROOT, "include", "aiqmc.h")).read()
    lib = _lib.load()
    for name in ("aiqmc_density_layout", "aiqmc_density_accumulate"):
        assert re.search(r"^int\s+" + name + r"\s*\(", hdr, re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    for k, v in (("LDS_WORDS", _lib.DENSITY_LDS_WORDS), ("MAX_BINS", _lib.DENSITY_MAX_BINS),
                 ("MAX_WORDS", _lib.DENSITY_MAX_WORDS)):
        m = re.search(r"#define AIQMC_DENSITY_" + k + r"\s+(\(?[0-9 <]+\)?)", hdr)
        assert eval(m.group(1)) == v, k
    cfg = _lib.density_cfg(pair=(2.0, 4))
    off, nw, pv = (ctypes.c_int64 * 8)(), ctypes.c_int64(), ctypes.c_int32()
    assert lib.aiqmc_density_layout(None, ctypes.byref(cfg), off, ctypes.byref(nw), ctypes.byref(pv)) < 0
    assert "context" in _lib.last_error()
    assert lib.aiqmc_density_accumulate(None, ctypes.byref(cfg), None, 4, None, None, None) < 0
    assert "context" in _lib.last_error()


def test_result_normalisation():
    """sum n dV + the outside electrons = the electrons of the spin; the radial shells and the pair
    counts close the same way; centres are the bin midpoints."""
    from aiqmc import observables
    name = "Z5"
    nup, ndn = _nspins(name)
    acc = observables.make_density(_NET, (nup, ndn), grid=GRID, radial=RADIAL, pair=PAIR)
    w = np.random.default_rng(8).uniform(0.0, 2.0, BMAX)
    acc.update(None, _data(walkers(name), name, torch.float64), weights=torch.tensor(w))
    r = acc.result()
    dv = np.prod([(GRID[1][d] - GRID[0][d]) / GRID[2][d] for d in range(3)])
    n_in = r["grid"].sum((1, 2, 3)).numpy() * dv
    assert 0.5 < n_in[0] < nup and 0.5 < n_in[1] < ndn
    np.testing.assert_allclose(n_in + r["grid_outside"].numpy(), [nup, ndn], rtol=1e-13)
    edges = np.arange(RADIAL[1] + 1) * RADIAL[0] / RADIAL[1]
    shell = 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
    np.testing.assert_allclose((r["radial"].numpy() * shell).sum(2) + r["radial_outside"].numpy(),
                               [[nup], [ndn]], rtol=1e-13)
    np.testing.assert_allclose(r["pair"].sum(1).numpy() + r["pair_outside"].numpy(),
                               [nup * (nup - 1) / 2, ndn * (ndn - 1) / 2, nup * ndn], rtol=1e-13)
    np.testing.assert_allclose(float(r["total"]), np.rint(w * 2.0 ** 32).sum() / 2.0 ** 32, rtol=1e-15)
    np.testing.assert_allclose(r["grid_centres"][2].numpy()[:2], [-3.5 + 7.0 / 32, -3.5 + 3 * 7.0 / 32], rtol=1e-14)
    np.testing.assert_allclose(r["radial_centres"].numpy()[[0, -1]], [0.125, 3.875], rtol=1e-14)
    np.testing.assert_allclose(r["pair_centres"].numpy()[0], 5.0 / 24, rtol=1e-14)
    assert int(r["skipped"]) == 0


def test_state_dict_round_trips(tmp_path):
    from aiqmc import observables
    name = "Be"
    mk = lambda: observables.make_density(_NET, _nspins(name), grid=GRID, radial=RADIAL, pair=PAIR)
    a = mk()
    a.update(None, _data(walkers(name)[:20], name, torch.float32))
    torch.save(a.state_dict(), tmp_path / "d.pt")
    sd = torch.load(tmp_path / "d.pt")
    assert all(isinstance(v, torch.Tensor) for v in sd.values())
    b = mk()
    b.load_state_dict(sd)
    assert torch.equal(a.words, b.words)
    # resumed and uninterrupted accumulation agree
    rest = _data(walkers(name)[20:], name, torch.float32)
    a.update(None, rest)
    b.update(None, rest)
    assert torch.equal(a.words, b.words)
    other = observables.make_density(_NET, _nspins(name), grid=GRID, radial=RADIAL, pair=(5.0, 13))
    with pytest.raises(ValueError, match="pair"):
        other.load_state_dict(sd)
    a.reset()
    assert int(a.words.abs().sum()) == 0


_WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "ab-initio-flexible-gaussian-basis-neural-network-quantum-monte-carlo_amd"))
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch, torch.distributed as dist
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
import test_density_host as T
acc, _ = T._two_rank_case(rank, world)
acc.reduce()
np.save(os.path.join(sys.argv[2], f"words_{rank}.npy"), acc.words.numpy())
dist.barrier()
dist.destroy_process_group()
'''


def _two_rank_case(rank, world):
    """This rank's block of the 70 N2 walkers (float32) with weights, accumulated on the host."""
    from aiqmc import observables
    name = "N2"
    pos = walkers(name)
    w = np.random.default_rng(9).uniform(0.0, 2.0, BMAX).astype(np.float32).astype(np.float64)
    n = BMAX // world
    sl = slice(rank * n, (rank + 1) * n)
    acc = observables.make_density(_NET, _nspins(name), grid=GRID, radial=RADIAL, pair=PAIR)
    acc.update(None, _data(pos[sl], name, torch.float32), weights=torch.tensor(w[sl]))
    return acc, (pos, w)


def test_two_rank_gloo_reduction_equals_one_process(tmp_path):
    world = 2
    assert support.run_ranks(_WORKER, world, [ROOT, str(tmp_path)], timeout=240) == [0] * world
    one, (pos, w) = _two_rank_case(0, 1)
    one.reduce()                         # the identity in a single process
    for r in range(world):
        np.testing.assert_array_equal(np.load(tmp_path / f"words_{r}.npy"), one.words.numpy())
    atoms, _, spins = geometry("N2")
    ref, edges = replica(pos, atoms, spins, GRID, RADIAL, PAIR, weights=w, tol=TOL[torch.float32])
    assert edges == 0
    assert_counts_equal(one.counts, ref)
