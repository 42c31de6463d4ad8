"""aiqmc_spin_squared / aiqmc_dipole on the GPU against the float64 oracle forward (oracle/network.py).

Per case the exchanged positions are built with numpy, the oracle evaluates psi on them and on the
walkers, and dlogabs, dphase and S2_L = diag - sum_pairs exp(dlogabs) e^{i dphase} follow from those.
Shapes: the smallest that take each dispatch of the value launch -- H2 (2,2) four configurations
per wave and a single pair, Be (4,1) four per wave, (5,1) with nspins (3,2) two per wave, unequal
channels and odd N, (8,2) the two-per-wave boundary, (9,1) with nspins (5,4) the first one-wave
shape, N2 (14,2).  Batches 5 (no multiple of a packing factor: the partial last wave) and 8.
Spin-polarised: Z4@dudd (1,3), Z5@uuuud (4,1), Z9@uuuuduuuu (8,1), as tests/test_gpu_spin_polarised.py.
Otherwise alternating spins; randomised auxiliary parameters, as tests/test_gpu_shapes.py.  The walkers are
rounded to float32 so that both dtypes and the oracle see the same positions.

Tolerances (none of them new):
  fp64  log|psi| rtol 1e-10 / atol 1e-10 (test_gpu_shapes.py), phase 1e-9 through cos / sin
        (test_gpu_parity.py), doubled because dlogabs and dphase are differences of two values;
  fp32  log|psi| rtol 1e-5 / atol 2e-4 (test_gpu_shapes.py, test_gpu_parity.py), doubled; those
        files have no fp32 phase bound: log|psi| and the phase are the real and imaginary part of
        one complex log det, so the phase takes log|psi|'s absolute bound 2e-4, doubled;
  S2_L  the per-pair bounds weighted by |ratio| and summed over the walker's pairs.
"""
import os

import numpy as np
import pytest
import torch

import support
from replicas_estimators import TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# spin-polarised walkers, "<system>@<u/d per slot>" (oracle/system.py): (1,3) with n_down > n_up, (4,1)
# two per wave, (8,1) one wave -- the pair index k runs over n_up * n_down with k / n_down, k % n_down
POLARISED = ["Z4@dudd", "Z5@uuuud", "Z9@uuuuduuuu"]
CASES = ["H2", "Be", "Z5", "Z4-4", "Z9", "N2"] + POLARISED
BMAX = 8

_REF = {}


def _exchange(pos, up, dn):
    """[B, n_up * n_down, 3N]: slots up[ia] and dn[ib] exchanged, pair ia * n_down + ib."""
    B, n3 = pos.shape
    out = np.empty((B, len(up) * len(dn), n3))
    for ia, i in enumerate(up):
        for ib, j in enumerate(dn):
            y = pos.reshape(B, -1, 3).copy()
            y[:, [i, j]] = y[:, [j, i]]
            out[:, ia * len(dn) + ib] = y.reshape(B, n3)
    return out


def _case(name):
    """(system, params, pos [8, 3N], xpos [8, K, 3N], dlogabs, dphase [8, n_up, n_down], s2 [8] complex)
    of the float64 oracle, computed once per system."""
    if name not in _REF:
        from oracle import network, system
        s = system.make_system(name)
        rng = np.random.default_rng(300 + 7 * s.nelectrons + s.natoms)
        params = system.init_params(rng, s, randomize_aux=True)
        pos = system.init_electrons(rng, s.atoms, s.charges, BMAX, 1.0).astype(np.float32).astype(np.float64)
        t = s.tables()
        up, dn = t["spin_up_indices"], t["spin_down_indices"]
        xpos = _exchange(pos, up, dn)
        net, pt = network.Network(s), network.to_torch(params)
        # the oracle forward takes one configuration [3N]
        psi = lambda x: np.array([[float(v) for v in net.apply(pt, r)] for r in torch.tensor(x)]).T
        ph0, la0 = psi(pos)
        ph1, la1 = (v.reshape(BMAX, -1) for v in psi(xpos.reshape(-1, pos.shape[1])))
        dl, dp = la1 - la0[:, None], ph1 - ph0[:, None]
        na, nb = max(s.nspins), min(s.nspins)
        diag = 0.5 * (na - nb) * (0.5 * (na - nb) + 1.0) + nb
        s2 = diag - (np.exp(dl) * np.exp(1j * dp)).sum(1)
        shp = (BMAX, len(up), len(dn))
        _REF[name] = (s, params, pos, xpos, dl.reshape(shp), dp.reshape(shp), s2)
    return _REF[name]


def _ctx(s, params, dtype):
    support.skip_unbuilt(s)
    return support.make_ctx(s, dtype, params)


@pytest.mark.parametrize("B", [5, 8])
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_spin_squared_matches_oracle(dtype, name, B):
    s, params, pos, _, dl_ref, dp_ref, s2_ref = _case(name)
    rtol, atol, atol_ph = TOL[dtype]
    ctx = _ctx(s, params, dtype)
    x = torch.tensor(pos[:B], device="cuda", dtype=dtype)
    s2, dl, dp = ctx.spin_squared(x, want_pairs=True)
    torch.cuda.synchronize()
    assert dl.shape == (B,) + tuple(s.nspins) and dp.shape == dl.shape and s2.shape == (B,)
    dl, dp = dl.double().cpu().numpy(), dp.double().cpu().numpy()
    s2 = s2.to(torch.complex128).cpu().numpy()
    dl_ref, dp_ref, s2_ref = dl_ref[:B], dp_ref[:B], s2_ref[:B]
    mag = np.exp(dl_ref)
    bound = (mag * (atol + rtol * np.abs(dl_ref) + atol_ph)).sum((1, 2))
    e_l = np.abs(dl - dl_ref) / (atol + rtol * np.abs(dl_ref))
    e_p = np.maximum(np.abs(np.cos(dp) - np.cos(dp_ref)), np.abs(np.sin(dp) - np.sin(dp_ref))) / atol_ph
    e_s = np.abs(s2 - s2_ref) / bound
    print(f"{name} {dtype} B={B}: dlogabs {e_l.max():.3g} dphase {e_p.max():.3g} s2 {e_s.max():.3g} of the bounds; "
          f"max |dlogabs err| {np.abs(dl - dl_ref).max():.3g}, sum|ratio| max {mag.sum((1, 2)).max():.3g}")
    np.testing.assert_allclose(dl, dl_ref, rtol=rtol, atol=atol)
    np.testing.assert_allclose(np.cos(dp), np.cos(dp_ref), atol=atol_ph)
    np.testing.assert_allclose(np.sin(dp), np.sin(dp_ref), atol=atol_ph)
    assert np.all(np.abs(s2.real - s2_ref.real) <= bound), (s2.real, s2_ref.real, bound)
    assert np.all(np.abs(s2.imag - s2_ref.imag) <= bound), (s2.imag, s2_ref.imag, bound)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_pairs_are_logpsi_differences_bitwise(dtype, name):
    """The exchanged configurations go through the launch aiqmc_logpsi uses, so dlogabs / dphase
    are, bit for bit, Context.logpsi on host-built exchanged positions minus logpsi at the walker."""
    s, params, pos, xpos, _, _, _ = _case(name)
    B = 5
    ctx = _ctx(s, params, dtype)
    x = torch.tensor(pos[:B], device="cuda", dtype=dtype)
    xx = torch.tensor(xpos[:B].reshape(-1, pos.shape[1]), device="cuda", dtype=dtype)
    _, dl, dp = ctx.spin_squared(x, want_pairs=True)
    la0, ph0 = ctx.logpsi(x)
    la1, ph1 = ctx.logpsi(xx)
    torch.cuda.synchronize()
    K = xpos.shape[1]
    dl_h = la1.reshape(B, K) - la0[:, None]
    dp_h = ph1.reshape(B, K) - ph0[:, None]
    print(f"{name} {dtype}: max |dlogabs - logpsi difference| {(dl.reshape(B, K) - dl_h).abs().max().item():.3g}")
    assert torch.equal(dl.reshape(B, K), dl_h)
    assert torch.equal(dp.reshape(B, K), dp_h)


@pytest.mark.parametrize("name", POLARISED)
def test_diagonal_and_pair_shapes_follow_nspins(name):
    """aiqmc.observables._s2_diagonal is S_z (S_z + 1) + the minority count whichever channel is the
    minority, the pair outputs are [B, n_up, n_down] in that order, and the kernel's S2_L is that
    diagonal minus the sum of its own pair ratios: K + 1 additions and, per term, exp, cos / sin and
    two products, each within a few units of roundoff of the magnitudes summed."""
    from aiqmc import observables
    s, params, pos, _, _, _, _ = _case(name)
    nup, ndn = s.nspins
    assert nup != (s.nelectrons + 1) // 2
    sz = 0.5 * abs(nup - ndn)
    diag = observables._s2_diagonal((nup, ndn))
    assert diag == observables._s2_diagonal((ndn, nup)) == sz * (sz + 1.0) + min(nup, ndn)
    ctx = _ctx(s, params, torch.float64)
    s2, dl, dp = ctx.spin_squared(torch.tensor(pos, device="cuda"), want_pairs=True)
    torch.cuda.synchronize()
    assert dl.shape == (BMAX, nup, ndn) and dp.shape == (BMAX, nup, ndn)
    ratio = (torch.exp(dl) * torch.complex(torch.cos(dp), torch.sin(dp))).cpu().numpy()
    K = nup * ndn
    bound = (K + 9) * 2.0 ** -53 * (diag + np.abs(ratio).sum((1, 2)))
    assert np.all(np.abs(s2.cpu().numpy() - (diag - ratio.sum((1, 2)))) <= bound)


@pytest.mark.parametrize("name,B,chunk", [("H2", 8, 5), ("Z5", 7, 16), ("N2", 5, 100)])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_chunked_equals_unchunked_bitwise(dtype, name, B, chunk):
    """chunk / (K + 1) whole walkers per value launch: H2 (one pair) two walkers per chunk (4 chunks), (5,1)
    two per chunk with a partial last chunk, N2 two per chunk (3 chunks, the last partial)."""
    s, params, pos, _, _, _, _ = _case(name)
    ctx = _ctx(s, params, dtype)
    x = torch.tensor(pos[:B], device="cuda", dtype=dtype)
    K1 = s.nspins[0] * s.nspins[1] + 1
    assert B * K1 > chunk >= K1 and -(-B // (chunk // K1)) >= 2
    one = ctx.spin_squared(x, want_pairs=True)
    many = ctx.spin_squared(x, want_pairs=True, chunk=chunk)
    again = ctx.spin_squared(x, want_pairs=True)     # the default chunk is back
    torch.cuda.synchronize()
    for a, b, c in zip(one, many, again):
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("name", ["Be", "N2"])
def test_two_calls_give_identical_bits(name):
    s, params, pos, _, _, _, _ = _case(name)
    ctx = _ctx(s, params, torch.float32)
    x = torch.tensor(pos, device="cuda", dtype=torch.float32)
    a = ctx.spin_squared(x, want_pairs=True)
    b = ctx.spin_squared(x, want_pairs=True)
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_empty_batch_and_missing_params():
    s, params, pos, _, _, _, _ = _case("H2")
    from aiqmc import _lib
    ctx = _lib.Context.for_system(s, torch.float64)
    x = torch.tensor(pos, device="cuda")
    with pytest.raises(RuntimeError, match="set_params"):
        ctx.spin_squared(x)
    assert ctx.dipole(x).shape == (BMAX, 3)          # the dipole needs no parameters
    assert ctx.dipole(x[:0]).shape == (0, 3)
    # B == 0 returns OK and writes nothing (state is checked first, as in the neighbouring calls)
    assert _ctx(s, params, torch.float64).spin_squared(x[:0]).shape == (0,)


@pytest.mark.parametrize("name", ["H2", "Z5", "N2"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_dipole_matches_numpy(dtype, name):
    """mu = sum_a Z_a R_a - sum_i r_i.  The kernel adds the N coordinates in ascending order and
    subtracts the sum from the rounded nuclear term: N + 1 roundings of at most the unit roundoff
    each, relative to the sum of the magnitudes."""
    s, params, pos, _, _, _, _ = _case(name)
    ctx = _ctx(s, params, dtype)
    mu = ctx.dipole(torch.tensor(pos, device="cuda", dtype=dtype)).double().cpu().numpy()
    r = pos.reshape(BMAX, -1, 3)
    nuc = (s.charges[:, None] * s.atoms).sum(0)
    ref = nuc[None] - r.sum(1)
    u = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
    bound = (s.nelectrons + 2) * u * (np.abs(nuc)[None] + np.abs(r).sum(1))
    assert mu.shape == (BMAX, 3)
    assert np.all(np.abs(mu - ref) <= bound), np.abs(mu - ref).max()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_drop_in_estimators_equal_the_context_calls(dtype):
    from aiqmc import observables, systems
    from aiqmc.wavefunction_Ynlm import nn
    s = systems.make_system("Be")
    net = s.make_network()
    params = net.init(9)
    pos = torch.tensor(_case("Be")[2], dtype=dtype, device="cuda")
    data = nn.AINetData(positions=pos, spins=s.spins, atoms=s.atoms, charges=s.charges)
    est = observables.make_s2(net.apply, s.nspins)
    s2 = est(params, data)
    ctx = net.apply._aiqmc_network.bind(params, s.atoms, dtype)
    ref, dl, dp = ctx.spin_squared(pos, want_pairs=True)
    assert torch.equal(s2, ref) and s2.dtype == (torch.complex128 if dtype == torch.float64 else torch.complex64)
    r = est.pair_ratios(params, data)
    assert r.shape == (BMAX, 2, 2)
    assert torch.equal(r, torch.exp(dl) * torch.complex(torch.cos(dp), torch.sin(dp)))
    assert torch.equal(observables.make_dipole(net.apply)(params, data), ctx.dipole(pos))
    with pytest.raises(ValueError):
        observables.make_s2(net.apply, (3, 1))
    # one rank: the batch statistics are the plain mean and variance of the real part
    mean, var = observables.s2_stats(s2)
    re = s2.real.double().cpu().numpy()
    assert abs(float(mean) - re.mean()) <= 1e-12 * max(1.0, abs(re.mean()))
    assert abs(float(var) - re.var()) <= 1e-10 * max(1.0, re.var())


def _rank_s2(rank, world):
    """This rank's contiguous block of the 8 Be walkers through Context.spin_squared (fp64)."""
    s, params, pos, _, _, _, _ = _case("Be")
    n = BMAX // world
    ctx = _ctx(s, params, torch.float64)
    out = ctx.spin_squared(torch.tensor(pos[rank * n:(rank + 1) * n], device="cuda"))
    torch.cuda.synchronize()
    return out


_WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "ab-initio-flexible-gaussian-basis-neural-network-quantum-monte-carlo_amd"))
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch, torch.distributed as dist
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo")
import test_gpu_observables as T
from aiqmc import observables
s2 = T._rank_s2(rank, world)
mean_d, var_d = observables.s2_stats(s2)            # device statistics kernel + all-reduce
mean_h, var_h = observables.s2_stats(s2.cpu())      # host path
bm = observables.batch_mean(torch.view_as_real(s2.cpu()))   # constants.pmean of the rank mean [re, im]
np.savez(os.path.join(sys.argv[2], f"s2_{rank}.npz"), s2=s2.cpu().numpy(), mean_d=mean_d.cpu().numpy(),
         var_d=var_d.cpu().numpy(), mean_h=mean_h.numpy(), var_h=var_h.numpy(), bm=bm.numpy())
dist.barrier()
dist.destroy_process_group()
'''


def test_two_rank_pooled_mean_equals_one_process(tmp_path):
    """Two gloo ranks on the one test GPU (the pattern of tests/test_gpu_sharded.py), four Be walkers
    each: the pooled <S^2> and its variance equal the one-process values over all eight."""
    world = 2
    assert support.run_ranks(_WORKER, world, [ROOT, str(tmp_path)], timeout=240,
                             env={"HSA_ENABLE_IPC_MODE_LEGACY": "0"}) == [0] * world
    outs = [dict(np.load(tmp_path / f"s2_{r}.npz")) for r in range(world)]
    full = _rank_s2(0, 1).cpu().numpy()
    np.testing.assert_array_equal(np.concatenate([o["s2"] for o in outs]), full)
    mean, var = full.real.mean(), full.real.var()
    for o in outs:
        for k in ("mean_d", "mean_h"):
            assert abs(float(o[k]) - mean) <= 1e-12 * max(1.0, abs(mean)), k
        for k in ("var_d", "var_h"):
            assert abs(float(o[k]) - var) <= 1e-10 * max(1.0, var), k
        assert abs(complex(*o["bm"]) - full.mean()) <= 1e-12 * max(1.0, abs(full.mean()))
