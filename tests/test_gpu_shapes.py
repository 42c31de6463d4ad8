"""Every built (nelectrons, natoms) shape against the float64 oracle (VERDICT r4 missing #2: the
reference network is generic in nelectrons / natoms / nspins, nn.py:511-526).

The library instantiates its kernels for 2 <= N <= 16 (the Gauss-Jordan's 64-lane layout: 16
columns x 4 row groups) and A <= 3, plus (10, 4) and (10, 5): 46 shapes, odd N with unequal spin
channels included (alternating spins: N = 7 gives nspins (4, 3)).
Systems: "Z<N>" one atom of charge N, "Z<a>-<b>" a diatomic (a + b = N) at z = -1, +1, up to
five atoms off the axis (oracle/system.py).  Per shape, four walkers (two for N > 10: the oracle's Laplacian),
randomised auxiliary parameters:
  fp64: log|psi| (1e-10), grad log|psi| (1e-8), E_L (1e-6 Ha, the north-star bar), one
        host-draw Metropolis sweep (positions 1e-9), the parameter gradient (1e-8 of each
        walker's largest component);
  fp32: log|psi| and E_L against the same fp64 oracle (the reference's dtype, the parity
        suite's fp32 tolerances).
Outside the built set aiqmc_create refuses with AIQMC_EUNSUPPORTED and a message naming the
limit (N = 17; A = 6), an empty spin channel likewise; spin tables that are no permutation of the
electron slots and pair tables that contradict nspins are AIQMC_EINVAL.  Spin-polarised systems:
tests/test_gpu_spin_polarised.py."""
import numpy as np
import pytest
import torch

import support

pytestmark = pytest.mark.gpu

# the Makefile's SHAPES; a shape the loaded library does not list (a development build) is skipped
SHAPES = [(n, a) for a in (1, 2, 3) for n in range(max(2, a), 17)] + [(10, 4), (10, 5)]


def _oracle(n, a):
    """(system, params, pos, e_l, logabs, grad) of the fp64 oracle, cached per shape."""
    support.skip_unbuilt((n, a))
    return support.oracle_case(support.z_name(n, a), 100 + 3 * n + a, randomize_aux=True)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: f"N{sh[0]}A{sh[1]}")
def test_shape_fp64_matches_oracle(shape):
    s, params, pos, e_ref, l_ref, g_ref = _oracle(*shape)
    assert (s.nelectrons, s.natoms) == shape
    ctx = support.make_ctx(s, torch.float64, params)
    x = torch.tensor(pos, device="cuda")
    e, l, g = ctx.local_energy(x, want_logabs=True, want_grad=True)
    l2, g2 = ctx.logpsi_grad(x)
    torch.cuda.synchronize()
    np.testing.assert_allclose(l.cpu().numpy(), l_ref, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(l2.cpu().numpy(), l_ref, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(g.cpu().numpy(), g_ref, rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(g2.cpu().numpy(), g_ref, rtol=1e-8, atol=1e-8)
    assert np.max(np.abs(e.cpu().numpy() - e_ref)) <= 1e-6, (e.cpu().numpy(), e_ref)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: f"N{sh[0]}A{sh[1]}")
def test_shape_metropolis_and_param_grad_match_oracle(shape):
    from oracle import loss, mcstep, network
    s, params, pos, _, _, _ = _oracle(*shape)
    N, B = s.nelectrons, pos.shape[0]
    ctx = support.make_ctx(s, torch.float64, params)
    rng = np.random.default_rng(7 + N)
    g1 = torch.tensor(rng.standard_normal((1, B, 3 * N)))
    g2 = torch.tensor(rng.standard_normal((1, B, N, 3 * N)))
    u = torch.tensor(rng.uniform(size=(1, B, N)))
    ref = mcstep.mc_step(network.Network(s), network.to_torch(params), torch.tensor(pos), g1, g2, u, 0.05, 1)
    idx = torch.arange(N)
    x = torch.tensor(pos, device="cuda").contiguous()
    ctx.mc_step(x, 1, 0.05, gauss1=g1, gauss2=g2.reshape(1, B, N, N, 3)[:, :, idx, idx, :].contiguous(), u=u)
    torch.cuda.synchronize()
    np.testing.assert_allclose(x.cpu().numpy(), ref.numpy(), rtol=1e-9, atol=1e-9)
    O = ctx.logpsi_param_grad(torch.tensor(pos, device="cuda")).cpu().numpy()
    O_ref = loss.logabs_param_grad(network.Network(s), params, torch.tensor(pos))
    assert O.shape == O_ref.shape
    err = np.abs(O - O_ref) / (np.abs(O_ref).max(axis=1, keepdims=True) + 1e-3)
    assert err.max() < 1e-8, (err.max(), np.unravel_index(err.argmax(), err.shape))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: f"N{sh[0]}A{sh[1]}")
def test_shape_fp32_matches_oracle(shape):
    s, params, pos, e_ref, l_ref, _ = _oracle(*shape)
    ctx = support.make_ctx(s, torch.float32, params)
    x = torch.tensor(pos, device="cuda").float().contiguous()
    e, l, _ = ctx.local_energy(x, want_logabs=True, want_grad=True)
    torch.cuda.synchronize()
    np.testing.assert_allclose(l.double().cpu().numpy(), l_ref, rtol=1e-5, atol=2e-4)
    np.testing.assert_allclose(e.double().cpu().numpy(), e_ref, rtol=2e-4, atol=2e-3)


@pytest.mark.parametrize("n,a,what", [(17, 1, "nelectrons"), (18, 2, "nelectrons"), (10, 6, "no kernel instantiation")])
def test_shape_outside_the_built_set_is_refused(n, a, what):
    from aiqmc import _lib
    atoms = np.zeros((a, 3))
    atoms[:, 2] = np.arange(a)
    charges = np.full(a, float(n) / a)
    spins = np.array([1.0 if i % 2 == 0 else -1.0 for i in range(n)])
    from oracle import system
    par, anti, _, _ = system.jastrow_indices_ee(spins, n)
    up, dn = system.spin_indices_h(spins)
    with pytest.raises(Exception) as ei:
        _lib.Context(n, a, (len(up), len(dn)), atoms, charges, up, dn, par, anti, dtype=torch.float64, device=0)
    assert what in str(ei.value)


@pytest.mark.parametrize("nspins,up,dn,pair_spins,code,what", [
    ((2, 2), [0, 0], [1, 3], "udud", -1, "permutation of 0..N-1: electron 2 is in neither"),          # a slot twice
    ((2, 2), [0, 2], [2, 3], "udud", -1, "electron 2 is in spin_up_indices and in spin_down_indices"),
    ((1, 3), [1], [0, 3, 3], "dudd", -1, "electron 2 is in neither"),
    ((2, 2), [0, 2], [1, 3], "uuud", -1, "n_antiparallel = 3 contradicts the spin tables: nspins[0] * nspins[1] = 4"),
    ((3, 1), [0, 1, 2], [3], "udud", -1, "n_antiparallel = 4 contradicts"),
    ((4, 0), [0, 1, 2, 3], [], "uuuu", -2, "both spin channels must be occupied"),
    ((0, 4), [], [0, 1, 2, 3], "dddd", -2, "both spin channels must be occupied"),
], ids=["repeated_up", "up_and_down", "repeated_down", "anti_too_few", "anti_too_many", "no_down", "no_up"])
def test_inconsistent_spin_tables_are_refused(nspins, up, dn, pair_spins, code, what):
    """aiqmc_create on four electrons: spin tables that are no permutation of 0..N-1 (a repeated
    slot is a repeated determinant row) and pair tables that contradict nspins are AIQMC_EINVAL (-1)
    with a message naming the offender; an empty spin channel is AIQMC_EUNSUPPORTED (-2)."""
    from aiqmc import _lib
    from oracle import system
    spins = np.array([1.0 if ch == "u" else -1.0 for ch in pair_spins])
    par, anti, _, _ = system.jastrow_indices_ee(spins, 4)
    with pytest.raises(RuntimeError) as ei:
        _lib.Context(4, 1, nspins, np.zeros((1, 3)), np.array([4.0]), np.array(up, dtype=np.int32),
                     np.array(dn, dtype=np.int32), par, anti, dtype=torch.float64, device=0)
    assert what in str(ei.value) and f"({code})" in str(ei.value), str(ei.value)
    # and the consistent tables of the same spins are accepted
    s = system.make_system("Z4@" + ("uuud" if pair_spins in ("uuuu", "dddd") else pair_spins))
    assert _lib.Context.for_system(s, torch.float64).nparams > 0


@pytest.mark.parametrize("shape", [(7, 1), (5, 3), (13, 3), (16, 3), (10, 5)], ids=lambda sh: f"N{sh[0]}A{sh[1]}")
def test_shape_fp32_sweeps_follow_fp64(shape):
    """Three fp32 Metropolis sweeps (the reference's dtype; packed N <= 8 kernels or the one-wave
    proposal path) against fp64 sweeps from the same float-rounded walkers and host draws: at most
    one acceptance decision in 100 flips, and the walkers that took the same decisions agree to
    fp32 rounding."""
    n, a = shape
    support.skip_unbuilt(shape)
    B, NS = 64, 3
    s, params, pos = support.seeded_case(support.z_name(n, a), 5 + n, B, randomize_aux=True)
    pos = pos.astype(np.float32).astype(np.float64)
    g = torch.Generator().manual_seed(n + 10 * a)
    kw = dict(gauss1=torch.randn(NS, B, 3 * n, generator=g, dtype=torch.float64),
              gauss2=torch.randn(NS, B, n, 3, generator=g, dtype=torch.float64),
              u=torch.rand(NS, B, n, generator=g, dtype=torch.float64))
    c64, c32 = support.make_ctx(s, torch.float64, params), support.make_ctx(s, torch.float32, params)
    x64 = torch.tensor(pos, device="cuda").contiguous()
    x32 = x64.float().contiguous()
    a64 = c64.mc_step(x64, NS, 0.05, count_accepts=True, **kw)
    a32 = c32.mc_step(x32, NS, 0.05, count_accepts=True, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(x32).all()
    n64, n32 = int(a64.sum()), int(a32.sum())
    assert n64 > B * n * NS // 4, n64
    assert abs(n32 - n64) <= max(1, B * n * NS // 100), (n32, n64)
    dw = (x32.double() - x64).abs().reshape(B, -1).amax(1)
    same = dw < 1e-3
    assert int((~same).sum()) <= max(1, B // 20), dw.topk(4)
    assert float(dw[same].max()) < 1e-4, float(dw[same].max())


@pytest.mark.parametrize("shape,B", [((4, 1), 5), ((2, 2), 5), ((3, 1), 7), ((6, 1), 3), ((8, 2), 3), ((7, 2), 5)],
                         ids=lambda v: str(v))
def test_param_grad_partial_last_wave(shape, B):
    """k_param_grad packs K walkers per wave (K = 4 for N <= 4, 2 for N <= 8): B not a multiple of
    K leaves the last wave partial (nk < K: the per-walker Gauss-Jordan skip, the zeroed reduction
    slots, the output loops).  Per-walker rows and weighted sums of d log|psi| and d phase, fp64
    vs the oracle and fp32 vs fp64, on such batches."""
    from oracle import loss, network, system
    n, a = shape
    support.skip_unbuilt(shape)
    s = system.make_system(support.z_name(n, a))
    rng = np.random.default_rng(40 + n + a)
    params = system.init_params(rng, s, randomize_aux=True)
    pos = system.init_electrons(rng, s.atoms, s.charges, B, 1.0)
    net = network.Network(s)
    O_ref = loss.logabs_param_grad(net, params, torch.tensor(pos))
    P_ref = loss.phase_param_grad(net, params, torch.tensor(pos))
    w = rng.normal(size=B)
    c64, c32 = support.make_ctx(s, torch.float64, params), support.make_ctx(s, torch.float32, params)
    x = torch.tensor(pos, device="cuda")
    for ref, fn in ((O_ref, "logpsi_param_grad"), (P_ref, "phase_param_grad")):
        rows = getattr(c64, fn)(x).cpu().numpy()
        ws = getattr(c64, fn)(x, weights=torch.tensor(w, device="cuda")).cpu().numpy()
        scale = np.abs(ref).max(axis=1, keepdims=True) + 1e-3
        assert (np.abs(rows - ref) / scale).max() < 1e-8, fn
        np.testing.assert_allclose(ws, w @ ref, rtol=0, atol=1e-8 * np.abs(w @ ref).max())
        r32 = getattr(c32, fn)(x.float().contiguous()).double().cpu().numpy()
        assert (np.abs(r32 - ref) / scale).max() < 5e-3, fn
        # the weighted multi-row entry (one gradient pass, two weight rows)
        W = torch.tensor(np.stack([w, np.ones(B)]), device="cuda")
        two = c64.param_grad_weighted(x, W, phase=fn.startswith("phase")).cpu().numpy()
        np.testing.assert_allclose(two[0], ws, rtol=1e-13, atol=1e-13 * np.abs(ws).max())
        np.testing.assert_allclose(two[1], ref.sum(0), rtol=0, atol=1e-8 * np.abs(ref.sum(0)).max())


@pytest.mark.parametrize("shape", [(7, 1), (9, 2), (13, 3), (16, 3), (10, 4), (10, 5)], ids=lambda sh: f"N{sh[0]}A{sh[1]}")
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_set_params_device_equals_host_upload_shapes(shape, dtype):
    """aiqmc_set_params_device on the round-5 shapes (odd N, A = 3..5 with their wider F4/B2 and
    conv-bias records): log|psi|, its gradient, E_L and the parameter gradient bitwise equal to the
    host upload."""
    from oracle import system
    n, a = shape
    support.skip_unbuilt(shape)
    s = system.make_system(support.z_name(n, a))
    rng = np.random.default_rng(60 + n + a)
    params = system.init_params(rng, s, randomize_aux=True)
    flat = system.flatten_params(params)
    pos = torch.tensor(system.init_electrons(rng, s.atoms, s.charges, 8, 1.0), device="cuda", dtype=dtype)
    outs = []
    for mode in ("host", "device"):
        ctx = support.make_ctx(s, dtype, params)
        if mode == "device":   # over a different host upload, so a no-op device repack would fail
            ctx.set_params(0.5 * flat)
            ctx.set_params_device(torch.tensor(flat, dtype=torch.float64, device="cuda"))
        la, g = ctx.logpsi_grad(pos)
        e, _, _ = ctx.local_energy(pos)
        pg = ctx.logpsi_param_grad(pos)
        torch.cuda.synchronize()
        outs.append([t.cpu() for t in (la, g, e, pg)])
    for x_, y_ in zip(*outs):
        assert torch.equal(x_, y_)
