"""Full-size (4096-walker N2) GPU checks through size-independent properties.

The oracle is too slow for 4096 walkers, so at the benchmark size we check:
  * reverse-mode gradient kernel == forward-mode gradient kernel (two
    independent derivative implementations) on every walker;
  * the gradient returned by the Laplacian kernel == both of them;
  * float32 kernels == float64 kernels (relative, on identical walkers);
  * log|psi| from all four kernels agree;
  * Metropolis with on-device Philox draws: finite, deterministic per
    (seed, offset), acceptance rate in (0, 1).
"""
import numpy as np
import pytest
import torch

import support

pytestmark = pytest.mark.gpu


def _ctx(name, dtype, params_seed=5):
    from oracle import system
    s = system.make_system(name)
    return s, support.make_ctx(s, dtype, system.init_params(np.random.default_rng(params_seed), s, randomize_aux=True))


def _walkers(s, B, seed=0):
    from oracle import system
    return system.init_electrons(np.random.default_rng(seed), s.atoms, s.charges, B, 1.0)


@pytest.mark.parametrize("name", ["N2", "Ne"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_reverse_vs_forward_gradient_4096(dtype, name):
    s, ctx = _ctx(name, dtype)
    pos = torch.tensor(_walkers(s, 4096), dtype=dtype, device="cuda")
    la_r, g_r = ctx.logpsi_grad(pos)
    la_f, g_f = ctx.logpsi_grad_forward_mode(pos)
    el, la_l, g_l = ctx.local_energy(pos, want_logabs=True, want_grad=True)
    torch.cuda.synchronize()
    # fp32: two different fp32 algorithms (forward vs reverse mode) disagree most on the few
    # walkers with a nearly singular orbital matrix; bound the worst case loosely (5e-3 of the
    # walker's largest gradient component) and the typical case tightly (median 1e-5)
    tol = 1e-9 if dtype == torch.float64 else 5e-3
    scale = g_f.abs().amax(dim=1, keepdim=True) + 1.0
    rel = (g_r - g_f).abs() / scale
    assert torch.all(rel <= tol), float(rel.max())
    if dtype == torch.float32:
        assert float(rel.median()) < 1e-5, float(rel.median())
    assert torch.all((g_l - g_f).abs() <= tol * scale)
    lt = 1e-10 if dtype == torch.float64 else 1e-4
    assert torch.allclose(la_r, la_f, rtol=lt, atol=lt)
    assert torch.allclose(la_l, la_f, rtol=lt, atol=lt)
    assert torch.isfinite(el).all()


def test_float32_matches_float64_4096():
    s, c64 = _ctx("N2", torch.float64)
    _, c32 = _ctx("N2", torch.float32)
    x = _walkers(s, 4096, seed=3)
    e64, l64, g64 = c64.local_energy(torch.tensor(x, device="cuda"), want_logabs=True, want_grad=True)
    e32, l32, g32 = c32.local_energy(torch.tensor(x, dtype=torch.float32, device="cuda"), want_logabs=True,
                                     want_grad=True)
    torch.cuda.synchronize()
    l64, l32 = l64.cpu().numpy(), l32.double().cpu().numpy()
    np.testing.assert_allclose(l32, l64, rtol=1e-4, atol=1e-3)
    e64, e32 = e64.cpu().numpy(), e32.double().cpu().numpy()
    rel = np.abs(e32 - e64) / (np.abs(e64) + 1.0)
    print("fp32 vs fp64 E_L, relative: median", np.median(rel), "p99", np.quantile(rel, 0.99),
          "p99.9", np.quantile(rel, 0.999), "max", rel.max(), "frac > 1e-3", np.mean(rel > 1e-3))
    # the fp32 oracle on 1,024 N2 walkers (tests/golden/N2_fp32.npz): median 7.9e-7, p99 9.3e-5,
    # 0.1 % of walkers above 1e-3, none above 1e-2.  Measured here: median 1.5e-6, p99 2.0e-4,
    # p99.9 1.0e-3, max 5.3e-3
    assert np.median(rel) < 1e-5, np.median(rel)
    assert np.quantile(rel, 0.99) < 1e-3, np.quantile(rel, 0.99)
    assert rel.max() < 2e-2, rel.max()


@pytest.mark.parametrize("name", ["N2", "Ne"])
def test_philox_mc_is_deterministic_and_sane(name):
    s, ctx = _ctx(name, torch.float32)
    N = s.nelectrons
    x0 = torch.tensor(_walkers(s, 4096, seed=4), dtype=torch.float32, device="cuda")
    a = x0.clone().contiguous()
    b = x0.clone().contiguous()
    acc_a = ctx.mc_step(a, 3, 0.05, seed=7, offset=11, count_accepts=True)
    ctx.mc_step(b, 3, 0.05, seed=7, offset=11)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.isfinite(a).all()
    moved = (a - x0).abs().reshape(4096, N, 3).amax(-1) > 0
    rate = float(acc_a.sum()) / (4096 * N * 3)
    assert 0.05 < rate < 1.0, rate
    assert 0.05 < float(moved.float().mean()) <= 1.0
    c = x0.clone().contiguous()
    ctx.mc_step(c, 3, 0.05, seed=8, offset=11)
    assert not torch.equal(a, c)


@pytest.mark.parametrize("B", [0, 1, 3, 65, 1000])
def test_ragged_batches_match_full_batch(B):
    s, ctx = _ctx("N2", torch.float64)
    x = torch.tensor(_walkers(s, 1000, seed=6), device="cuda")
    e_full, l_full, g_full = ctx.local_energy(x, want_logabs=True, want_grad=True)
    e, l, g = ctx.local_energy(x[:B], want_logabs=True, want_grad=True)
    la, gr = ctx.logpsi_grad(x[:B])
    torch.cuda.synchronize()
    assert e.shape == (B,)
    if B:
        assert torch.equal(e, e_full[:B]) and torch.equal(l, l_full[:B]) and torch.equal(g, g_full[:B])
        assert torch.allclose(gr, g_full[:B], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("name", ["H2", "Be", "C", "Ne", "C2", "C2_ecp", "O2"])
def test_other_shapes_reverse_vs_forward(name):
    s, ctx = _ctx(name, torch.float64)
    pos = torch.tensor(_walkers(s, 256), device="cuda")
    la_r, g_r = ctx.logpsi_grad(pos)
    la_f, g_f = ctx.logpsi_grad_forward_mode(pos)
    torch.cuda.synchronize()
    assert torch.allclose(g_r, g_f, rtol=1e-8, atol=1e-8)
    assert torch.allclose(la_r, la_f, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("name", ["H2", "Be", "C", "Ne", "C2", "C2_ecp", "N2", "O2"])
def test_proposal_reuse_matches_recompute(name):
    """Proposals from the walker cache (moved electron + its 2(N-1) pairs recomputed)
    == proposals evaluated from scratch, on the same Philox draws."""
    s, ctx = _ctx(name, torch.float64)
    x0 = torch.tensor(_walkers(s, 512, seed=9), device="cuda")
    a = x0.clone().contiguous()
    b = x0.clone().contiguous()
    ctx.set_proposal_reuse(True)
    acc_a = ctx.mc_step(a, 4, 0.05, seed=3, offset=5, count_accepts=True)
    ctx.set_proposal_reuse(False)
    acc_b = ctx.mc_step(b, 4, 0.05, seed=3, offset=5, count_accepts=True)
    ctx.set_proposal_reuse(True)
    torch.cuda.synchronize()
    assert torch.equal(acc_a, acc_b)
    assert torch.allclose(a, b, rtol=0, atol=1e-11), float((a - b).abs().max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("draws", ["philox", "host"])
def test_fused_acceptance_is_bitwise_identical(dtype, draws):
    """mc_step applies each sweep's acceptance inside the next sweep's walker launch (the last
    sweep keeps its own launch); the separate-launch path must give the same bits: positions
    and accepted-move counts."""
    s, ctx = _ctx("N2", dtype)
    B, NS, N = 4096, 4, s.nelectrons
    x0 = torch.tensor(_walkers(s, B, seed=12), dtype=dtype, device="cuda")
    kw = dict(seed=2, offset=3)
    if draws == "host":
        g = torch.Generator().manual_seed(0)
        kw = dict(gauss1=torch.randn(NS, B, 3 * N, generator=g, dtype=torch.float64),
                  gauss2=torch.randn(NS, B, N, 3, generator=g, dtype=torch.float64),
                  u=torch.rand(NS, B, N, generator=g, dtype=torch.float64))
    a = x0.clone().contiguous()
    b = x0.clone().contiguous()
    acc_a = ctx.mc_step(a, NS, 0.05, count_accepts=True, **kw)
    ctx.set_fuse_accept(False)
    acc_b = ctx.mc_step(b, NS, 0.05, count_accepts=True, **kw)
    ctx.set_fuse_accept(True)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(acc_a, acc_b)
    assert int(acc_a.sum()) > 0 and not torch.equal(a, x0)


@pytest.mark.parametrize("name,dtype,B,NS", [("N2", torch.float64, 4096, 6), ("C", torch.float64, 4096, 6),
                                             ("N2", torch.float32, 4096, 6),
                                             # a long mc_step (burn-in runs 50+ sweeps): the re-used
                                             # order is checked against the pivots partial pivoting
                                             # chose (the anchor), not the previous sweep's
                                             ("N2", torch.float64, 1024, 50), ("C", torch.float64, 1024, 50),
                                             ("N2", torch.float32, 1024, 50)])
def test_walker_pivot_reuse_matches_partial_pivoting(name, dtype, B, NS):
    """From an mc_step's second sweep on, the walker launch eliminates in its previous sweep's
    pivot order (partial pivoting only when a pivot shrinks below 0.1 of the previous one) and
    refreshes the pivot record its proposals are relative to.  Against partial pivoting in every
    sweep (aiqmc_debug_set_walker_pivots(0)), six host-draw sweeps: fp64 positions to 1e-10 with
    equal accept counts; fp32 positions to 1e-5 except where rounding flips a near-tie acceptance."""
    s, ctx = _ctx(name, dtype)
    N = s.nelectrons
    x0 = torch.tensor(_walkers(s, B, seed=21), dtype=dtype, device="cuda")
    g = torch.Generator().manual_seed(5)
    kw = dict(gauss1=torch.randn(NS, B, 3 * N, generator=g, dtype=torch.float64),
              gauss2=torch.randn(NS, B, N, 3, generator=g, dtype=torch.float64),
              u=torch.rand(NS, B, N, generator=g, dtype=torch.float64))
    a = x0.clone().contiguous()
    b = x0.clone().contiguous()
    acc_a = ctx.mc_step(a, NS, 0.05, count_accepts=True, **kw)
    ctx.set_walker_pivots(False)
    acc_b = ctx.mc_step(b, NS, 0.05, count_accepts=True, **kw)
    ctx.set_walker_pivots(True)
    torch.cuda.synchronize()
    assert int(acc_a.sum()) > 0 and not torch.equal(a, x0)
    dw = (a - b).abs().reshape(B, -1).amax(1)
    if dtype == torch.float64:
        assert float(dw.max()) < 1e-10, float(dw.max())
        assert torch.equal(acc_a, acc_b)
    else:
        flipped = dw > 1e-4
        # a walker whose near-tie acceptance flipped follows its own chain from then on
        assert float(flipped.float().mean()) < 2e-3 * max(1, NS // 6), float(flipped.float().mean())
        # rounding differences of two elimination orders drift the chains apart slowly
        assert float(dw[~flipped].max()) < 1e-5 * max(1, NS // 12), float(dw[~flipped].max())


def test_proposal_reuse_matches_recompute_f32_4096():
    s, ctx = _ctx("N2", torch.float32)
    x0 = torch.tensor(_walkers(s, 4096, seed=10), dtype=torch.float32, device="cuda")
    a = x0.clone().contiguous()
    b = x0.clone().contiguous()
    ctx.mc_step(a, 2, 0.05, seed=1, offset=0)
    ctx.set_proposal_reuse(False)
    ctx.mc_step(b, 2, 0.05, seed=1, offset=0)
    ctx.set_proposal_reuse(True)
    torch.cuda.synchronize()
    # fp32 rounding may flip an acceptance whose ratio sits within ~1e-6 of its uniform
    differ = ((a - b).abs().reshape(4096, -1).amax(1) > 1e-4).float().mean()
    assert float(differ) < 2e-3, float(differ)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_local_energy_adjoint_vs_forward_laplacian_4096(dtype):
    """Production local energy (adjoint pass + first-derivative pass) == the single-launch
    forward-Laplacian kernel (second-order jets through the whole network) on every walker."""
    s, ctx = _ctx("N2", dtype)
    pos = torch.tensor(_walkers(s, 4096, seed=12), dtype=dtype, device="cuda")
    e1, l1, g1 = ctx.local_energy(pos, want_logabs=True, want_grad=True)
    e0, l0, g0 = ctx.local_energy_forward_mode(pos, want_logabs=True, want_grad=True)
    torch.cuda.synchronize()
    e1, e0 = e1.double().cpu().numpy(), e0.double().cpu().numpy()
    rel = np.abs(e1 - e0) / (np.abs(e0) + 1.0)
    scale = g0.abs().amax(dim=1, keepdim=True) + 1.0
    if dtype == torch.float64:
        assert rel.max() < 1e-8, rel.max()
        assert torch.all((g1 - g0).abs() <= 1e-9 * scale)
        assert torch.allclose(l1, l0, rtol=1e-10, atol=1e-10)
    else:
        assert np.median(rel) < 1e-5, np.median(rel)
        assert np.mean(rel < 1e-3) > 0.99
        assert torch.all((g1 - g0).abs() <= 2e-3 * scale)


@pytest.mark.parametrize("name", ["H2", "Be", "C", "Ne", "C2", "O2", "N2"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_multiwave_local_energy_matches_single_wave(name, dtype):
    """The first-derivative pass split over 2 or 4 waves per walker (small per-GPU batches) ==
    one wave per walker: same E_L and gradient to rounding (only the summation order of the
    per-wave partial sums differs)."""
    s, ctx = _ctx(name, dtype)
    pos = torch.tensor(_walkers(s, 512, seed=14), dtype=dtype, device="cuda")
    out = {}
    for w in (1, 2, 4, 0):
        ctx.set_lap_waves(w)
        out[w] = ctx.local_energy(pos, want_logabs=True, want_grad=True)
    ctx.set_lap_waves(0)
    torch.cuda.synchronize()
    e1, l1, g1 = out[1]
    tol = 1e-10 if dtype == torch.float64 else 2e-4
    for w in (2, 4, 0):
        e, l, g = out[w]
        assert torch.equal(l, l1)                      # log|psi| comes from the (unsplit) adjoint pass
        assert torch.allclose(e, e1, rtol=tol, atol=tol * 10), (w, float((e - e1).abs().max()))
        assert torch.allclose(g, g1, rtol=tol, atol=tol * 10), (w, float((g - g1).abs().max()))
    assert torch.equal(out[0][0], out[4][0])           # 512 walkers: the default splits 4 ways


@pytest.mark.parametrize("name", ["H2", "Be", "C", "Ne", "C2", "C2_ecp", "O2"])
def test_other_shapes_local_energy_adjoint_vs_forward(name):
    s, ctx = _ctx(name, torch.float64)
    pos = torch.tensor(_walkers(s, 256, seed=13), device="cuda")
    e1, _, g1 = ctx.local_energy(pos, want_grad=True)
    e0, _, g0 = ctx.local_energy_forward_mode(pos, want_grad=True)
    torch.cuda.synchronize()
    assert torch.allclose(e1, e0, rtol=1e-9, atol=1e-8), float((e1 - e0).abs().max())
    assert torch.allclose(g1, g0, rtol=1e-8, atol=1e-8)


@pytest.mark.parametrize("name", ["Be", "H2", "C", "C2_ecp"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_small_n_packed_proposals_match_one_wave_path(name, dtype):
    """N <= 4: the Metropolis proposals run four configurations per wave (quad_small.h
    k_quad_grad); 5 <= N <= 8 (the all-electron C atom, C2 with ccECP -- the reference's example/C2): two
    per wave in 32-lane slots (round 4).  With the walker cache off every proposal goes through
    k_walker_rev's general path instead.  Same host draws -> same trajectory (fp64: to 1e-10,
    identical accept counts; fp32: all but rounding-level acceptance flips)."""
    s, ctx = _ctx(name, dtype)
    B, NS, N = 1001, 3, s.nelectrons    # odd B: the last wave of the walker launch (and of H2's proposals) is partial
    x0 = torch.tensor(_walkers(s, B, seed=4), dtype=dtype, device="cuda")
    g = torch.Generator().manual_seed(1)
    kw = dict(gauss1=torch.randn(NS, B, 3 * N, generator=g, dtype=torch.float64),
              gauss2=torch.randn(NS, B, N, 3, generator=g, dtype=torch.float64),
              u=torch.rand(NS, B, N, generator=g, dtype=torch.float64))
    a = x0.clone().contiguous()
    b = x0.clone().contiguous()
    acc_a = ctx.mc_step(a, NS, 0.05, count_accepts=True, **kw)
    ctx.set_proposal_reuse(False)
    acc_b = ctx.mc_step(b, NS, 0.05, count_accepts=True, **kw)
    ctx.set_proposal_reuse(True)
    torch.cuda.synchronize()
    assert int(acc_a.sum()) > 0
    if dtype == torch.float64:
        assert torch.allclose(a, b, rtol=0, atol=1e-10), float((a - b).abs().max())
        assert torch.equal(acc_a, acc_b)
    else:
        differ = ((a - b).abs().reshape(B, -1).amax(1) > 1e-4).float().mean()
        assert float(differ) < 5e-3, float(differ)


@pytest.mark.parametrize("name", ["Be", "H2", "C", "C2_ecp"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_small_n_packed_walkers_match_one_wave_path(name, dtype):
    """N <= 8: the walker launches of a sweep (value, gradient, the walker cache the proposals read,
    the fused acceptance) run several walkers per wave (quad_small.h k_quad_grad<WALK>: four for
    N <= 4, two in 32-lane slots for 5 <= N <= 8, round 4) against one wave per walker
    (k_walker_rev, aiqmc_debug_set_packed_walkers(0)).  Same host draws -> same trajectory (fp64:
    to 1e-10, identical accept counts; fp32: all but rounding-level acceptance flips)."""
    s, ctx = _ctx(name, dtype)
    B, NS, N = 1001, 4, s.nelectrons    # odd B: the last wave of the walker launch is partial
    x0 = torch.tensor(_walkers(s, B, seed=8), dtype=dtype, device="cuda")
    g = torch.Generator().manual_seed(2)
    kw = dict(gauss1=torch.randn(NS, B, 3 * N, generator=g, dtype=torch.float64),
              gauss2=torch.randn(NS, B, N, 3, generator=g, dtype=torch.float64),
              u=torch.rand(NS, B, N, generator=g, dtype=torch.float64))
    a = x0.clone().contiguous()
    b = x0.clone().contiguous()
    acc_a = ctx.mc_step(a, NS, 0.05, count_accepts=True, **kw)
    ctx.set_packed_walkers(False)
    acc_b = ctx.mc_step(b, NS, 0.05, count_accepts=True, **kw)
    ctx.set_packed_walkers(True)
    torch.cuda.synchronize()
    assert int(acc_a.sum()) > 0 and not torch.equal(a, x0)
    if dtype == torch.float64:
        assert torch.allclose(a, b, rtol=0, atol=1e-10), float((a - b).abs().max())
        assert torch.equal(acc_a, acc_b)
    else:
        differ = ((a - b).abs().reshape(B, -1).amax(1) > 1e-4).float().mean()
        assert float(differ) < 5e-3, float(differ)


@pytest.mark.parametrize("name", ["N2", "Be"])
def test_fused_limdrift_reduction_matches_reduction_launches(name):
    """fp32 mc_step sums the two limdrift reductions of a sweep (VMCmcstep.py:11-14) inside the
    walker and proposal launches as exact integer accumulations (kargs.h TACC_SCALE, limdrift.h)
    instead of two reduction launches.  The integer sum is order independent: repeated runs are
    bitwise equal, and so is the unfused path, whose reduction launches (k_taueff_part) sum the
    same integers.  Against the fp64 tree-sum launch (k_taueff, mode 3) the limdrift factor
    differs only in the float rounding of v2, so the positions agree to rounding, with at most a
    rare acceptance flip (a ratio within ~1e-6 of its uniform).  Be runs the
    4-configurations-per-wave proposal kernel (quad_small.h), N2 k_walker_rev."""
    s, ctx = _ctx(name, torch.float32)
    B, NS, N = 4096, 4, s.nelectrons
    x0 = torch.tensor(_walkers(s, B, seed=21), dtype=torch.float32, device="cuda")
    g = torch.Generator().manual_seed(1)
    kw = dict(gauss1=torch.randn(NS, B, 3 * N, generator=g, dtype=torch.float64),
              gauss2=torch.randn(NS, B, N, 3, generator=g, dtype=torch.float64),
              u=torch.rand(NS, B, N, generator=g, dtype=torch.float64))
    a, a2, w, b = (x0.clone().contiguous() for _ in range(4))
    ctx.set_fuse_reduce(2)          # fused (the default at every batch size since round 4)
    acc_a = ctx.mc_step(a, NS, 0.05, count_accepts=True, **kw)
    ctx.mc_step(a2, NS, 0.05, **kw)
    ctx.set_fuse_reduce(0)          # integer reduction launches
    ctx.mc_step(w, NS, 0.05, **kw)
    ctx.set_fuse_reduce(3)          # fp64 tree-sum launch
    acc_b = ctx.mc_step(b, NS, 0.05, count_accepts=True, **kw)
    ctx.set_fuse_reduce(1)
    torch.cuda.synchronize()
    assert torch.equal(a, a2)
    assert torch.equal(a, w)
    d = (a - b).abs().reshape(B, -1).amax(1)
    flips = int((acc_a != acc_b).sum())
    assert flips <= B // 200, flips
    same = acc_a == acc_b
    assert float(d[same].max()) < 1e-4, float(d[same].max())
    assert int(acc_a.sum()) > 0 and not torch.equal(a, x0)
