"""The phases every proposal repeats, after their instruction trim (gj.h: gj_fixed_regs parks its
pivots by v_writelane and forms the row update from one multiplier pair with v_pk_fma_f32's
op_sel / neg modifiers in fp32; walker_rev.h: k_moved_electron reads the Yt weights row by row).

The library hands out no proposal's log|psi|, gradient or sum |grad|^2 and no ECache record.  What
they decide is a sweep's acceptances: the ratio is formed from the proposal's log|psi| and its own
gradient under the limdrift sum, and an accepted position is the walker launch's x + g.  So every
check is a sweep whose decisions are pinned: the draws are chosen on the fp64 oracle so that no
acceptance ratio lies within MARGIN (relative) of its uniform.  fp32 rounding moves a ratio by
~1e-4 of itself at most (test_gpu_b3_handover.py); MARGIN is ten times that, so a flipped
acceptance is a defect in either precision and the accept counts are asserted equal to the
oracle's.  Once the decisions agree the positions do, so log|psi|, the gradient and sum |grad|^2
at the new positions are asserted as well, but it is the decisions that see the proposal kernels.

  1. cached proposals against from-scratch proposals (set_proposal_reuse(False): no ECache, no
     fixed-order elimination, B3 recomputes every pair), 8 walkers, seeded Philox draws (the seed
     is the first whose draws, read back from the device, keep MARGIN on the oracle).
     Tolerances of test_gpu_b3_handover.py: fp64 1e-11; fp32 no walker further than 1e-4 apart.
     fp32 values at the new positions: the parity suite's fp32 bounds (log|psi| rtol 1e-5, atol
     2e-4, test_gpu_shapes.py; gradient rtol 1e-3, atol 1e-3, test_gpu_fp32_pivot_range.py) and
     for s2 = sum g^2 what the gradient bound implies, |ds2| <= sum 2 |g| |dg| + |dg|^2.
  2. the same shapes, 3 walkers, host draws, against the fp64 oracle's sweep at test_gpu_shapes.py's
     tolerance (positions 1e-9), the accepted moves being exactly the oracle's; then log|psi| (1e-10)
     and the gradient (1e-8) at the new positions against the oracle.
  3. 3 walkers leave k_moved_electron's last wave partial (N2: 42 records = 16 + 16 + 10; (5, 1):
     15): its records (Yt row, derivative rows, h0 / hd, J_ae, position) through their only
     readers, the proposal kernels, against proposals that evaluate the moved electron's stage
     from scratch; fp32 moves exactly the oracle's electrons.
  4. RW = 2: in one process the proposals of N <= 8 take the packed route (k_quad_grad; the switch
     to k_walker_rev<PROP> is read from the environment once per process), so (5, 1) reaches the
     fixed-order elimination through the walker launch instead: with set_packed_walkers(False)
     the second sweep of an mc_step runs gj_fixed_regs on the order its first sweep recorded
     (k_walker_rev, rows 7 / 6 asserted with launch_row).  Two host-draw sweeps of (5, 1) (odd N,
     unequal spin channels) and (8, 2) (both row groups full) against the oracle's two sweeps.

Shapes of 1-2: (14, 2) the benchmark's; (13, 2) and (16, 3) the edges of the MFMA-Phi and RW = 4
register layout; (12, 2) RW = 3 with the last row group full; (5, 1), which there runs
k_moved_electron and the packed proposals.
"""
import functools

import numpy as np
import pytest
import torch

import support

pytestmark = pytest.mark.gpu

SHAPES = [(14, 2), (13, 2), (16, 3), (12, 2), (5, 1)]
MARGIN = 1e-3   # relative gap of every oracle acceptance ratio to its uniform (10x fp32's ~1e-4)
TSTEP = 0.05
_ids = lambda sh: f"N{sh[0]}A{sh[1]}"


@functools.lru_cache(maxsize=None)
def _system(shape):
    """(system, params, oracle network, oracle params), cached per shape."""
    from oracle import network
    n, a = shape
    s, params, _ = support.seeded_case(support.z_name(n, a), 800 + 3 * n + a, randomize_aux=True)
    return s, params, network.Network(s), network.to_torch(params)


def _ctx(shape, dtype, reuse=True):
    s, params, _, _ = _system(shape)
    ctx = support.make_ctx(s, dtype, params)
    ctx.set_proposal_reuse(reuse)
    return ctx


def _full_gauss2(g2d):
    """[B, N, 3] draws of the moved electrons -> the oracle's [B, N, 3N] (only the diagonal blocks
    enter its ratio)."""
    B, N, _ = g2d.shape
    idx = torch.arange(N)
    g2 = torch.zeros(B, N, N, 3, dtype=torch.float64)
    g2[:, idx, idx, :] = g2d.double().cpu()
    return g2.reshape(B, N, 3 * N)


def _gap(acc, u):
    """smallest relative distance of an acceptance ratio to its uniform"""
    acc, u = acc.numpy(), u.numpy()
    return float((np.abs(acc - u) / np.maximum(acc, u)).min())


def _values(net, pt, x):
    """oracle log|psi| [B] and gradient [B, 3N] at x"""
    ls, gs = [], []
    for b in range(x.shape[0]):
        xb = x[b].clone().requires_grad_(True)
        la = net.logabs(pt, xb)
        (gb,) = torch.autograd.grad(la, xb)
        ls.append(float(la.detach()))
        gs.append(gb.numpy())
    return np.array(ls), np.array(gs)


# ---------------------------------------------------------------- 1. Philox sweep, reuse on / off
_PHILOX = {}


def _philox_case(shape):
    """(pos, seed, oracle accepts per walker): 8 walkers and the first Philox seed of 0, 1, ...
    whose draws keep MARGIN on the oracle.  The draws depend on (seed, offset, walker, electron)
    alone; they are read back after a sweep of a scratch context."""
    if shape not in _PHILOX:
        from oracle import mcstep, system
        s, _, net, pt = _system(shape)
        B = 8
        pos = system.init_electrons(np.random.default_rng(17 + shape[0]), s.atoms, s.charges, B, 1.0)
        scratch = _ctx(shape, torch.float64)
        found = None
        for seed in range(48):
            x = torch.tensor(pos, device="cuda").contiguous()
            scratch.mc_step(x, 1, TSTEP, seed=seed, offset=0)
            g1, g2d, u = (t.double().cpu() for t in scratch.last_draws(B))
            _, acc = mcstep.walkers_update(net, pt, torch.tensor(pos), g1, _full_gauss2(g2d), u, TSTEP)
            gap = _gap(acc, u)
            if gap > MARGIN:
                found = (pos, seed, (acc.numpy() > u.numpy()).sum(1))
                break
        assert found is not None, (shape, gap)
        print(f"{shape}: Philox seed {found[1]}, min relative |ratio - u| {gap:.3e}, accepts {found[2].tolist()}")
        _PHILOX[shape] = found
    return _PHILOX[shape]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_cached_proposals_match_from_scratch(shape, dtype):
    pos, seed, n_ref = _philox_case(shape)
    B = pos.shape[0]
    out = []
    for reuse in (True, False):
        ctx = _ctx(shape, dtype, reuse)
        x = torch.tensor(pos, dtype=dtype, device="cuda").contiguous()
        acc = ctx.mc_step(x, 1, TSTEP, seed=seed, offset=0, count_accepts=True)
        la, g = ctx.logpsi_grad(x)
        torch.cuda.synchronize()
        out.append((x.double().cpu(), acc.cpu(), la.double().cpu(), g.double().cpu().reshape(B, -1)))
    (xa, acc_a, la_a, g_a), (xb, acc_b, la_b, g_b) = out
    d = (xa - xb).abs().reshape(B, -1).amax(1)
    s2a, s2b = (g_a * g_a).sum(1), (g_b * g_b).sum(1)
    print(f"{shape} {dtype}: accepted {acc_a.tolist()} / {acc_b.tolist()} (oracle {n_ref.tolist()}), "
          f"max |dx| {float(d.max()):.3e}, max |dlog| {float((la_a - la_b).abs().max()):.3e}, "
          f"max |dgrad| {float((g_a - g_b).abs().max()):.3e}, max rel |ds2| {float(((s2a - s2b).abs() / s2b).max()):.3e}")
    assert acc_a.reshape(-1).tolist() == n_ref.tolist()
    assert acc_b.reshape(-1).tolist() == n_ref.tolist()
    assert not torch.equal(xa, torch.tensor(pos, dtype=dtype).double())
    if dtype == torch.float64:
        assert float(d.max()) <= 1e-11, float(d.max())
        assert torch.allclose(la_a, la_b, rtol=0, atol=1e-11)
        assert torch.allclose(g_a, g_b, rtol=1e-11, atol=1e-11)
        assert torch.allclose(s2a, s2b, rtol=1e-11, atol=1e-11)
    else:
        assert float(d.max()) <= 1e-4, d
        assert torch.allclose(la_a, la_b, rtol=1e-5, atol=2e-4)
        assert torch.allclose(g_a, g_b, rtol=1e-3, atol=1e-3)
        dg = 1e-3 * g_b.abs() + 1e-3
        assert bool(((s2a - s2b).abs() <= (2 * g_b.abs() * dg + dg * dg).sum(1)).all()), (s2a, s2b)


# ---------------------------------------------------------------- 2, 3. host-draw sweep vs the oracle
_REF = {}


def _oracle_sweeps(shape, B, nsweeps):
    """Host draws: (pos, draws [nsweeps, ...], oracle positions, accepts per walker and sweep
    [nsweeps, B, N], oracle log|psi| and grad at the final positions), cached.  The seed of the draws
    is the first of 0, 1, ... that keeps MARGIN in every sweep."""
    key = (shape, B, nsweeps)
    if key not in _REF:
        from oracle import mcstep, system
        s, _, net, pt = _system(shape)
        n = shape[0]
        pos = system.init_electrons(np.random.default_rng(29 + n), s.atoms, s.charges, B, 1.0)
        found = None
        for seed in range(48):
            g1, g2, u = support.host_draws(seed, B, n, nsweeps)
            x, conds, gap = torch.tensor(pos), [], 1.0
            for k in range(nsweeps):
                x, acc = mcstep.walkers_update(net, pt, x, g1[k], g2[k], u[k], TSTEP)
                gap = min(gap, _gap(acc, u[k]))
                conds.append(acc.numpy() > u[k].numpy())
            if gap > MARGIN:
                found = (g1, g2, u, x, np.array(conds))
                break
        assert found is not None, (shape, gap)
        g1, g2, u, x, conds = found
        print(f"{shape} B={B} sweeps={nsweeps}: draws seed {seed}, min relative |ratio - u| {gap:.3e}")
        l_ref, g_ref = _values(net, pt, x)
        _REF[key] = (pos, (g1, g2, u), x.numpy(), conds, l_ref, g_ref)
    return _REF[key]


def _host_sweeps(shape, dtype, B, nsweeps, reuse=True, packed=True):
    """(positions, accepts per walker, log|psi|, grad, context) of one mc_step of nsweeps sweeps"""
    pos, (g1, g2, u), *_ = _oracle_sweeps(shape, B, nsweeps)
    N = shape[0]
    idx = torch.arange(N)
    ctx = _ctx(shape, dtype, reuse)
    ctx.set_packed_walkers(packed)
    x = torch.tensor(pos, dtype=dtype, device="cuda").contiguous()
    acc = ctx.mc_step(x, nsweeps, TSTEP, count_accepts=True, gauss1=g1,
                      gauss2=g2.reshape(nsweeps, B, N, N, 3)[:, :, idx, idx, :].contiguous(), u=u)
    la, g = ctx.logpsi_grad(x)
    torch.cuda.synchronize()
    return x, acc, la, g, ctx


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_proposal_sweep_matches_oracle(shape):
    """fp64, 3 walkers (k_moved_electron's last wave partial): the oracle's acceptances exactly, its
    positions to 1e-9, log|psi| to 1e-10 and the gradient to 1e-8 at the new positions."""
    pos, _, x_ref, conds, l_ref, g_ref = _oracle_sweeps(shape, 3, 1)
    x, acc, la, g, _ = _host_sweeps(shape, torch.float64, 3, 1)
    n_ref = conds.sum((0, 2))
    print(f"{shape}: accepted {acc.tolist()} (oracle {n_ref.tolist()}), "
          f"max |x - oracle| {np.abs(x.cpu().numpy() - x_ref).max():.3e}, "
          f"max |log - oracle| {np.abs(la.cpu().numpy() - l_ref).max():.3e}, "
          f"max |grad - oracle| {np.abs(g.cpu().numpy() - g_ref).max():.3e}")
    assert n_ref.sum() > 0
    assert acc.cpu().numpy().reshape(-1).tolist() == n_ref.tolist()
    np.testing.assert_allclose(x.cpu().numpy(), x_ref, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(la.cpu().numpy(), l_ref, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(g.cpu().numpy(), g_ref, rtol=1e-8, atol=1e-8)


@pytest.mark.parametrize("shape", [(14, 2), (5, 1)], ids=_ids)
def test_moved_electron_records_partial_wave(shape):
    """The ECache records through their readers (k_walker_rev<PROP> on N2, k_quad_grad on (5, 1)):
    the sweep from k_moved_electron's records (last wave 10 of 16 records on N2, 15 of 16 on (5, 1))
    equals the sweep whose proposals evaluate the moved electron's stage from scratch, at the oracle
    tolerance in fp64; in fp32 it moves exactly the oracle's electrons."""
    pos, _, _, conds, _, _ = _oracle_sweeps(shape, 3, 1)
    a = _host_sweeps(shape, torch.float64, 3, 1, reuse=True)
    b = _host_sweeps(shape, torch.float64, 3, 1, reuse=False)
    assert torch.equal(a[1], b[1])
    for p, q, tol in zip((a[0], a[2], a[3]), (b[0], b[2], b[3]), (1e-9, 1e-10, 1e-8)):
        assert torch.allclose(p, q, rtol=tol, atol=tol), float((p - q).abs().max())
    cond = conds[0]
    x32 = _host_sweeps(shape, torch.float32, 3, 1, reuse=True)[0]
    moved = np.any(x32.cpu().numpy().reshape(cond.shape + (3,)) != pos.astype(np.float32).reshape(cond.shape + (3,)), axis=2)
    assert np.array_equal(moved, cond), (moved, cond)


# ---------------------------------------------------------------- 4. RW = 2 through the walker launch
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("shape", [(5, 1), (8, 2)], ids=_ids)
def test_rw2_fixed_order_walker_elimination(shape, dtype):
    """One wave per walker (set_packed_walkers(False)): the second sweep's walker launch eliminates
    in the order the first recorded (gj_fixed_regs, RW = 2).  fp64: the oracle's two sweeps to 1e-9;
    fp32: the oracle's decisions and positions to the handover bound 1e-4."""
    B, NS = 3, 2
    _, _, x_ref, conds, l_ref, g_ref = _oracle_sweeps(shape, B, NS)
    x, acc, la, g, ctx = _host_sweeps(shape, dtype, B, NS, packed=False)
    f32 = dtype == torch.float32
    # k_walker_rev (one or, for a small fp32 batch, two waves per walker), not the packed kernel
    assert ctx.launch_row("sweep_walker", B) == (6 if f32 else 7)
    assert ctx.launch_row("walker_grad", B) == 7
    n_ref = conds.sum((0, 2))
    d = np.abs(x.double().cpu().numpy() - x_ref).max()
    print(f"{shape} {dtype}: accepted {acc.tolist()} (oracle {n_ref.tolist()}), max |x - oracle| {d:.3e}")
    assert acc.cpu().numpy().reshape(-1).tolist() == n_ref.tolist()
    if f32:
        assert d <= 1e-4, d
    else:
        np.testing.assert_allclose(x.cpu().numpy(), x_ref, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(la.cpu().numpy(), l_ref, rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(g.cpu().numpy(), g_ref, rtol=1e-8, atol=1e-8)
