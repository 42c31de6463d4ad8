"""The places where a 32-bit lane offset or a clamp of the scalar-base addressing (jets.h: uat,
ubase) can go wrong: the kernels address the parameter block, the walker cache (WCache), the
proposal records (ECache) and the local energy's cache (LapCache) as a wave-uniform base plus an
unsigned 32-bit offset within one record.

Every case is one Metropolis sweep with host draws followed by log|psi|, its gradient and E_L at
the new positions, against the fp64 oracle, in fp64 and fp32:

  * shapes (14, 2) the benchmark's (the widest records of the MFMA-Phi proposals), (5, 1) odd N on
    the packed route, (8, 2) the packed route's full row groups, (16, 3) the widest records of all;
  * 1 and 3 walkers: the proposal launch's and k_moved_electron's last workgroup is partial (two
    proposal waves and two 16-record waves per workgroup: N = 14 gives 14 and 42 proposals);
  * the uniforms of electrons 0 and N - 1 are ~0, so both are accepted in every walker and the
    accepted position is the proposal built from the first / last row of every cache (pi = 0 and
    pi = N - 1); the test asserts that both moved.

Tolerances are those of test_gpu_prop_trim.py and test_gpu_shapes.py: fp64 positions 1e-9, log|psi|
1e-10, gradient 1e-8, E_L 1e-6; fp32 the oracle's acceptances exactly (the draws are chosen so that
no oracle ratio lies within MARGIN = 1e-3 of its uniform, ten times fp32's ~1e-4), positions 1e-4,
and at the kernel's own fp32 positions log|psi| rtol 1e-5 / atol 2e-4, gradient rtol / atol 1e-3,
E_L rtol 2e-4 / atol 2e-3 against the oracle evaluated there.

No case places a walker's record beyond 2^31 bytes of the walker cache: the fp32 N2 record is
13,568 bytes, so that needs about 160,000 walkers' buffers and 2.2 million proposals per sweep (far
from a few seconds, with the oracle out of reach).  The guarantee is static instead: the per-configuration base (conf * size)
is 64-bit scalar arithmetic in every kernel, only the offset within one record is 32-bit, and
k_walker_rev static_asserts every record and table size it indexes (URecordFits).
"""
import functools

import numpy as np
import pytest
import torch

import support

pytestmark = pytest.mark.gpu

SHAPES = [(14, 2), (5, 1), (8, 2), (16, 3)]
BATCHES = [1, 3]
MARGIN = 1e-3
TSTEP = 0.05
_ids = lambda sh: f"N{sh[0]}A{sh[1]}"


_REF = {}


@functools.lru_cache(maxsize=None)
def _system(shape):
    """(system, params, oracle network, oracle params), cached per shape."""
    from oracle import network
    n, a = shape
    s, params, _ = support.seeded_case(support.z_name(n, a), 900 + 3 * n + a, randomize_aux=True)
    return s, params, network.Network(s), network.to_torch(params)


def _reference(shape, B):
    """(pos, draws, oracle positions after the sweep, oracle acceptances [B, N]), computed once per
    (shape, B): the first draw seed whose oracle ratios all keep MARGIN from their uniforms, with the
    uniforms of electrons 0 and N - 1 set to 1e-12 (always accepted)."""
    key = (shape, B)
    if key not in _REF:
        from oracle import mcstep, system
        s, _, net, pt = _system(shape)
        n = shape[0]
        pos = system.init_electrons(np.random.default_rng(31 + n + B), s.atoms, s.charges, B, 1.0)
        found, gap = None, 0.0
        for seed in range(48):
            rng = np.random.default_rng(seed)
            g1 = torch.tensor(rng.standard_normal((B, 3 * n)))
            g2 = torch.tensor(rng.standard_normal((B, n, 3 * n)))
            u = torch.tensor(rng.uniform(size=(B, n)))
            u[:, 0] = 1e-12
            u[:, n - 1] = 1e-12
            x, acc = mcstep.walkers_update(net, pt, torch.tensor(pos), g1, g2, u, TSTEP)
            a, uu = acc.numpy(), u.numpy()
            gap = float((np.abs(a - uu) / np.maximum(a, uu)).min())
            if gap > MARGIN:
                found = (pos, (g1, g2, u), x.numpy(), a > uu)
                break
        assert found is not None, (shape, B, gap)
        print(f"{shape} B={B}: draws seed {seed}, min relative |ratio - u| {gap:.3e}")
        _REF[key] = found
    return _REF[key]


def _oracle_values(shape, x):
    from oracle import hamiltonian
    _, _, net, pt = _system(shape)
    e, l, g = hamiltonian.batch_local_energy(net, pt, torch.tensor(x))
    return e.numpy(), l.numpy(), g.numpy()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("B", BATCHES, ids=lambda b: f"B{b}")
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_sweep_and_values_match_oracle(shape, B, dtype):
    s, params, _, _ = _system(shape)
    pos, (g1, g2, u), x_ref, cond = _reference(shape, B)
    N = shape[0]
    idx = torch.arange(N)
    ctx = support.make_ctx(s, dtype, params)
    x = torch.tensor(pos, dtype=dtype, device="cuda").contiguous()
    acc = ctx.mc_step(x, 1, TSTEP, count_accepts=True, gauss1=g1[None],
                      gauss2=g2.reshape(1, B, N, N, 3)[:, :, idx, idx, :].contiguous(), u=u[None])
    e, l, g = ctx.local_energy(x, want_logabs=True, want_grad=True)
    torch.cuda.synchronize()
    xk = x.double().cpu().numpy()
    x0 = torch.tensor(pos, dtype=dtype).double().numpy()
    moved = np.any(xk.reshape(B, N, 3) != x0.reshape(B, N, 3), axis=2)
    dx = float(np.abs(xk - x_ref).max())
    f32 = dtype == torch.float32
    # fp32: the oracle at the kernel's own positions (a position error is asserted apart)
    e_ref, l_ref, g_ref = _oracle_values(shape, xk if f32 else x_ref)
    ek, lk, gk = (t.double().cpu().numpy() for t in (e, l, g))
    gk = gk.reshape(g_ref.shape)
    print(f"{shape} B={B} {dtype}: accepted {acc.cpu().numpy().reshape(-1).tolist()} (oracle {cond.sum(1).tolist()}), "
          f"max |x - oracle| {dx:.3e}, |log - oracle| {np.abs(lk - l_ref).max():.3e}, "
          f"|grad - oracle| {np.abs(gk - g_ref).max():.3e}, |E_L - oracle| {np.abs(ek - e_ref).max():.3e}")
    assert cond[:, 0].all() and cond[:, N - 1].all()
    assert np.array_equal(moved, cond), (moved, cond)          # pi = 0 and pi = N - 1 among them
    assert acc.cpu().numpy().reshape(-1).tolist() == cond.sum(1).tolist()
    if f32:
        assert dx <= 1e-4, dx
        np.testing.assert_allclose(lk, l_ref, rtol=1e-5, atol=2e-4)
        np.testing.assert_allclose(gk, g_ref, rtol=1e-3, atol=1e-3)
        np.testing.assert_allclose(ek, e_ref, rtol=2e-4, atol=2e-3)
    else:
        np.testing.assert_allclose(xk, x_ref, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(lk, l_ref, rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(gk, g_ref, rtol=1e-8, atol=1e-8)
        assert np.max(np.abs(ek - e_ref)) <= 1e-6, (ek, e_ref)
