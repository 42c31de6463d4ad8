"""Device-memory ownership of a context: workspaces that grow, are reused at a smaller batch and
grow again give the bits of a fresh context; the fp32 accumulator banks and the weighted-gradient
rows keep their layout across reallocations; aiqmc_workspace_bytes counts what it always counted;
destroying a context returns its device memory.  Every comparison is bitwise (torch.equal)."""
import gc

import numpy as np
import pytest
import torch

from oracle import pphamiltonian as opp, system

pytestmark = pytest.mark.gpu

BATCHES = (3, 70, 5, 130)   # grow, reuse, regrow; 70 and 130 cross a wave / chunk boundary, 3 and 5 end in a partial wave


def _ctx(name, dtype):
    from aiqmc import _lib
    s = system.make_system(name)
    ctx = _lib.Context.for_system(s, dtype)
    ctx.set_params(system.flatten_params(system.init_params(np.random.default_rng(3), s, randomize_aux=True)))
    if name.endswith("_ecp"):
        e = opp.c_atom_ccecp()
        ctx.set_ecp_tables(e)
    return s, ctx


def _pos(s, B, dtype):
    x = system.init_electrons(np.random.default_rng(100 + B), s.atoms, s.charges, B, 1.0)
    return torch.tensor(x, dtype=dtype, device="cuda").reshape(B, -1).contiguous()


def _calls(name, dtype, ctx, x):
    """Every entry point with a workspace of its own, at the walkers x; fixed seeds."""
    out = list(ctx.logpsi(x)) + list(ctx.logpsi_grad(x)) + list(ctx.local_energy(x, want_logabs=True, want_grad=True))
    out.append(ctx.local_energy_complex(x))
    xm = x.clone()
    ctx.mc_step(xm, 2, 0.05, seed=11)
    out.append(xm)
    out.append(ctx.logpsi_param_grad(x))
    if name.endswith("_ecp"):
        out.append(ctx.local_energy_ecp(x, seed=5))
        xt = x.clone()
        out.append(ctx.dmc_tmoves(xt, 0.1, seed=7))
        out.append(xt)
    if name == "Be" and dtype == torch.float32:
        out.append(ctx.spin_squared(x))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name,dtype", [("Be", torch.float64), ("Be", torch.float32), ("C_ecp", torch.float64),
                                        ("C_ecp", torch.float32)])
def test_grow_reuse_regrow_matches_fresh_context(name, dtype):
    s, ctx = _ctx(name, dtype)
    last = ctx.workspace_bytes()
    for B in BATCHES:
        x = _pos(s, B, dtype)
        got = _calls(name, dtype, ctx, x)
        assert ctx.workspace_bytes() >= last
        last = ctx.workspace_bytes()
        _, fresh = _ctx(name, dtype)
        ref = _calls(name, dtype, fresh, x)
        assert len(got) == len(ref)
        for k, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a, b), (name, dtype, B, k)


def test_accumulator_banks_survive_reallocation():
    """mc_step(2 sweeps), 5 sweeps (the accumulators are reallocated: another bank stride, both
    banks unclean), then 2 sweeps twice (both banks used): the positions equal those of the
    unfused reductions, which give the same bits by design (k_taueff_part)."""
    s, fused = _ctx("Be", torch.float32)
    _, plain = _ctx("Be", torch.float32)
    plain.set_fuse_reduce(0)
    xa = _pos(s, 70, torch.float32)
    xb = xa.clone()
    for call, nsteps in enumerate((2, 5, 2, 2)):
        fused.mc_step(xa, nsteps, 0.05, seed=21, offset=10 * call)
        plain.mc_step(xb, nsteps, 0.05, seed=21, offset=10 * call)
        torch.cuda.synchronize()
        assert torch.equal(xa, xb), (call, nsteps)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_weighted_gradient_rows_after_regrow(dtype):
    """1 weight row, 4 rows (the row block of the sums grows), 1 row again: each as a fresh context."""
    s, ctx = _ctx("Be", dtype)
    B = 70   # two chunks of k_grad_partial
    x = _pos(s, B, dtype)
    w = torch.tensor(np.random.default_rng(9).standard_normal((4, B)), dtype=dtype, device="cuda")
    for rows in (1, 4, 1):
        got = ctx.param_grad_weighted(x, w[:rows].contiguous())
        _, fresh = _ctx("Be", dtype)
        ref = fresh.param_grad_weighted(x, w[:rows].contiguous())
        torch.cuda.synchronize()
        assert got.shape == (rows, ctx.nparams)
        assert torch.equal(got, ref), rows


# aiqmc_workspace_bytes of a fresh context after each call, 8 walkers.  After mc_step: the sweep
# workspace, 4 bytes x 8 walkers x (3N + 1 + 1 + N + 3N + N + 3N + 3N + N elements, the WCache's
# 3,392 per walker and the ECache's 96 per proposal, N = 14) + 16 for the two limdrift factors.
N2_F32_MC_STEP = 4 * 8 * (42 + 1 + 1 + 14 + 42 + 14 + 42 + 42 + 14 + 3392 + 14 * 96) + 16
# the later values are those of the commit before the buffers changed owner (byte counts: exact)
N2_F32_LOCAL_ENERGY = 352912
N2_F32_SPIN_SQUARED = 5850512
C_ECP_F64_LOCAL_ENERGY_ECP = 799888


def test_workspace_bytes_accounting():
    assert N2_F32_MC_STEP == 158352
    s, ctx = _ctx("N2", torch.float32)
    assert ctx.workspace_bytes() == 0
    x = _pos(s, 8, torch.float32)
    ctx.mc_step(x.clone(), 1, 0.05, seed=1)
    a = ctx.workspace_bytes()
    ctx.local_energy(x)
    b = ctx.workspace_bytes()
    ctx.spin_squared(x)
    c = ctx.workspace_bytes()
    s2, ecp = _ctx("C_ecp", torch.float64)
    ecp.local_energy_ecp(_pos(s2, 8, torch.float64), seed=5)
    d = ecp.workspace_bytes()
    torch.cuda.synchronize()
    print("workspace_bytes:", a, b, c, d)
    assert a == N2_F32_MC_STEP
    assert b == N2_F32_LOCAL_ENERGY
    assert c == N2_F32_SPIN_SQUARED
    assert d == C_ECP_F64_LOCAL_ENERGY_ECP


# bytes: the device allocator hands out memory in 2 MiB granules; before the buffers changed owner
# the same loop gave a difference of 0 at every iteration
GRANULE = 2 << 20


def test_destroy_returns_device_memory():
    """20 contexts created, used and destroyed in one process: free device memory stays where it
    was after the first (a buffer missing from the context's teardown would leak each time)."""
    free = []
    for it in range(20):
        for name, dtype in (("Be", torch.float32), ("C_ecp", torch.float64)):
            s, ctx = _ctx(name, dtype)
            x = _pos(s, 5, dtype)
            _calls(name, dtype, ctx, x)
            ctx.param_grad_weighted(x, torch.ones(3, 5, dtype=dtype, device="cuda"))
            ctx.dmc_drift_diffusion(x.clone(), 0.05, seed=3)
            torch.cuda.synchronize()
            del ctx
        gc.collect()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    print("free device memory after each iteration, relative to the first:", [f - free[0] for f in free])
    assert abs(free[-1] - free[0]) <= GRANULE, free
