"""The on-device Philox draws (AIQMC_RNG_PHILOX, the production mode of every sampler) against
the float64 host replica oracle/philox.py, read back through aiqmc_debug_read_draws.

A draw is a pure function of (seed, step, stream id, kind), so it is pinned exactly:
  a. the draw buffers a sweep leaves equal the replica (u bitwise, the normals to NORMAL_BOUND);
  b. mc_step in Philox mode equals mc_step in host mode fed the device's own draws, bit for bit
     (fused and separate acceptance): every parity result obtained with injected draws carries
     over to the production path, and a draw buffer rewritten before its last reader shows;
  c. the same for dmc_drift_diffusion;
  d. k_ecp_rot's Haar rotations equal the replica, are orthogonal, and reproduce the Philox
     local energy bit for bit when injected;
  e. k_tmove's inline uniforms (kinds 19, 20) equal the replica's: injected, they reproduce the
     Philox T-moves bit for bit.

Rows (the smallest batches that reach every draw writer and its tail):
  H2 (N = 2) B = 5     packed writer, four walkers per wave, partial last wave
  C  (N = 6) B = 3     packed writer, two per wave, partial last wave; and one wave each
  N2 (N = 14) B = 7    one wave per walker (fp64), the two-wave split (fp32, B <= 8 per CU)
  N2 fp32 B = 2112     above the split's batch limit: the single-wave fp32 launch

Normal draws: the device runs Box-Muller in float with the fast log and sincos; the largest
|device - float64 replica| over all rows and (seed, offset) pairs of test (a), measured on an
MI355X, is NORMAL_DEV_MEASURED.  The tests assert NORMAL_BOUND = 8 x that; a wrong stream id,
kind or counter word gives O(1) errors, and the bound itself must stay <= 1e-4.
"""
import functools

import numpy as np
import pytest
import torch

import support
from oracle import philox

pytestmark = pytest.mark.gpu

NORMAL_DEV_MEASURED = 1.636e-6    # N2 fp32 B = 2112, seed 2^32 + 7, offset 5 (gauss1); the small rows: 1.05e-6
NORMAL_BOUND = 8.0 * NORMAL_DEV_MEASURED     # 1.31e-5

F32, F64 = torch.float32, torch.float64
# (system, dtype, B, packed walkers)
ROWS = [
    ("H2", F64, 5, True), ("H2", F32, 5, True),
    ("C", F64, 3, True), ("C", F32, 3, True),
    ("C", F64, 3, False), ("C", F32, 3, False),
    ("N2", F64, 7, True), ("N2", F32, 7, True),
    ("N2", F32, 2112, True),
]
PAIRS = [(7, 0), (7, 2 ** 32 + 3), (2 ** 32 + 7, 5)]     # (seed, offset): low words, high step, high seed


def _id(row):
    name, dtype, B, packed = row
    return f"{name}-{'f32' if dtype == F32 else 'f64'}-B{B}" + ("" if packed else "-onewave")


@functools.lru_cache(maxsize=None)
def _setup(name):
    from oracle import system
    s = system.make_system(name)
    flat = system.flatten_params(system.init_params(np.random.default_rng(1), s))
    return s, flat


@functools.lru_cache(maxsize=None)
def _walkers(name, B, seed=2, width=1.0):
    from oracle import system
    s, _ = _setup(name)
    return system.init_electrons(np.random.default_rng(seed), s.atoms, s.charges, B, width)


def _ctx(name, dtype, packed=True, ecp=False):
    from oracle import pphamiltonian as pp
    s, flat = _setup(name)
    ctx = support.make_ctx(s, dtype, flat, ecp=pp.c_atom_ccecp() if ecp else None)
    if not packed:
        ctx.set_packed_walkers(False)
    return s, ctx


def _x0(name, B, dtype, seed=2, width=1.0):
    return torch.tensor(_walkers(name, B, seed, width), dtype=dtype, device="cuda").contiguous()


@functools.lru_cache(maxsize=None)
def _ref_draws(seed, offset, B, N):
    g1, g2, u = philox.mc_draws(seed, offset, 1, B, N)
    return g1[0], g2[0], u[0]


# ----------------------------------------------------------------------------- a. draws == replica

@pytest.mark.parametrize("row", ROWS, ids=_id)
def test_sweep_draws_equal_the_replica(row):
    """After mc_step(pos, 1, 0.05, seed, offset) the context's draw buffers hold
    mc_draws(seed, offset, 1, B, N): u bit for bit, gauss1 and gauss2 to NORMAL_BOUND.
    Measured on MI355X: largest |device normal - float64 replica| over all rows and pairs
    1.636e-6 (N2 fp32 B = 2112; 1.05e-6 over the rows of B <= 7), so NORMAL_BOUND = 1.31e-5."""
    name, dtype, B, packed = row
    s, ctx = _ctx(name, dtype, packed)
    N = s.nelectrons
    assert NORMAL_BOUND <= 1e-4
    worst = 0.0
    for seed, offset in PAIRS:
        pos = _x0(name, B, dtype)
        ctx.mc_step(pos, 1, 0.05, seed=seed, offset=offset)
        g1, g2, u = ctx.last_draws(B)
        torch.cuda.synchronize()
        assert g1.shape == (B, 3 * N) and g2.shape == (B, N, 3) and u.shape == (B, N) and u.dtype == dtype
        r1, r2, ru = _ref_draws(seed, offset, B, N)
        d1 = float(np.max(np.abs(support.to_np(g1).astype(np.float64) - r1)))
        d2 = float(np.max(np.abs(support.to_np(g2).astype(np.float64) - r2)))
        print(f"philox draws {_id(row)} seed {seed} offset {offset}: max |g1 - ref| {d1:.3e} |g2 - ref| {d2:.3e}")
        worst = max(worst, d1, d2)
        assert np.array_equal(support.to_np(u).astype(np.float64), ru), (seed, offset)
        assert d1 <= NORMAL_BOUND and d2 <= NORMAL_BOUND, (seed, offset, d1, d2)
        assert bool(torch.isfinite(pos).all())
    print(f"philox draws {_id(row)}: worst normal deviation {worst:.3e}")


# ----------------------------------------------------------------------------- b. Philox == host mode fed the device's draws

# seed 8, tstep 0.5: every row both accepts and rejects (H2 27 of 30 moves accepted, C 49 of 54, N2 260
# of 294; with seed 7 the H2 row accepts all 30)
MC_SEED, MC_OFFSET, MC_TSTEP = 8, 11, 0.5


@pytest.mark.parametrize("row", [r for r in ROWS if r[2] < 2112], ids=_id)
def test_philox_mc_step_equals_host_mode_fed_the_device_draws(row):
    """Three sweeps in one Philox call (deferred, fused acceptance, then separate acceptance
    launches) against three sweeps in host mode fed the draws a scratch context produced for
    the same (seed, offset + k): positions and acceptance counts identical bit for bit."""
    name, dtype, B, packed = row
    s, scratch = _ctx(name, dtype, packed)
    N = s.nelectrons
    xs = _x0(name, B, dtype)
    got = []
    for k in range(3):
        scratch.mc_step(xs, 1, MC_TSTEP, seed=MC_SEED, offset=MC_OFFSET + k)
        got.append([t.clone() for t in scratch.last_draws(B)])
    g1, g2, u = (torch.stack([g[j] for g in got]) for j in range(3))
    torch.cuda.synchronize()
    for k in range(3):    # the scratch draws are the replica's (u exactly), so this feeds what (a) pinned
        assert np.array_equal(support.to_np(u[k]).astype(np.float64), _ref_draws(MC_SEED, MC_OFFSET + k, B, N)[2])

    _, b = _ctx(name, dtype, packed)
    xb = _x0(name, B, dtype)
    cb = b.mc_step(xb, 3, MC_TSTEP, gauss1=g1, gauss2=g2, u=u, count_accepts=True)
    torch.cuda.synchronize()
    n_acc = int(cb.sum())
    print(f"philox mc_step {_id(row)}: accepted {n_acc} of {3 * B * N}")
    assert bool((xb != _x0(name, B, dtype)).any()) and 0 < n_acc < 3 * B * N   # moves and rejections both occur

    _, a = _ctx(name, dtype, packed)
    for fuse in (True, False):
        a.set_fuse_accept(fuse)
        xa = _x0(name, B, dtype)
        ca = a.mc_step(xa, 3, MC_TSTEP, seed=MC_SEED, offset=MC_OFFSET, count_accepts=True)
        torch.cuda.synchronize()
        assert support.same_bits(ca, cb), (fuse, support.to_np(ca), support.to_np(cb))
        assert support.same_bits(xa, xb), (fuse, float((xa - xb).abs().max()))


# ----------------------------------------------------------------------------- c. DMC drift-diffusion

@pytest.mark.parametrize("name,dtype,B", [("N2", F64, 7), ("Be", F32, 5)], ids=["N2-f64-B7", "Be-f32-B5"])
def test_philox_drift_diffusion_equals_host_mode_fed_the_device_draws(name, dtype, B):
    s, a = _ctx(name, dtype)
    N = s.nelectrons
    xa = _x0(name, B, dtype)
    go_a, gn_a, td_a = a.dmc_drift_diffusion(xa, 0.05, seed=9, offset=2 ** 32 + 4)
    g1, g2, u = a.last_draws(B)
    torch.cuda.synchronize()
    assert np.array_equal(support.to_np(u).astype(np.float64), _ref_draws(9, 2 ** 32 + 4, B, N)[2])
    _, b = _ctx(name, dtype)
    xb = _x0(name, B, dtype)
    go_b, gn_b, td_b = b.dmc_drift_diffusion(xb, 0.05, gauss1=g1[None], gauss2=g2[None], u=u[None])
    torch.cuda.synchronize()
    assert bool((xa != _x0(name, B, dtype)).any())
    assert support.same_bits(xa, xb), float((xa - xb).abs().max())
    assert support.same_bits(go_a, go_b) and support.same_bits(gn_a, gn_b)
    assert support.same_bits(td_a, td_b), (support.to_np(td_a), support.to_np(td_b))
    assert bool(torch.isfinite(go_a).all() and torch.isfinite(gn_a).all() and torch.isfinite(td_a).all())


# ----------------------------------------------------------------------------- d. rotations

ECP_B = 9


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_philox_rotations_equal_the_replica(dtype):
    """C atom with the ccECP tables: the rotations local_energy_ecp(seed=5, offset=2) drew are
    haar_rotations(5, 2, B) to NORMAL_BOUND (float32: plus their storage rounding, below it),
    orthogonal to 1e-12 (float32 storage: 8 eps), and injecting them gives the same energy bits."""
    s, ctx = _ctx("C_ecp", dtype, ecp=True)
    pos = _x0("C_ecp", ECP_B, dtype)
    e = ctx.local_energy_ecp(pos, seed=5, offset=2)
    R = ctx.last_rotations(ECP_B)
    torch.cuda.synchronize()
    assert R.shape == (ECP_B, 3, 3) and R.dtype == dtype
    Rn = support.to_np(R).astype(np.float64)
    ref = philox.haar_rotations(5, 2, ECP_B)
    dev = float(np.max(np.abs(Rn - ref)))
    orth = float(np.max(np.abs(np.einsum("bij,bkj->bik", Rn, Rn) - np.eye(3))))
    print(f"philox rotations {dtype}: max |R - ref| {dev:.3e}, |R R^T - I| {orth:.3e}")
    assert np.array_equal(np.sign(np.linalg.det(Rn)), np.sign(np.linalg.det(ref)))     # kind 18, exact
    assert dev <= NORMAL_BOUND
    assert orth <= (1e-12 if dtype == F64 else 8 * float(np.finfo(np.float32).eps))
    e2 = ctx.local_energy_ecp(pos, rot=R)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(e.real).all() and torch.isfinite(e.imag).all())
    assert support.same_bits(e, e2), float((e - e2).abs().max())


# ----------------------------------------------------------------------------- e. T-moves

# With the ccECP tables and these parameters a T-move is rare (measured: 28 to 33 of 16,384 electrons
# of walkers of width 0.5 move, 5 to 8 of width 1.0), so the nine walkers are the init_electrons
# draw (seed, width) below, for which the draws of (seed 7, offset 1) move an electron.
TM_WALKERS = (30, 0.5)    # one of the 36 electrons moves, in float64 and float32 alike (so does seed 125)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_philox_tmoves_equal_host_mode_fed_the_replica_uniforms(dtype):
    """dmc_tmoves(seed=7, offset=1) against dmc_tmoves fed the read-back rotations and the
    replica's selection (kind 19) and acceptance (kind 20) uniforms: positions and acceptances
    identical bit for bit, and at least one electron moves."""
    s, ctx = _ctx("C_ecp", dtype, ecp=True)
    N = s.nelectrons
    x0 = _x0("C_ecp", ECP_B, dtype, *TM_WALKERS)
    xa = x0.clone()
    acc_a = ctx.dmc_tmoves(xa, 0.3, seed=7, offset=1)
    R = ctx.last_rotations(ECP_B)
    torch.cuda.synchronize()
    np.testing.assert_allclose(support.to_np(R).astype(np.float64), philox.haar_rotations(7, 1, ECP_B), rtol=0, atol=NORMAL_BOUND)
    us, ua = philox.tmove_draws(7, 1, ECP_B, N)
    xb = x0.clone()
    acc_b = ctx.dmc_tmoves(xb, 0.3, rot=R, u_sel=torch.tensor(us), u_acc=torch.tensor(ua))
    torch.cuda.synchronize()
    moved = int(((xa != x0).reshape(ECP_B, N, 3).any(dim=-1)).sum())
    print(f"philox tmoves {dtype}: {moved} of {ECP_B * N} electrons moved")
    assert support.same_bits(xa, xb), float((xa - xb).abs().max())
    assert support.same_bits(acc_a, acc_b)
    assert bool(torch.isfinite(acc_a).all())
    assert moved >= 1


# ----------------------------------------------------------------------------- the read-back's argument checks

def test_read_draws_argument_checks():
    from aiqmc import _lib
    s, ctx = _ctx("H2", F64)
    lib, N, B = _lib.load(), s.nelectrons, 5
    out = torch.zeros(B * 3 * N + 1, dtype=F64, device="cuda")
    rd = lambda which, dst, n: lib.aiqmc_debug_read_draws(ctx._h, which, dst, n, None)
    assert rd(0, out.data_ptr(), 1) == -1                  # nothing allocated yet: capacity 0
    pos = _x0("H2", B, F64)
    ctx.mc_step(pos, 1, 0.05, seed=1, offset=0)
    assert rd(0, out.data_ptr(), 3 * B * N) == 0
    assert rd(2, out.data_ptr(), B * N) == 0
    assert rd(0, out.data_ptr(), 0) == 0
    assert rd(0, out.data_ptr(), 3 * B * N + 1) == -1      # past the buffer's capacity
    assert rd(2, out.data_ptr(), B * N + 1) == -1
    assert rd(0, None, 1) == -1 and rd(0, out.data_ptr(), -1) == -1
    assert rd(4, out.data_ptr(), 1) == -1 and rd(-1, out.data_ptr(), 1) == -1
    assert rd(3, out.data_ptr(), 1) == -1                  # no ECP call on this context: unallocated
    with pytest.raises(RuntimeError, match="aiqmc_debug_read_draws"):
        ctx.last_draws(B + 1)
    torch.cuda.synchronize()
