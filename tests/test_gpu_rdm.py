"""aiqmc_rdm_accumulate / aiqmc_rdm_basis_values on the GPU against the float64 oracle forward
(oracle/network.py) on numpy-built moved configurations, as tests/test_gpu_observables.py does for S^2.

Systems: H2 (2,2) four configurations per wave, Z5 with nspins (3,2) two per wave and odd N, N2
(14,2); spin-polarised Z5@uuuud (4,1) and Z5@duddd (1,4), the minority first.  Batches 5 (partial last wave, one partial group) and 8; H2 also 37 (two groups, the second
partial).  S = 3 points per walker for H2 and Z5 (S n_sigma is no multiple of 4), 1 for N2.  Bases:
"p3" one p shell (norb = 3, below one MFMA tile) and "spd17" s, p and d shells on two centres
(nao = 20) with a random [2][20][17] coefficient matrix (two tiles with a tail, rho_up != rho_down).
Walkers, points and weights are rounded to float32, so both dtypes and the oracle see the same input.

The element-wise bound of the matrix is derived, not measured.  With t_c the oracle's term of row
c = (walker, point, electron of the channel) and T_c >= |t_c| the same term with every basis value
replaced by sum_a |ao_a| |C_aj|,

    |sum - ref| <= sum_c |t_c| eps_c + T_c gamma,

eps_c = atol + rtol |dlogabs_c| + atol_phase: the single-value bounds of tests/test_gpu_observables.py
(TOL, already doubled for a difference); gamma = n u / (1 - n u), u = 2^-24 or 2^-53, with n counted
from csrc/rdm.hip:
    2 (nao + 1)   each of the two basis values: the fp64 Gaussian rounded once, then the nao fma's of
                  the MO contraction (1 without coefficients; nao + 1 is used for both)
    8             F = exp(dl) (cos dp, sin dp) / q w: expf 1, sincosf 2 (of |ratio|), the product a c, the
                  rounding of 1 / q, the products with it and with w, and phi_j F: 5
    R             one rounding per row of the MFMA accumulation chain, R = min(B, 32) S n_sigma rows
                  of a group (the products themselves are exact inside the fma)
plus, for the fp64 Gaussians (both dtypes), (12 + primitives + 5 max alpha r^2) 2^-53 per basis
value: the rounding of exp's argument is amplified by the argument itself.  The fp64 fold of the
group tiles adds nothing at this level.
"""
import numpy as np
import pytest
import torch

import support
from replicas_estimators import C0, C1, TOL, _shells

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DTYPES = pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
# spin-polarised, "<system>@<u/d per slot>" (oracle/system.py): (4,1), and (1,4) with the minority first
POLARISED = ["Z5@uuuud", "Z5@duddd"]
SAMPLES = {"H2": 3, "Z5": 3, "N2": 1, "Z5@uuuud": 3, "Z5@duddd": 3}
BMAX = {"H2": 37, "Z5": 8, "N2": 8, "Z5@uuuud": 8, "Z5@duddd": 8}
QC, QS, QP = np.array([[0.0, 0.0, -0.7], [0.1, 0.0, 0.8]]), np.array([1.25, 1.5]), np.array([0.625, 0.375])
NORMAL_BOUND = 1.31e-5      # tests/test_gpu_philox.py: device Box-Muller against the float64 replica

_REF, _BASIS = {}, {}


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _basis(kind):
    """(GaussianBasis, Mixture)."""
    if kind not in _BASIS:
        from aiqmc import observables as obs
        if kind == "p3":
            b = obs.GaussianBasis([obs.Shell(C0, 1, [0.9, 0.3], obs.normalized_shell(1, [0.9, 0.3], [0.5, 0.6]))])
        else:
            b = obs.GaussianBasis(_shells(obs), np.random.default_rng(17).standard_normal((2, 20, 17)))
        _BASIS[kind] = (b, obs.mixture(QC, QS, QP))
    return _BASIS[kind]


def ao_np(basis, pts):
    """(values [M, nao], largest alpha r^2, most primitives of a shell), float64 numpy, vectorised over points."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    cols, arg, npmax = [], 0.0, 0
    for s in basis.shells:
        d = pts - s.center
        r2 = (d * d).sum(1)
        rad = (s.coefs[None] * np.exp(-s.exponents[None] * r2[:, None])).sum(1)
        arg, npmax = max(arg, float(s.exponents.max() * r2.max())), max(npmax, s.exponents.size)
        if s.l == 0:
            cols.append(rad)
        elif s.l == 1:
            cols += [d[:, k] * rad for k in range(3)]
        else:
            cols += [d[:, i] * d[:, j] * rad for i in range(3) for j in range(i, 3)]
    return np.stack(cols, 1), arg, npmax


def basis_np(basis, pts, spin):
    """(phi [M, K], sum_a |ao_a| |C_aj| [M, K], gamma of one basis value in units of 1: see the module docstring)."""
    ao, arg, npmax = ao_np(basis, pts)
    g64 = (12 + npmax + 5.0 * arg) * 2.0 ** -53
    if basis.mo_coeff is None:
        return ao, np.abs(ao), g64
    return ao @ basis.mo_coeff[spin], np.abs(ao) @ np.abs(basis.mo_coeff[spin]), g64


def _case(name):
    """(system, params, pos [Bmax, 3N], rp [Bmax, S, 3], w [Bmax], dl, dp [Bmax, S, N]) of the float64
    oracle, computed once per system."""
    if name not in _REF:
        from oracle import network, system
        s = system.make_system(name)
        N, S, B = s.nelectrons, SAMPLES[name], BMAX[name]
        rng = np.random.default_rng(500 + 7 * N + s.natoms)
        params = system.init_params(rng, s, randomize_aux=True)
        pos = _f32(system.init_electrons(rng, s.atoms, s.charges, B, 1.0))
        rp = _f32(QC[rng.integers(0, 2, (B, S))] + rng.standard_normal((B, S, 3)))
        w = _f32(rng.uniform(0.5, 1.5, B))
        x = np.repeat(pos.reshape(B, 1, 1, N, 3), S, 1).repeat(N, 2)
        for e in range(N):
            x[:, :, e, e, :] = rp
        net, pt = network.Network(s), network.to_torch(params)
        psi = lambda y: np.array([[float(v) for v in net.apply(pt, r)] for r in torch.tensor(y)]).T
        ph0, la0 = psi(pos)
        ph1, la1 = (v.reshape(B, S, N) for v in psi(x.reshape(-1, 3 * N)))
        _REF[name] = (s, params, pos, rp, w, la1 - la0[:, None, None], ph1 - ph0[:, None, None],
                      x.reshape(B, S * N, 3 * N))
    return _REF[name][:7]


def q_np(r):
    d2 = ((np.asarray(r)[..., None, :] - QC) ** 2).sum(-1)
    return (QP * (2 * np.pi * QS ** 2) ** -1.5 * np.exp(-d2 / (2 * QS ** 2))).sum(-1)


def reference(s, basis, pos, rp, w, dl, dp, dtype):
    """(sums [1 + 2 K K 2] float64 in the layout of acc, bound of the same shape) from the ratios dl, dp."""
    B, S, N, K = pos.shape[0], rp.shape[1], s.nelectrons, basis.norb
    t = s.tables()
    rtol, atol, atol_ph = TOL[dtype]
    u = 2.0 ** -24 if dtype == F32 else 2.0 ** -53
    wv = np.ones(B) if w is None else w
    f = np.exp(dl) * np.exp(1j * dp) * (wv[:, None] / q_np(rp))[:, :, None]            # [B, S, N]
    eps = atol + rtol * np.abs(dl) + atol_ph
    out, bound = np.zeros((2, K, K), dtype=np.complex128), np.zeros((2, K, K))
    for sg, slots in enumerate((t["spin_up_indices"], t["spin_down_indices"])):
        slots = np.asarray(slots).reshape(-1)
        a, a_abs, g1 = basis_np(basis, pos.reshape(B, N, 3)[:, slots].reshape(-1, 3), sg)
        p, p_abs, g2 = basis_np(basis, rp.reshape(-1, 3), sg)
        a, a_abs = a.reshape(B, len(slots), K), a_abs.reshape(B, len(slots), K)
        p, p_abs = p.reshape(B, S, K), p_abs.reshape(B, S, K)
        n = 2 * (basis.nao + 1) + 8 + min(B, 32) * S * len(slots)
        gamma = n * u / (1 - n * u) + g1 + g2
        fs = f[:, :, slots]
        out[sg] = np.einsum("bei,bsj,bse->ij", a, p, fs)
        bound[sg] = (np.einsum("bei,bsj,bse->ij", np.abs(a), np.abs(p), np.abs(fs) * eps[:, :, slots])
                     + gamma * np.einsum("bei,bsj,bse->ij", a_abs, p_abs, np.abs(fs)))
    flat = np.stack([out.real, out.imag], -1).reshape(-1)
    return np.concatenate([[wv.sum()], flat]), np.concatenate([[B * u * wv.sum()], np.repeat(bound.reshape(-1), 2)])


def _ctx(s, params, dtype, kind=None):
    support.skip_unbuilt(s)
    ctx = support.make_ctx(s, dtype, params)
    if kind is not None:
        b, q = _basis(kind)
        ctx.set_rdm_basis(b.shell_l, b.shell_nprim, b.shell_center, b.exps, b.coefs, b.mo_coeff, q.centres, q.sigmas,
                          q.probs)
    return ctx


CASES = [("H2", 5), ("H2", 8), ("H2", 37), ("Z5", 5), ("Z5", 8), ("N2", 5), ("N2", 8)] + [(n, B) for n in POLARISED
                                                                                          for B in (5, 8)]


@pytest.mark.parametrize("kind", ["p3", "spd17"])
@pytest.mark.parametrize("name,B", CASES)
@DTYPES
def test_matrix_matches_oracle(dtype, name, B, kind):
    s, params, pos, rp, w, dl, dp = _case(name)
    basis, _ = _basis(kind)
    wb = w[:B] if B == 5 else None                     # B = 5 runs weighted, the others with unit weights
    ref, bound = reference(s, basis, pos[:B], rp[:B], wb, dl[:B], dp[:B], dtype)
    ctx = _ctx(s, params, dtype, kind)
    acc = ctx.rdm_accumulate(support.dev(pos[:B], dtype), SAMPLES[name], rprime=support.dev(rp[:B], dtype),
                             weights=None if wb is None else support.dev(wb, dtype))
    torch.cuda.synchronize()
    got = acc.cpu().numpy()
    assert got.shape == (1 + 4 * basis.norb ** 2,)
    err = np.abs(got - ref)
    print(f"{name} {dtype} B={B} {kind}: max |err| / bound {np.max(err[1:] / bound[1:]):.3g}, max |err| {err[1:].max():.3g}, "
          f"max |ref| {np.abs(ref[1:]).max():.3g}, W err {err[0]:.3g}")
    assert np.all(np.isfinite(got))
    assert np.all(err <= bound), (np.max(err / bound), int(np.argmax(err / bound)))
    K = basis.norb
    m = got[1:].reshape(2, K, K, 2)
    if kind == "spd17":
        assert np.abs(m[0] - m[1]).max() > 1e-3 * np.abs(m).max()
    if name in POLARISED:
        # the trace of a channel's block is a sum over that channel's n_up or n_down electron slots.  In
        # this finite, non-orthogonal basis it is not the electron count itself, so it is held to the
        # replica's trace within the summed diagonal bounds; and the replica alone shows that the
        # channels cannot be swapped unnoticed: with the slot lists exchanged its traces move by
        # more than twice those bounds.
        from oracle import system
        swapped = system.make_system(name.translate(str.maketrans("ud", "du")))
        assert swapped.nspins == s.nspins[::-1] and s.nspins[0] != s.nspins[1]
        ref_sw, bound_sw = reference(swapped, basis, pos[:B], rp[:B], wb, dl[:B], dp[:B], dtype)
        tr = lambda v: np.einsum("siic->sc", v[1:].reshape(2, K, K, 2))
        tb = np.maximum(tr(bound), tr(bound_sw)[::-1])
        assert np.all(np.abs(tr(got) - tr(ref)) <= tr(bound))
        assert np.all(np.abs(tr(ref)[:, 0] - tr(ref_sw)[:, 0]) > 2 * tb[:, 0]), (tr(ref), tr(ref_sw), tb)


@pytest.mark.parametrize("name", ["H2", "Z5", "N2"])
@DTYPES
def test_ratios_are_logpsi_differences_bitwise(dtype, name):
    """ratio_out is, bit for bit, Context.logpsi on host-built moved positions minus logpsi at the walker."""
    s, params, pos, rp, _, _, _ = _case(name)
    B, S, N = 5, SAMPLES[name], s.nelectrons
    ctx = _ctx(s, params, dtype, "p3")
    x = support.dev(pos[:B], dtype)
    xm = support.dev(_REF[name][7][:B].reshape(-1, 3 * N), dtype)
    _, rpo, ro = ctx.rdm_accumulate(x, S, rprime=support.dev(rp[:B], dtype), want_points=True, want_ratios=True)
    la0, ph0 = ctx.logpsi(x)
    la1, ph1 = ctx.logpsi(xm)
    torch.cuda.synchronize()
    assert ro.shape == (B, S, N, 2) and torch.equal(rpo, support.dev(rp[:B], dtype))
    assert torch.equal(ro[..., 0].reshape(B, S * N), la1.reshape(B, S * N) - la0[:, None])
    assert torch.equal(ro[..., 1].reshape(B, S * N), ph1.reshape(B, S * N) - ph0[:, None])


@pytest.mark.parametrize("kind", ["p3", "spd17"])
@DTYPES
def test_basis_values_match_numpy(dtype, kind):
    """|phi - ref| <= (n u) sum_a |ao_a| |C_aj|, n = nao + 1 roundings of the operand dtype (the rounded
    Gaussian, the fma chain) plus the fp64 Gaussian's own (12 + primitives + 5 max alpha r^2) 2^-53.
    M = 70 points: three tiles of 32 with a partial last one."""
    s, params, _, _, _, _, _ = _case("H2")
    basis, _ = _basis(kind)
    ctx = _ctx(s, None, dtype, kind)                   # the evaluator needs no parameters
    pts = _f32(np.random.default_rng(23).standard_normal((70, 3)) * 1.5)
    u = 2.0 ** -24 if dtype == F32 else 2.0 ** -53
    for spin in (0, 1):
        got = ctx.rdm_basis_values(support.dev(pts, dtype), spin).double().cpu().numpy()
        ref, mag, g64 = basis_np(basis, pts, spin)
        n = basis.nao + 1
        bound = (n * u / (1 - n * u) + g64) * mag
        assert got.shape == ref.shape == (70, basis.norb)
        print(f"{kind} {dtype} spin {spin}: max |err| / bound {np.max(np.abs(got - ref) / bound):.3g}")
        assert np.all(np.abs(got - ref) <= bound)
    assert ctx.rdm_basis_values(support.dev(pts[:0], dtype)).shape == (0, basis.norb)


@pytest.mark.parametrize("name,B", [("H2", 37), ("Z5", 5)])
@DTYPES
def test_philox_points_and_injection(dtype, name, B):
    """rprime_out equals the host replica (Mixture.sample = oracle/philox.py kinds 24 / 25, sid = b S + s)
    to the device normals' bound times sigma plus the roundings of sigma, c and the fma in the operand
    dtype; the matrix equals the injected-mode matrix fed with that rprime_out, bit for bit."""
    s, params, pos, _, w, _, _ = _case(name)
    S = SAMPLES[name]
    _, q = _basis("spd17")
    ctx = _ctx(s, params, dtype, "spd17")
    x, wd = support.dev(pos[:B], dtype), support.dev(w[:B], dtype)
    u = 2.0 ** -24 if dtype == F32 else 2.0 ** -53
    for seed, step in ((5, 0), (2 ** 32 + 7, 2 ** 32 + 3)):
        a, rpo = ctx.rdm_accumulate(x, S, seed=seed, step=step, weights=wd, want_points=True)
        b = ctx.rdm_accumulate(x, S, rprime=rpo, weights=wd)
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        ref = q.sample(seed, step, B, S)
        got = rpo.double().cpu().numpy()
        # |c| + sigma |g| <= 2 |c| + |r'|: one rounding each of sigma, c and the fma
        bound = q.sigmas.max() * NORMAL_BOUND + 3 * u * (2 * np.abs(q.centres).max() + np.abs(ref))
        print(f"{name} {dtype}: max |r' - replica| {np.abs(got - ref).max():.3g}")
        assert got.shape == (B, S, 3) and np.all(np.abs(got - ref) <= bound)
    assert not torch.equal(a, ctx.rdm_accumulate(x, S, seed=5, step=1, weights=wd))


@DTYPES
def test_chunking_repeats_and_accumulate_are_bitwise(dtype):
    """H2, B = 37, S = 3: 7 configurations per walker; a chunk of 224 is one group of 32 walkers, so two
    chunks with a partial second one.  accumulate = 1 after accumulate = 0 on one group doubles every entry."""
    s, params, pos, rp, w, _, _ = _case("H2")
    ctx = _ctx(s, params, dtype, "spd17")
    x, r, wd = support.dev(pos, dtype), support.dev(rp, dtype), support.dev(w, dtype)
    one = ctx.rdm_accumulate(x, 3, rprime=r, weights=wd, want_ratios=True)
    many = ctx.rdm_accumulate(x, 3, rprime=r, weights=wd, want_ratios=True, chunk=224)
    tiny = ctx.rdm_accumulate(x, 3, rprime=r, weights=wd, want_ratios=True, chunk=1)    # still whole groups
    again = ctx.rdm_accumulate(x, 3, rprime=r, weights=wd, want_ratios=True)
    torch.cuda.synchronize()
    for other in (many, tiny, again):
        for a, b in zip(one, other):
            assert torch.equal(a, b)
    acc = ctx.rdm_accumulate(x[:8], 3, rprime=r[:8], weights=wd[:8])
    single = acc.clone()
    ctx.rdm_accumulate(x[:8], 3, rprime=r[:8], weights=wd[:8], acc=acc, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(acc, 2.0 * single) and float(single[1:].abs().max()) > 0


@DTYPES
def test_drop_in_accumulator_equals_the_context_call(dtype):
    from aiqmc import observables as obs, systems
    from aiqmc.wavefunction_Ynlm import nn
    s = systems.make_system("Be")
    net = s.make_network()
    params = net.init(9)
    rng = np.random.default_rng(31)
    B, S = 8, 2
    from oracle import system as osys
    so = osys.make_system("Be")
    pos = _f32(osys.init_electrons(rng, so.atoms, so.charges, B, 1.0))
    rp = _f32(rng.standard_normal((B, S, 3)))
    w = _f32(rng.uniform(0.5, 1.5, B))
    basis, q = _basis("spd17")
    x, r, wd = support.dev(pos, dtype), support.dev(rp, dtype), support.dev(w, dtype)
    data = nn.AINetData(positions=x, spins=s.spins, atoms=s.atoms, charges=s.charges)
    acc = obs.make_density_matrix(net.apply, s.nspins, basis, q=q, samples=S)
    acc.update(params, data, r, weights=wd)
    ctx = net.apply._aiqmc_network.bind(params, s.atoms, dtype)
    v, ro = ctx.rdm_accumulate(x, S, rprime=r, weights=wd, want_ratios=True)
    K = basis.norb
    assert torch.equal(acc.last(), torch.view_as_complex(v[1:].clone().reshape(2, K, K, 2)) / (v[0] * S))
    acc.update(params, data, 7)                           # Philox mode through the accumulator
    v2 = ctx.rdm_accumulate(x, S, seed=7, step=0)
    assert torch.equal(acc.state[1:1 + acc.n], v + v2) and float(acc.state[0]) == 2.0
    # the generic torch path on the same tensors: an untagged callable around the same kernels
    gen = obs.make_density_matrix(lambda *a: net.apply(*a), s.nspins, basis, q=q, samples=S)
    gen.update(params, data, r, weights=wd)
    ro = ro.double().cpu().numpy()
    _, bound = reference(so, basis, pos, rp, w, ro[..., 0], ro[..., 1], dtype)
    got, ref = v.cpu().numpy(), gen._last.cpu().numpy()
    print(f"Be {dtype}: kernel against generic path, max |diff| / bound {np.max(np.abs(got - ref) / bound):.3g}")
    assert np.all(np.abs(got - ref) <= bound)


def test_empty_batch_missing_params_and_missing_basis():
    s, params, pos, rp, _, _, _ = _case("H2")
    x, r = support.dev(pos[:4], F64), support.dev(rp[:4], F64)
    with pytest.raises(RuntimeError, match="set_params"):
        _ctx(s, None, F64, "p3").rdm_accumulate(x, 3, rprime=r)
    ctx = _ctx(s, params, F64)
    with pytest.raises(RuntimeError, match="set_rdm_basis"):
        ctx.rdm_accumulate(x, 3, rprime=r)
    with pytest.raises(RuntimeError, match="set_rdm_basis"):
        ctx.rdm_basis_values(x[:, :3])
    ctx = _ctx(s, params, F64, "p3")
    acc = torch.full((1 + 4 * 9,), 3.0, dtype=F64, device="cuda")
    ctx.rdm_accumulate(x[:0], 3, rprime=r[:0], acc=acc)       # B == 0 returns OK and writes nothing
    assert float(acc.min()) == 3.0 == float(acc.max())
    with pytest.raises(RuntimeError, match="S must be"):
        ctx.rdm_accumulate(x, 0, rprime=r[:, :0])
    ctx.clear_rdm_basis()
    with pytest.raises(RuntimeError, match="set_rdm_basis"):
        ctx.rdm_accumulate(x, 3, rprime=r)
