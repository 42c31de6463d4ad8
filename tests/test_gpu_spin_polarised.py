"""The kernels on spin-polarised systems against the float64 oracle: n_up != ceil(N / 2), n_down >
n_up, minority-first slot orders.  Every other GPU test builds alternating spins (n_up = ceil(N / 2),
n_up - n_down in {0, 1}) or the (4, 4) block order of C2_ecp, where a wrong spin-group bound, a
swapped 1 / n_up and 1 / n_down, or an n_down / n_up mix-up changes nothing or only the last row.

Systems are named "<system>@<u/d per slot>" (oracle/system.py).  The smallest cases that put each
lopsided partition through each kernel family:
  four walkers per wave (N <= 4)   Z3@ddu (1,2) minority first, Z4@uuud (3,1), Z4@dudd (1,3),
                                   Z2-2@uduu (3,1) on two atoms
  two walkers per wave (N <= 8)    Z5@uuuud (4,1), Z6@uuduud (4,2) the C triplet, Z7@uuuduud (5,2) the
                                   N quartet, Z4-3@duddudd (2,5), Z4-4@dddduddd (1,7)
  one wave per walker (N >= 9)     Z9@uuuuduuuu (8,1), Z5-5@uuuduuduud (7,3), Z5-4-4@ddudddudddudd
                                   (3,10) on three atoms, Z8-8@uuuuuuuuuddddddd (9,7) the O2 triplet
Four walkers per case (two for N > 10: the oracle's Laplacian), randomised auxiliary parameters,
electrons at their atoms plus a unit normal, as tests/test_gpu_shapes.py.  The oracle of a case is
computed once and shared by its tests.

Tolerances (those of test_gpu_shapes.py, test_gpu_parity.py, test_ecp.py and test_dmc.py):
  fp64  log|psi| rtol / atol 1e-10, its gradient 1e-8, cos / sin of the phase 1e-9 (the parity of
        the row permutation lives in the phase), E_L 1e-6 Ha; two host-draw Metropolis sweeps
        (the second one starts from the walker cache) positions 1e-9; d log|psi| / d theta and
        d phase / d theta 1e-8 of each walker's largest component, the e-e Jastrow columns
        (ee_anti before ee_par in the canonical vector) also on their own; pseudopotential E_L real
        and imaginary part 1e-6 Ha; T-moves positions 1e-9, acceptance rtol 1e-8 / atol 1e-10.
  fp32  against the same fp64 oracle: log|psi| rtol 1e-5 / atol 2e-4, E_L rtol 2e-4 / atol 2e-3, the
        parameter gradients 5e-3 of the row maximum, pseudopotential Re E_L rtol 2e-4 / atol 2e-3;
        three fp32 sweeps follow the fp64 sweeps (at most one decision in 100 flips, at most B / 20
        walkers diverge, the rest agree to 1e-4).
The Metropolis comparison first asserts, on the oracle alone, that the first sweep (and so the two
together) accepts some but not all of its B N proposals.

Walkers: no walker is excluded or replaced in this file; the seeds are 700 + the case's position
in CASES, and every fp32 comparison passes on them (MI355X: fp32 |d log|psi|| <= 4.3e-5, the oracle's
orbital matrices have 2-norm condition numbers between 1e2 and 3.6e4).  Should an fp32 comparison
ever fail on a walker the fp64 kernel passes, the only admissible change is another seed for that
case, chosen because the condition number of the ORACLE's orbital matrix
(oracle.network.Network.orbitals) of that walker exceeds 1e5: the elimination's error in log|psi|
grows with cond x 2^-24, which then reaches 6e-3, beyond the 2e-4 the bound allows, whatever the
kernel does.  No kernel output enters that choice, and the fp64 assertions admit no exclusions.
"""
import numpy as np
import pytest
import torch

import support

pytestmark = pytest.mark.gpu

PACK4 = ["Z3@ddu", "Z4@uuud", "Z4@dudd", "Z2-2@uduu"]
PACK2 = ["Z5@uuuud", "Z6@uuduud", "Z7@uuuduud", "Z4-3@duddudd", "Z4-4@dddduddd"]
WAVE1 = ["Z9@uuuuduuuu", "Z5-5@uuuduuduud", "Z5-4-4@ddudddudddudd", "Z8-8@" + "u" * 9 + "d" * 7]
CASES = PACK4 + PACK2 + WAVE1
NSPINS = {"Z3@ddu": (1, 2), "Z4@uuud": (3, 1), "Z4@dudd": (1, 3), "Z2-2@uduu": (3, 1), "Z5@uuuud": (4, 1),
          "Z6@uuduud": (4, 2), "Z7@uuuduud": (5, 2), "Z4-3@duddudd": (2, 5), "Z4-4@dddduddd": (1, 7),
          "Z9@uuuuduuuu": (8, 1), "Z5-5@uuuduuduud": (7, 3), "Z5-4-4@ddudddudddudd": (3, 10), WAVE1[3]: (9, 7)}
TSTEP, SWEEPS = 0.05, 2
# seeds of the Metropolis draws, 7 + N + 100 k: per case the first k at which the ORACLE rejects a
# proposal in every sweep (at tstep 0.05 it accepts about 97 in 100; Z2-2@uduu: in the first sweep)
MC_SEED = dict(zip(CASES, [1510, 11, 2211, 1211, 112, 813, 614, 514, 115, 16, 117, 120, 123]))

_PG, _MC = {}, {}


def _system(name):
    from oracle import system
    s = system.make_system(name)
    support.skip_unbuilt(s)
    return s


def _draw(name, B=None, seed=None):
    """(system, params, pos [B, 3N]) of a case: its seeded parameters and walkers."""
    _system(name)
    return support.seeded_case(name, 700 + CASES.index(name) if seed is None else seed, B, randomize_aux=True)


def _oracle(name):
    """(system, params, pos, e_l, logabs, phase, grad) of the fp64 oracle, cached per case."""
    _system(name)
    return support.oracle_case(name, 700 + CASES.index(name), randomize_aux=True, phase=True)


def _param_grads(name):
    """(d log|psi| / d theta, d phase / d theta) [B, P] of the oracle, cached per case."""
    if name not in _PG:
        from oracle import loss, network
        s, params, pos = _oracle(name)[:3]
        net = network.Network(s)
        _PG[name] = (loss.logabs_param_grad(net, params, torch.tensor(pos)),
                     loss.phase_param_grad(net, params, torch.tensor(pos)))
    return _PG[name]


def _metropolis(name):
    """(gauss1, gauss2, u, final positions, accepted proposals per sweep) of SWEEPS oracle sweeps."""
    if name not in _MC:
        from oracle import mcstep, network
        s, params, pos = _oracle(name)[:3]
        N, B = s.nelectrons, pos.shape[0]
        g1, g2, u = support.host_draws(MC_SEED[name], B, N, SWEEPS)
        net, pt = network.Network(s), network.to_torch(params)
        x, accepts = torch.tensor(pos), []
        for k in range(SWEEPS):
            info = {}
            x, _ = mcstep.walkers_update(net, pt, x, g1[k], g2[k], u[k], TSTEP, info=info)
            accepts.append(int(info["cond"].sum()))
        _MC[name] = (g1, g2, u, x.numpy(), accepts)
    return _MC[name]


def _ee_columns(s, params):
    """Canonical-vector slices of ee_anti and ee_par: tree_flatten sorts the keys, so the vector is
    envelope, jastrow_ae, jastrow_ee (ee_anti, then ee_par), layers, orbitals, y."""
    from oracle import system
    off = sum(a.size for a in system.tree_flatten({k: params[k] for k in ("envelope", "jastrow_ae")}))
    t = s.tables()
    anti = slice(off, off + t["n_antiparallel"])
    par = slice(anti.stop, anti.stop + t["n_parallel"])
    flat = system.flatten_params(params)
    assert np.array_equal(flat[anti], params["jastrow_ee"]["ee_anti"])
    assert np.array_equal(flat[par], params["jastrow_ee"]["ee_par"])
    return anti, par


def _assert_rows(got, ref, bound, s, params, what):
    """|got - ref| below `bound` of each row's largest component: the e-e Jastrow columns first, by
    name, then every column."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref) / (np.abs(ref).max(axis=1, keepdims=True) + 1e-3)
    anti, par = _ee_columns(s, params)
    assert anti.stop - anti.start == s.nspins[0] * s.nspins[1]
    for label, sl in (("ee_anti", anti), ("ee_par", par)):
        if sl.stop > sl.start:
            assert err[:, sl].max() < bound, (what, label, err[:, sl].max())
    assert err.max() < bound, (what, err.max(), np.unravel_index(err.argmax(), err.shape))


@pytest.mark.parametrize("name", CASES)
def test_case_is_the_partition_it_claims(name):
    s = _system(name)
    assert s.nspins == NSPINS[name] and s.nspins[0] != (s.nelectrons + 1) // 2


@pytest.mark.parametrize("name", CASES)
def test_polarised_fp64_matches_oracle(name):
    s, params, pos, e_ref, l_ref, ph_ref, g_ref = _oracle(name)
    ctx = support.make_ctx(s, torch.float64, params)
    x = torch.tensor(pos, device="cuda")
    e, l, g = ctx.local_energy(x, want_logabs=True, want_grad=True)
    l2, g2 = ctx.logpsi_grad(x)
    l3, ph = ctx.logpsi(x)
    torch.cuda.synchronize()
    for la in (l, l2, l3):
        np.testing.assert_allclose(la.cpu().numpy(), l_ref, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(g.cpu().numpy(), g_ref, rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(g2.cpu().numpy(), g_ref, rtol=1e-8, atol=1e-8)
    ph = ph.cpu().numpy()
    np.testing.assert_allclose(np.cos(ph), np.cos(ph_ref), atol=1e-9)
    np.testing.assert_allclose(np.sin(ph), np.sin(ph_ref), atol=1e-9)
    err = np.abs(e.cpu().numpy() - e_ref)
    print(f"{name}: max |dE_L| {err.max():.3g} Ha")
    assert err.max() <= 1e-6, (e.cpu().numpy(), e_ref)


@pytest.mark.parametrize("name", CASES)
def test_polarised_two_metropolis_sweeps_match_oracle(name):
    s, params, pos = _oracle(name)[:3]
    g1, g2, u, x_ref, accepts = _metropolis(name)
    N, B = s.nelectrons, pos.shape[0]
    # the oracle alone: the comparison is not vacuous, and the second sweep starts from walkers of
    # which some electrons moved and some did not
    assert 0 < accepts[0] < B * N and 0 < sum(accepts) < SWEEPS * B * N, (accepts, B * N)
    ctx = support.make_ctx(s, torch.float64, params)
    idx = torch.arange(N)
    x = torch.tensor(pos, device="cuda").contiguous()
    ctx.mc_step(x, SWEEPS, TSTEP, gauss1=g1, gauss2=g2.reshape(SWEEPS, B, N, N, 3)[:, :, idx, idx, :].contiguous(), u=u)
    torch.cuda.synchronize()
    np.testing.assert_allclose(x.cpu().numpy(), x_ref, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("name", CASES)
def test_polarised_param_grads_match_oracle(name):
    s, params, pos = _oracle(name)[:3]
    O_ref, P_ref = _param_grads(name)
    ctx = support.make_ctx(s, torch.float64, params)
    x = torch.tensor(pos, device="cuda")
    _assert_rows(ctx.logpsi_param_grad(x).cpu().numpy(), O_ref, 1e-8, s, params, "logpsi_param_grad")
    _assert_rows(ctx.phase_param_grad(x).cpu().numpy(), P_ref, 1e-8, s, params, "phase_param_grad")


@pytest.mark.parametrize("name", CASES)
def test_polarised_fp32_matches_oracle(name):
    s, params, pos, e_ref, l_ref, _, _ = _oracle(name)
    O_ref, P_ref = _param_grads(name)
    ctx = support.make_ctx(s, torch.float32, params)
    x = torch.tensor(pos, device="cuda").float().contiguous()
    e, l, _ = ctx.local_energy(x, want_logabs=True, want_grad=True)
    O, P = ctx.logpsi_param_grad(x), ctx.phase_param_grad(x)
    torch.cuda.synchronize()
    l, e = l.double().cpu().numpy(), e.double().cpu().numpy()
    print(f"{name}: fp32 max |dlogabs| {np.abs(l - l_ref).max():.3g}, max |dE_L| {np.abs(e - e_ref).max():.3g}")
    np.testing.assert_allclose(l, l_ref, rtol=1e-5, atol=2e-4)
    np.testing.assert_allclose(e, e_ref, rtol=2e-4, atol=2e-3)
    _assert_rows(O.double().cpu().numpy(), O_ref, 5e-3, s, params, "logpsi_param_grad fp32")
    _assert_rows(P.double().cpu().numpy(), P_ref, 5e-3, s, params, "phase_param_grad fp32")


@pytest.mark.parametrize("name,B", [("Z4@uuud", 5), ("Z7@uuuduud", 3)])
def test_polarised_param_grad_partial_last_wave(name, B):
    """B no multiple of the walkers per wave (4 for N <= 4, 2 for N <= 8): the last wave is partial.
    Rows and one weighted sum of d log|psi| and d phase, fp64 against the oracle at 1e-8, fp32 at 5e-3."""
    from oracle import loss, network
    s, params, pos = _draw(name, B=B, seed=40 + CASES.index(name))
    net = network.Network(s)
    w = np.random.default_rng(3).normal(size=B)
    c64, c32 = support.make_ctx(s, torch.float64, params), support.make_ctx(s, torch.float32, params)
    x = torch.tensor(pos, device="cuda")
    for ref, fn in ((loss.logabs_param_grad(net, params, torch.tensor(pos)), "logpsi_param_grad"),
                    (loss.phase_param_grad(net, params, torch.tensor(pos)), "phase_param_grad")):
        _assert_rows(getattr(c64, fn)(x).cpu().numpy(), ref, 1e-8, s, params, fn)
        ws = getattr(c64, fn)(x, weights=torch.tensor(w, device="cuda")).cpu().numpy()
        np.testing.assert_allclose(ws, w @ ref, rtol=0, atol=1e-8 * np.abs(w @ ref).max())
        _assert_rows(getattr(c32, fn)(x.float().contiguous()).double().cpu().numpy(), ref, 5e-3, s, params, fn + " fp32")


def _ecp_tables(name):
    from oracle import pphamiltonian as pp
    return pp.c_atom_ccecp() if name.startswith("C_ecp") else pp.c2_ccecp()


@pytest.mark.parametrize("name", ["C_ecp@uuud", "C_ecp@dudd", "C2_ecp@uuuuuudd"])
def test_polarised_ecp_local_energy_matches_oracle(name):
    """Pseudopotential E_L (the packed quadrature launch: four configurations per wave for the C
    atom, two for C2) with injected rotations against oracle.pphamiltonian, live; the ccECP tables of
    the C and C2 examples."""
    from oracle import network, pphamiltonian as pp, system
    s = _system(name)
    ecp = _ecp_tables(name)
    rng = np.random.default_rng(71 + len(name))
    params = system.init_params(rng, s, randomize_aux=True)
    B = 4 if s.nelectrons <= 4 else 2
    pos = system.init_electrons(rng, s.atoms, s.charges, B, 1.0)
    rots = pp.haar_rotations(rng, B)
    ref, _, _, _ = pp.batch_local_energy_pp(network.Network(s), network.to_torch(params), ecp, torch.tensor(pos), rots)
    ref = ref.detach().numpy()
    c64, c32 = support.make_ctx(s, torch.float64, params), support.make_ctx(s, torch.float32, params)
    c64.set_ecp_tables(ecp)
    c32.set_ecp_tables(ecp)
    e = c64.local_energy_ecp(torch.tensor(pos, device="cuda"), rot=torch.tensor(rots, device="cuda"))
    e32 = c32.local_energy_ecp(torch.tensor(pos, device="cuda", dtype=torch.float32),
                               rot=torch.tensor(rots, device="cuda", dtype=torch.float32))
    torch.cuda.synchronize()
    e, e32 = e.cpu().numpy(), e32.cpu().numpy().astype(np.complex128)
    print(f"{name}: max |dE| fp64 {np.abs(e - ref).max():.3g}, fp32 {np.abs(e32.real - ref.real).max():.3g}")
    assert np.max(np.abs(e.real - ref.real)) <= 1e-6, (e, ref)
    assert np.max(np.abs(e.imag - ref.imag)) <= 1e-6, (e, ref)
    np.testing.assert_allclose(e32.real, ref.real, rtol=2e-4, atol=2e-3)


@pytest.mark.parametrize("table", ["ccecp", "attractive"])
def test_polarised_tmoves_match_oracle(table):
    """One T-move step on C_ecp@uuud (3,1) with host draws against oracle.dmc.tmoves, live: the draws
    and the two tables (the ccECP one, and the attractive list_l = 1 table under which electrons
    move) of tests/golden/make_golden_tmoves.py; positions 1e-9, acceptance rtol 1e-8 / atol 1e-10."""
    from oracle import dmc as odmc, network, pphamiltonian as pp, system
    s = _system("C_ecp@uuud")
    ecp, tau = {"ccecp": (pp.c_atom_ccecp(), 0.1),
                "attractive": (pp.ECP([[1.0]], [[0.0]], [[1.0]], [[[2.0], [1.0]]], [[[-3.0], [-5.0]]], [[[0.7], [0.4]]], 1),
                               0.3)}[table]
    B = 8
    rng = np.random.default_rng(41)
    params = system.init_params(rng, s, randomize_aux=True)
    pos = system.init_electrons(rng, s.atoms, s.charges, B, 1.0)
    rots = pp.haar_rotations(rng, B)
    u_sel = np.array([0.0, 1e-4, 1e-3, 3e-3, 0.0, 0.5, 2e-4, 0.9])
    u_acc = rng.uniform(size=(B, s.nelectrons))
    net, pt = network.Network(s), network.to_torch(params)
    new, acc = zip(*[odmc.tmoves(net, pt, ecp, torch.tensor(pos[b]), rots[b], u_sel[b], u_acc[b], tau) for b in range(B)])
    new, acc = torch.stack(new).numpy(), np.stack(acc)
    if table == "attractive":
        assert (np.abs(new - pos).reshape(B, -1, 3).sum(-1) > 0).any()     # the oracle moves electrons
    ctx = support.make_ctx(s, torch.float64, params)
    ctx.set_ecp_tables(ecp)
    x = torch.tensor(pos, device="cuda").contiguous()
    got = ctx.dmc_tmoves(x, tau, rot=torch.tensor(rots), u_sel=torch.tensor(u_sel), u_acc=torch.tensor(u_acc))
    torch.cuda.synchronize()
    np.testing.assert_allclose(x.cpu().numpy(), new, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(got.cpu().numpy(), acc, rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("name", ["Z7@uuuduud", "Z9@uuuuduuuu", "Z5-4-4@ddudddudddudd"])
def test_polarised_fp32_sweeps_follow_fp64(name):
    """Three fp32 Metropolis sweeps against fp64 sweeps from the same float-rounded walkers and host
    draws (the caps of test_shape_fp32_sweeps_follow_fp64): at most one acceptance decision in 100
    flips, at most B / 20 walkers diverge, and the others agree to 1e-4."""
    B, NS = 64, 3
    s, params, pos = _draw(name, B=B, seed=5 + CASES.index(name))
    n = s.nelectrons
    pos = pos.astype(np.float32).astype(np.float64)
    g = torch.Generator().manual_seed(n + 10 * s.natoms)
    kw = dict(gauss1=torch.randn(NS, B, 3 * n, generator=g, dtype=torch.float64),
              gauss2=torch.randn(NS, B, n, 3, generator=g, dtype=torch.float64),
              u=torch.rand(NS, B, n, generator=g, dtype=torch.float64))
    c64, c32 = support.make_ctx(s, torch.float64, params), support.make_ctx(s, torch.float32, params)
    x64 = torch.tensor(pos, device="cuda").contiguous()
    x32 = x64.float().contiguous()
    a64 = c64.mc_step(x64, NS, TSTEP, count_accepts=True, **kw)
    a32 = c32.mc_step(x32, NS, TSTEP, count_accepts=True, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(x32).all()
    n64, n32 = int(a64.sum()), int(a32.sum())
    assert n64 > B * n * NS // 4, n64
    assert abs(n32 - n64) <= max(1, B * n * NS // 100), (n32, n64)
    dw = (x32.double() - x64).abs().reshape(B, -1).amax(1)
    same = dw < 1e-3
    assert int((~same).sum()) <= max(1, B // 20), dw.topk(4)
    assert float(dw[same].max()) < 1e-4, float(dw[same].max())
