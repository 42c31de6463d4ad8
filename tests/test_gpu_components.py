"""aiqmc_energy_components on the GPU against the float64 oracle, column by column.

Inputs as tests/test_gpu_observables.py builds them: alternating spins, randomised auxiliary
parameters, walkers from init_electrons rounded to float32 so that both dtypes and the oracle see the
same positions.  The oracle's slow pieces (kinetic_jvp_of_grad, grad log|psi|, the complex kinetic
energy of Be, nonlocal_pp_energy under injected rotations) are the recorded oracle outputs of
tests/golden/components.npz (make_golden_components.py; tests/test_components_host.py recomputes the
cheap cases); the potentials are evaluated by the oracle here.

Cases: H2 (2,2) B = 5, Be (4,1) B = 7, N2 (14,2) B = 7, C atom ccECP (4,1) B = 5, CO2 ccECP (16,3)
B = 3 (a full 16-lane group), H2 B = 1 (a group whose wave is mostly idle).

Tolerances, u = 2^-24 (fp32) or 2^-53 (fp64):
  v_ee, v_en, v_pp_local   4 n_terms u sum |term| per walker from the oracle's own terms (n_terms
                N (N - 1) / 2, N A, N A KL): a distance carries at most 3.5 u (three differences,
                three squares, two additions, one square root), its reciprocal 4.5 u, the sum of n
                terms (n - 1) u sum |term|; pow and exp add a few u per term and exp(-a r^2)
                a r^2 times the 6 u of its argument, which weighs only on terms that are small
                next to the walker's sum |term|
  v_nn          equal to the oracle's float64 value rounded to the dtype
  kinetic       what tests/test_gpu_parity.py and tests/test_gpu_shapes.py grant aiqmc_local_energy
                (fp64 1e-6 absolute; fp32 rtol 2e-4, atol 2e-3 on E_L) plus the v_ee and v_en bounds
  kinetic_grad  their gradient bound d per component (fp64 1e-8 |g| + 1e-8; fp32 2e-3 max |g| + 1e-4)
                carried through 1/2 sum g^2: sum (|g| d + d^2 / 2), plus (3 N + 2) u of the value for
                the squares and their sum in the dtype
  v_pp_nonlocal what tests/test_ecp.py grants the ECP local energy (fp64 1e-6; fp32 rtol 2e-4,
                atol 2e-3) plus the bounds of the columns it is the remainder of (kinetic, v_ee,
                v_en, v_pp_local)
  closure       |total - sum of rows 1, 3, 4, 5, 6, 7| <= 8 u sum |row|, in the context dtype
"""
import os

import numpy as np
import pytest
import torch

import support
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = [("H2", 5), ("Be", 7), ("N2", 7), ("C_ecp", 5), ("CO2_ecp", 3), ("H2", 1)]
ECP = {"C_ecp": "c_atom_ccecp", "CO2_ecp": "co2_ccecp"}
DTYPES = [torch.float64, torch.float32]
U = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24}
TOT, KIN, KING, VEE, VEN, VNN, VPL, VPN = range(8)

_REF = {}
_GOLD = []


def _gold():
    if not _GOLD:
        _GOLD.append(np.load(os.path.join(GOLDEN, "components.npz")))
    return _GOLD[0]


def _el_tol(dtype, e_ref):
    """The bound the parity / shape / ECP tests grant a local energy whose oracle value is e_ref."""
    return np.full_like(e_ref, 1e-6) if dtype == torch.float64 else 2e-4 * np.abs(e_ref) + 2e-3


def _case(name):
    """Oracle references of one system, computed once and left unchanged: system, parameters,
    positions, rotations, and per walker the potentials, their sums of absolute terms and term
    counts, the kinetic energies, the gradient and the nonlocal energy."""
    if name not in _REF:
        from oracle import hamiltonian as ham, pphamiltonian as pp, system
        g = _gold()
        s = system.make_system(name)
        pos = g[f"{name}_pos"]
        atoms, charges = torch.tensor(s.atoms), torch.tensor(s.charges)
        ecp = getattr(pp, ECP[name])() if name in ECP else None
        zero = torch.zeros_like(charges)
        absecp = None if ecp is None else pp.ECP(ecp.rn_local, np.abs(ecp.local_coes), ecp.local_exps, ecp.rn_non_local,
                                                 ecp.non_local_coes, ecp.non_local_exps, ecp.list_l)
        v = np.zeros((4, pos.shape[0]))
        absv = np.zeros((4, pos.shape[0]))
        for b, x in enumerate(torch.tensor(pos)):
            r_ae, r_ee = ham.construct_r(x, atoms)
            v[0, b] = ham.potential_electron_electron(r_ee)
            v[1, b] = ham.potential_electron_nuclear(charges, r_ae)
            v[2, b] = ham.potential_nuclear_nuclear(charges, atoms)
            if ecp is not None:   # zero charges: local_pp_energy without its part1
                v[3, b] = pp.local_pp_energy(ecp, x, atoms, zero)
                absv[3, b] = pp.local_pp_energy(absecp, x, atoms, zero)
        absv[0], absv[1] = v[0], -v[1]       # every term of v_ee is positive, of v_en negative
        N, A = s.nelectrons, s.natoms
        nterms = np.array([N * (N - 1) // 2, N * A, 1, N * A * (ecp.rn_local.shape[1] if ecp is not None else 0)])
        _REF[name] = dict(s=s, ecp=ecp, params=g[f"{name}_params"], pos=pos, v=v, absv=absv, nterms=nterms,
                          rot=g[f"{name}_rot"] if ecp is not None else None, ke=g[f"{name}_ke"],
                          grad=g[f"{name}_grad"], nl=g[f"{name}_nl_re"] if ecp is not None else None,
                          ke_complex=g["Be_ke_complex"] if name == "Be" else None)
    return _REF[name]


def _ctx(c, dtype, set_params=True):
    support.skip_unbuilt(c["s"])
    return support.make_ctx(c["s"], dtype, c["params"] if set_params else None, ecp=c["ecp"])


def _run(c, ctx, dtype, sl=slice(None), complex_output=False):
    x = torch.tensor(c["pos"][sl], device="cuda", dtype=dtype)
    rot = None if c["rot"] is None else torch.tensor(c["rot"][sl], device="cuda", dtype=dtype)
    out = ctx.energy_components(x, complex_output=complex_output, rot=rot)
    torch.cuda.synchronize()
    return x, rot, out


@pytest.mark.parametrize("name,B", CASES, ids=[f"{n}-B{b}" for n, b in CASES])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_columns_match_the_oracle(dtype, name, B):
    c = _case(name)
    u = U[dtype]
    ctx = _ctx(c, dtype)
    x, rot, out = _run(c, ctx, dtype, slice(0, B))
    assert out.shape == (8, B) and out.dtype == dtype
    got = out.double().cpu().numpy()
    v, absv, nt = c["v"][:, :B], c["absv"][:, :B], c["nterms"]
    bound = 4.0 * nt[:, None] * u * absv                       # rows v_ee, v_en, (v_nn), v_pp_local
    ke, gr = c["ke"][:B], c["grad"][:B]
    # v_ee, v_en, v_pp_local
    for row, k in ((VEE, 0), (VEN, 1), (VPL, 3)):
        err = np.abs(got[row] - v[k])
        print(f"{name} {dtype} B={B} row {row}: max err {err.max():.3g}, of the bound "
              f"{(err / np.maximum(bound[k], 1e-300)).max():.3g}")
        assert np.all(err <= bound[k]), (row, got[row], v[k], bound[k])
    # v_nn
    want_nn = torch.tensor(v[2]).to(dtype).double().numpy()
    print(f"{name} {dtype} v_nn {got[VNN][0]!r} oracle {v[2][0]!r}")
    assert np.array_equal(got[VNN], want_nn)
    # kinetic
    e_ae = ke + v[0] + v[1] + v[2]
    tol_kin = _el_tol(dtype, e_ae) + bound[0] + bound[1]
    err = np.abs(got[KIN] - ke)
    print(f"{name} {dtype} kinetic: max err {err.max():.3g}, of the bound {(err / tol_kin).max():.3g}")
    assert np.all(err <= tol_kin), (got[KIN], ke, tol_kin)
    # kinetic_grad
    tg = 0.5 * (gr ** 2).sum(1)
    d = 1e-8 * np.abs(gr) + 1e-8 if dtype == torch.float64 else 2e-3 * np.abs(gr).max(axis=1, keepdims=True) + 1e-4
    tol_tg = (np.abs(gr) * d + 0.5 * d * d).sum(1) + (gr.shape[1] + 2) * u * tg
    err = np.abs(got[KING] - tg)
    print(f"{name} {dtype} kinetic_grad: max err {err.max():.3g}, of the bound {(err / tol_tg).max():.3g}")
    assert np.all(err <= tol_tg), (got[KING], tg, tol_tg)
    # total: the bits of the existing call; v_pp_nonlocal
    if c["ecp"] is None:
        e0, _, _ = ctx.local_energy(x)
        assert np.all(got[VPL] == 0.0) and np.all(got[VPN] == 0.0)
    else:
        e0 = ctx.local_energy_ecp(x, rot=rot).real
        nl = c["nl"][:B]
        tol_nl = _el_tol(dtype, e_ae + v[3] + nl) + tol_kin + bound[0] + bound[1] + bound[3]
        err = np.abs(got[VPN] - nl)
        print(f"{name} {dtype} v_pp_nonlocal: max err {err.max():.3g}, of the bound {(err / tol_nl).max():.3g}")
        assert np.all(err <= tol_nl), (got[VPN], nl, tol_nl)
    torch.cuda.synchronize()
    assert torch.equal(out[TOT], e0.contiguous())
    # closure, in the context dtype
    rows = [KIN, VEE, VEN, VNN, VPL, VPN]
    ssum = out[rows[0]].clone()
    for r in rows[1:]:
        ssum = ssum + out[r]
    gap = (out[TOT] - ssum).abs().double().cpu().numpy()
    lim = 8.0 * u * out.abs().double().sum(0).cpu().numpy()
    print(f"{name} {dtype} closure: max {gap.max():.3g}, of the bound {(gap / lim).max():.3g}")
    assert np.all(gap <= lim), (gap, lim)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_complex_output_kinetic_matches_the_oracle(dtype):
    c = _case("Be")
    ctx = _ctx(c, dtype)
    x, _, out = _run(c, ctx, dtype, complex_output=True)
    got = out.double().cpu().numpy()
    v, ke = c["v"], c["ke_complex"]
    bound = 4.0 * c["nterms"][:, None] * U[dtype] * c["absv"]
    tol = _el_tol(dtype, ke + v[0] + v[1] + v[2]) + bound[0] + bound[1]
    err = np.abs(got[KIN] - ke)
    print(f"Be {dtype} complex kinetic: max err {err.max():.3g}, of the bound {(err / tol).max():.3g}")
    assert np.all(err <= tol), (got[KIN], ke, tol)
    assert torch.equal(out[TOT], ctx.local_energy_complex(x).real.contiguous())
    real = ctx.energy_components(x)
    assert torch.equal(out[VEE:VPN + 1], real[VEE:VPN + 1]) and torch.equal(out[KING], real[KING])


@pytest.mark.parametrize("name,split", [("N2", 3), ("C_ecp", 2)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_potential_rows_do_not_depend_on_batching(dtype, name, split):
    """Rows 3..6 of a walker are the same bits in one call, in two calls that split the batch (N2:
    7 = 3 + 4), and from run to run."""
    c = _case(name)
    ctx = _ctx(c, dtype)
    _, _, whole = _run(c, ctx, dtype)
    _, _, again = _run(c, ctx, dtype)
    _, _, head = _run(c, ctx, dtype, slice(0, split))
    _, _, tail = _run(c, ctx, dtype, slice(split, None))
    assert torch.equal(whole[VEE:VPL + 1], again[VEE:VPL + 1])
    assert torch.equal(whole[VEE:VPL + 1], torch.cat([head, tail], dim=1)[VEE:VPL + 1])
    assert torch.isfinite(whole).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_coincident_electrons_stay_in_their_walker(dtype):
    """H2, B = 4, electron 0 of walker 2 copied onto electron 1: v_ee[2] = +inf by ordinary
    arithmetic, and the potential rows of walkers 0, 1 and 3 keep their bits."""
    c = _case("H2")
    ctx = _ctx(c, dtype)
    x = torch.tensor(c["pos"][:4], device="cuda", dtype=dtype)
    ref = ctx.energy_components(x)
    bad = x.clone()
    bad[2, 3:6] = bad[2, 0:3]
    out = ctx.energy_components(bad)
    torch.cuda.synchronize()
    assert out[VEE, 2] == float("inf")
    keep = [0, 1, 3]
    assert torch.equal(out[VEE:VPL + 1][:, keep], ref[VEE:VPL + 1][:, keep])
    assert torch.isfinite(out[:, keep]).all()


def _network(name):
    from oracle import system
    from aiqmc import spin_indices
    from aiqmc.wavefunction_Ynlm import nn
    s = system.make_system(name)
    par, anti, npar, nanti = spin_indices.jastrow_indices_ee(spins=s.spins, nelectrons=s.nelectrons)
    up, dn = spin_indices.spin_indices_h(s.spins)
    net = nn.make_ai_net(ndim=3, nelectrons=s.nelectrons, natoms=s.natoms, nspins=s.nspins, determinants=1,
                         charges=s.charges, parallel_indices=par, antiparallel_indices=anti, n_parallel=npar,
                         n_antiparallel=nanti, spin_up_indices=up, spin_down_indices=dn)
    return s, net, nn


@pytest.mark.parametrize("name", ["Be", "C_ecp"])
def test_drop_in_equals_the_context_call(name):
    from oracle import system
    from aiqmc.Energy import components, pphamiltonian
    c = _case(name)
    s, net, nn = _network(name)
    params = system.unflatten_params(system.init_params(np.random.default_rng(0), s), c["params"])
    x = torch.tensor(c["pos"], device="cuda")
    data = nn.AINetData(positions=x, spins=s.spins, atoms=s.atoms, charges=s.charges)
    kw = {}
    if c["ecp"] is not None:
        e = c["ecp"]
        kw = dict(rn_local=e.rn_local, local_coes=e.local_coes, local_exps=e.local_exps, rn_non_local=e.rn_non_local,
                  non_local_coes=e.non_local_coes, non_local_exps=e.non_local_exps, list_l=e.list_l,
                  natoms=s.natoms, nelectrons=s.nelectrons, ndim=3)
    fn = components.make_energy_components(net.apply, s.charges, s.nspins, **kw)
    if c["ecp"] is None:
        out = fn(params, None, data)
        ctx = net.apply._aiqmc_network.bind(params, s.atoms, torch.float64)
        want = ctx.energy_components(x)
    else:
        rot = torch.tensor(c["rot"])
        out = fn(params, pphamiltonian.HostRotations(rot), data)
        ctx = net.apply._aiqmc_network.bind(params, s.atoms, torch.float64)
        want = ctx.energy_components(x, rot=rot)
        seeded = fn(params, 11, data)                    # Philox rotations
        assert torch.equal(seeded, ctx.energy_components(x, seed=11))
        assert torch.equal(seeded[VEE:VPL + 1], out[VEE:VPL + 1])
    assert out.shape == (8, x.shape[0]) and torch.equal(out, want)
    empty = ctx.energy_components(x[:0])
    assert empty.shape == (8, 0) and empty.dtype == torch.float64


def test_call_before_set_params_raises_the_library_message():
    c = _case("H2")
    ctx = _ctx(c, torch.float32, set_params=False)
    with pytest.raises(RuntimeError, match="aiqmc_set_params has not been called"):
        ctx.energy_components(torch.tensor(c["pos"][:2], device="cuda", dtype=torch.float32))
    assert ctx.workspace_bytes() == 0


def test_samples_feed_the_blocking_accumulator():
    """8 samples of N2 (B = 8, one sweep between them) straight into make_blocking(nseries=8): the
    level-0 means are the fp64 means of the stacked samples, so [K][B] is the layout blocking expects."""
    from aiqmc import statistics
    from aiqmc.Energy import components
    c = _case("N2")
    ctx = _ctx(c, torch.float32)
    x = torch.tensor(np.concatenate([c["pos"], c["pos"][:1] + 0.125]), device="cuda", dtype=torch.float32).contiguous()
    acc = statistics.make_blocking(nseries=8, names=components.COMPONENT_NAMES)
    samples = []
    for it in range(8):
        ctx.mc_step(x, 1, 0.02, seed=3, offset=it)
        out = ctx.energy_components(x)
        acc.update(out)
        samples.append(out.double().cpu().numpy())
    torch.cuda.synchronize()
    want = np.stack(samples).mean(axis=(0, 2))
    for k, name in enumerate(components.COMPONENT_NAMES):
        m = float(acc.result(name)["mean"][0])
        assert abs(m - want[k]) <= 1e-12 * max(abs(want[k]), 1e-300), (name, m, want[k])
    s = components.summarize(acc)
    assert abs(s["v_nn"]["mean"] - samples[0][VNN, 0]) <= 1e-12 * samples[0][VNN, 0]
    assert np.isfinite(s["virial_ratio"]["value"]) and np.isfinite(s["kinetic_gap"]["value"])
    assert ctx.workspace_bytes() > 0
