"""The kernels on close-approach walkers against the recorded oracle
(tests/golden/close_approach_<name>.npz, make_golden_close_approach.py; the reference's own
soundness on these walkers is tests/test_close_approach_host.py).

Every other kernel-versus-oracle test draws ordinary walkers; here an electron sits 1e-1 ... 1e-4
bohr from a nucleus (en, en2, en_ax) or from another electron (ee_anti, ee_par), where the 1/r,
1/r^2 and 1/r^3 jets of electron.h and of the pair stream, their reciprocal / square-root / tanh
approximations and the proposal launch's cache reuse are most fragile: |grad log|psi|| reaches 5e4
and E_L 8e8 Ha.  Systems: Be (4,1), C (6,1), Z5-4 (9,2), C_ecp (4,1), 19 walkers each (odd: the packed
launches end in a partial wave that holds close walkers).  No walker is masked.

Bounds per walker, S = |E_L - V| + V_ee + |V_en| + V_nn the cancellation scale of the fixture:
  tol64 = 1e-9 max(S, 1e3) Ha   (the 1e-6 Ha bar on walkers whose terms are of order 1e3, scaled)
  tol32 = 2e-4 max(S, 10) Ha    (the suite's fp32 relative tolerance applied to S)
  log|psi| and its gradient as tests/test_gpu_shapes.py: rtol = atol = 1e-10 and 1e-8 in fp64; fp32
  rtol 1e-5 / atol 2e-4 and 2e-3 of the walker's largest gradient component.
fp32 runs start from the float32-rounded positions and are compared with the float64 oracle at
those same positions (rounding moves a 1e-4 distance by up to 1e-3 of itself).

Every test prints, per (kind, d), the largest error over its bound and the quantity it belongs to,
  CLOSE <system> <dtype> <entry> <kind> d=<d> <error / bound> <quantity>
(profiles/close_approach_errors.txt is that output of an MI355X run) and fails with the list of
(kind, d) groups above 1.

Measured on MI355X (largest error / bound over all systems, layouts and walkers):
  fp64  E_L 8.6e-5 (en2, 1e-2; the complex energy the same), log|psi| 8e-5, gradient 8e-6,
        parameter gradient 3.9e-6, ECP energy 2.5e-5, reuse vs scratch 7e-11, sweep positions 4.4e-7
        with every decision the oracle's, drift-diffusion 2.7e-6, tdamp 3e-16 absolute;
  fp32  E_L 0.26 (en, 1e-1; 0.013 at 1e-4), log|psi| 0.041, gradient 3.7e-3, ECP energy 0.036,
        v_ee 0.12 and v_en 0.14 of their rounding bounds, closure 0.061, no decision different from
        the fp64 kernels', same-decision positions 1.7e-3, fused == unfused limdrift sums.
A scratch library with the float reciprocal's argument clamped at 1e-3 in magnitude (jets.h f_rcp)
fails 17 of the fp32 cases here (every value / energy case, the components, the ECP energy, one
sweep); f_rcp serves more than the distance jets, so tests/test_gpu_mc_fp32.py and
tests/test_precision_fp32.py notice that mutation on N2 as well.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

NAMES = ["Be", "C", "Z5-4", "C_ecp"]
KINDS = ("base", "pad", "en", "ee_anti", "ee_par", "en2", "en_ax", "mid")
TSTEP = 0.05
DT = {"fp64": torch.float64, "fp32": torch.float32}
LAYOUTS = [(n, lay) for n in NAMES for lay in ("default", "lap1", "unpacked") if not (lay == "unpacked" and n == "Z5-4")]

_FIX = {}


def tol64(S):
    return 1e-9 * np.maximum(S, 1e3)


def tol32(S):
    return 2e-4 * np.maximum(S, 10.0)


def _fix(name):
    """(system, fixture arrays), loaded once and left unchanged."""
    if name not in _FIX:
        from oracle import system
        g = dict(np.load(os.path.join(GOLDEN, f"close_approach_{name}.npz")))
        for a in g.values():
            a.flags.writeable = False
        _FIX[name] = (system.make_system(name), g)
    return _FIX[name]


def _ctx(name, dtype, ecp=False):
    from aiqmc import _lib
    s, g = _fix(name)
    assert (s.nelectrons, s.natoms) in _lib.supported_shapes()
    ctx = _lib.Context.for_system(s, dtype)
    if ecp:
        from oracle import pphamiltonian
        ctx.set_ecp_tables(pphamiltonian.c_atom_ccecp())
    ctx.set_params(g["params_flat"])
    return s, g, ctx


def _pos(g, dtype):
    return torch.tensor(g["pos32"] if dtype == torch.float32 else g["pos"], device="cuda", dtype=dtype)


class Report:
    """Largest error / bound per (kind, d) of each compared quantity; the groups above 1 fail."""

    def __init__(self, name, tag, entry, g):
        self.head, self.g, self.bad, self.worst = f"CLOSE {name} {tag} {entry}", g, [], {}
        print()   # the records start their own lines under pytest -s

    def note(self, text):
        print(f"{self.head} {text}")

    def add(self, what, err, bound):
        """err, bound: [B] or [B, ...] arrays (bound broadcastable to err)."""
        err = np.asarray(err, np.float64)
        ratio = err / np.broadcast_to(np.maximum(bound, 1e-300), err.shape)
        ratio = np.where(np.isfinite(err), ratio, np.inf).reshape(err.shape[0], -1).max(axis=1)
        kind, d = self.g["kind"], self.g["d"]
        for k, dd in sorted({(int(k), float(x)) for k, x in zip(kind, d)}):
            r = float(ratio[(kind == k) & (d == dd)].max())
            if not r <= self.worst.get((k, dd), (-1.0, ""))[0]:
                self.worst[(k, dd)] = (r, what)
            if not r <= 1.0:
                self.bad.append((what, KINDS[k], dd, float(f"{r:.3g}")))

    def check(self):
        """One line per (kind, d): the largest error / bound and the quantity it belongs to."""
        for (k, dd), (r, what) in sorted(self.worst.items()):
            print(f"{self.head} {KINDS[k]} d={dd:.0e} {r:.3g} {what}")
        assert not self.bad, f"{self.head}: error / bound > 1 for (quantity, kind, d, ratio) {self.bad}"


def _value_bounds(g, dtype):
    """Reference and bound arrays of log|psi|, its gradient and E_L for a dtype."""
    if dtype == torch.float64:
        l, gr, e = g["logabs"], g["grad"], g["e_l"]
        return l, gr, e, 1e-10 + 1e-10 * np.abs(l), 1e-8 + 1e-8 * np.abs(gr), tol64(g["S"])
    l, gr, e = g["r32_logabs"], g["r32_grad"], g["r32_e_l"]
    return l, gr, e, 2e-4 + 1e-5 * np.abs(l), 2e-3 * np.abs(gr).max(axis=1, keepdims=True), tol32(g["r32_S"])


def _np(t):
    return t.double().cpu().numpy()


@pytest.mark.parametrize("name,layout", LAYOUTS, ids=[f"{n}-{lay}" for n, lay in LAYOUTS])
@pytest.mark.parametrize("tag", ["fp64", "fp32"])
def test_value_gradient_and_local_energy(tag, name, layout):
    """(a) logpsi, logpsi_grad and local_energy(want_logabs, want_grad) in the default layout, with
    one wave per walker in the first-derivative pass (set_lap_waves(1); 19 walkers split 4 ways by
    default) and, for N <= 8, with one wave per walker in the walker launch
    (set_packed_walkers(False)).  The same bounds for every layout."""
    dtype = DT[tag]
    s, g, ctx = _ctx(name, dtype)
    if layout == "lap1":
        ctx.set_lap_waves(1)
    if layout == "unpacked":
        ctx.set_packed_walkers(False)
    x = _pos(g, dtype)
    la, ph = ctx.logpsi(x)
    l2, g2 = ctx.logpsi_grad(x)
    e, l3, g3 = ctx.local_energy(x, want_logabs=True, want_grad=True)
    torch.cuda.synchronize()
    l, gr, el, bl, bg, be = _value_bounds(g, dtype)
    rep = Report(name, tag, f"value[{layout}]", g)
    rep.add("logpsi.logabs", np.abs(_np(la) - l), bl)
    if dtype == torch.float64:
        rep.add("logpsi.phase", np.abs(np.angle(np.exp(1j * (_np(ph) - g["phase"])))), np.full_like(l, 1e-9))
    rep.add("logpsi_grad.logabs", np.abs(_np(l2) - l), bl)
    rep.add("logpsi_grad.grad", np.abs(_np(g2) - gr), bg)
    rep.add("local_energy.logabs", np.abs(_np(l3) - l), bl)
    rep.add("local_energy.grad", np.abs(_np(g3) - gr), bg)
    rep.add("local_energy.e_l", np.abs(_np(e) - el), be)
    rep.check()


@pytest.mark.parametrize("name", NAMES)
def test_complex_local_energy(name):
    """(b) local_energy_complex in fp64: real and imaginary parts within tol64."""
    s, g, ctx = _ctx(name, torch.float64)
    e = ctx.local_energy_complex(_pos(g, torch.float64))
    torch.cuda.synchronize()
    rep = Report(name, "fp64", "local_energy_complex", g)
    rep.add("re", np.abs(_np(e.real) - g["e_re"]), tol64(g["S"]))
    rep.add("im", np.abs(_np(e.imag) - g["e_im"]), tol64(g["S"]))
    rep.check()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("tag", ["fp64", "fp32"])
def test_energy_components(tag, name):
    """(c) energy_components: the parts sum to the total (8 u sum |row|, in the context dtype) and
    v_ee, v_en equal the oracle potentials to 4 n_terms u sum |term| (tests/test_gpu_components.py)."""
    dtype = DT[tag]
    s, g, ctx = _ctx(name, dtype)
    u = 2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24
    out = ctx.energy_components(_pos(g, dtype))
    torch.cuda.synchronize()
    TOT, KIN, KING, VEE, VEN, VNN, VPL, VPN = range(8)
    N, A = s.nelectrons, s.natoms
    pre = "" if dtype == torch.float64 else "r32_"
    v_ee, v_en = g[pre + "v_ee"], g[pre + "v_en"]
    got = _np(out)
    rep = Report(name, tag, "energy_components", g)
    rep.add("v_ee", np.abs(got[VEE] - v_ee), 4.0 * (N * (N - 1) // 2) * u * v_ee)
    rep.add("v_en", np.abs(got[VEN] - v_en), 4.0 * N * A * u * -v_en)
    ssum = out[KIN].clone()
    for r in (VEE, VEN, VNN, VPL, VPN):
        ssum = ssum + out[r]
    rep.add("closure", _np((out[TOT] - ssum).abs()), 8.0 * u * _np(out.abs()).sum(0))
    e_ref = g["e_l"] if dtype == torch.float64 else g["r32_e_l"]
    rep.add("total", np.abs(got[TOT] - e_ref), tol64(g["S"]) if dtype == torch.float64 else tol32(g["r32_S"]))
    rep.check()


@pytest.mark.parametrize("name", NAMES)
def test_parameter_gradient(name):
    """(d) logpsi_param_grad in fp64: error at most 1e-8 of each walker's largest component."""
    s, g, ctx = _ctx(name, torch.float64)
    O = _np(ctx.logpsi_param_grad(_pos(g, torch.float64)))
    ref = g["pgrad"]
    assert O.shape == ref.shape
    rep = Report(name, "fp64", "logpsi_param_grad", g)
    rep.add("rows", np.abs(O - ref), 1e-8 * np.abs(ref).max(axis=1, keepdims=True))
    rep.check()


def _sweep(ctx, g, sweep, dtype, rounded):
    """One host-draw sweep from the fixture's start; (x0, x1, moved [B, N])."""
    x0 = g[f"{sweep}_x0"]
    if rounded:
        x0 = x0.astype(np.float32).astype(np.float64)
    B = x0.shape[0]
    x = torch.tensor(x0, device="cuda", dtype=dtype).contiguous()
    ctx.mc_step(x, 1, TSTEP, gauss1=torch.tensor(g[f"{sweep}_g1"][None]), gauss2=torch.tensor(g[f"{sweep}_g2d"][None]),
                u=torch.tensor(g[f"{sweep}_u"][None]))
    torch.cuda.synchronize()
    x1 = _np(x)
    moved = np.any(x1.reshape(B, -1, 3) != _np(torch.tensor(x0, dtype=dtype)).reshape(B, -1, 3), axis=2)
    return x0, x1, moved, x


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("sweep", ["start", "land"])
def test_metropolis_sweep_fp64(sweep, name):
    """(e) mc_step, one host-draw sweep, fp64: from the close walkers (start), and from ordinary
    walkers whose electron-0 proposal lands at distance d (land: the proposal launch, not the walker
    launch, meets the close geometry).  Decisions equal the oracle's, positions within 1e-9."""
    s, g, ctx = _ctx(name, torch.float64)
    _, x1, moved, _ = _sweep(ctx, g, sweep, torch.float64, False)
    cond = g[f"{sweep}_cond"]
    rep = Report(name, "fp64", f"mc_step[{sweep}]", g)
    rep.add("decisions", (moved != cond).sum(axis=1).astype(float), np.full(cond.shape[0], 0.5))
    same = (moved == cond).all(axis=1, keepdims=True)
    rep.add("positions", np.where(same, np.abs(x1 - g[f"{sweep}_x1"]), np.inf), np.full((1, 1), 1e-9))
    rep.check()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("sweep", ["start", "land"])
def test_metropolis_sweep_fp32(sweep, name):
    """(e) fp32 against the fp64 kernels from the same float32-rounded start and host draws:
    everything finite, the accept count within max(1, B N / 100) of the fp64 count, walkers that
    took the same decisions within 1e-4; the fused and unfused limdrift reductions bitwise equal
    (|grad|^2 reaches 1e9 here: the mid word of the integer accumulators, limdrift.h)."""
    s, g, c64 = _ctx(name, torch.float64)
    _, _, c32 = _ctx(name, torch.float32)
    _, x64, m64, _ = _sweep(c64, g, sweep, torch.float64, True)
    _, x32, m32, t32 = _sweep(c32, g, sweep, torch.float32, True)
    assert np.isfinite(x32).all() and np.isfinite(x64).all()
    B, N = m64.shape
    rep = Report(name, "fp32", f"mc_step[{sweep}]", g)
    rep.note(f"accepts fp32 {int(m32.sum())} fp64 {int(m64.sum())} decisions flipped {int((m32 != m64).sum())}")
    assert abs(int(m32.sum()) - int(m64.sum())) <= max(1, B * N // 100), (m32.sum(), m64.sum())
    same = (m32 == m64).all(axis=1, keepdims=True)
    rep.add("positions", np.where(same, np.abs(x32 - x64), 0.0), np.full((1, 1), 1e-4))
    rep.check()
    c32.set_fuse_reduce(0)
    _, _, _, plain = _sweep(c32, g, sweep, torch.float32, True)
    c32.set_fuse_reduce(2)
    _, _, _, fused = _sweep(c32, g, sweep, torch.float32, True)
    assert torch.equal(plain, fused) and torch.equal(fused, t32)


@pytest.mark.parametrize("name", NAMES)
def test_dmc_drift_diffusion(name):
    """(f) dmc_drift_diffusion in fp64 from the close walkers, at the tolerance of
    tests/test_dmc.py::test_drift_diffusion_matches_oracle."""
    s, g, ctx = _ctx(name, torch.float64)
    x = _pos(g, torch.float64).contiguous()
    go, gn, td = ctx.dmc_drift_diffusion(x, TSTEP, gauss1=torch.tensor(g["start_g1"][None]),
                                         gauss2=torch.tensor(g["start_g2d"][None]), u=torch.tensor(g["start_u"][None]))
    torch.cuda.synchronize()
    rep = Report(name, "fp64", "dmc_drift_diffusion", g)
    rep.add("positions", np.abs(_np(x) - g["dd_x1"]), 1e-9 + 1e-9 * np.abs(g["dd_x1"]))
    rep.add("grad_eff_old", np.abs(_np(go) - g["dd_go"]), 1e-9 + 1e-8 * np.abs(g["dd_go"]))
    rep.add("grad_new_eff", np.abs(_np(gn) - g["dd_gn"]), 1e-9 + 1e-8 * np.abs(g["dd_gn"]))
    rep.check()
    rep.note(f"tdamp error {abs(td[2].item() - float(g['dd_tdamp'])):.3g}")
    assert abs(td[2].item() - float(g["dd_tdamp"])) < 1e-10


@pytest.mark.parametrize("tag", ["fp64", "fp32"])
def test_ecp_local_energy(tag):
    """(g) local_energy_ecp on C_ecp, an electron at distance d from the ECP centre, injected
    rotations: fp64 within tol64, fp32 within tol32 (S with the local pseudopotential in V); the
    proposal-reuse path equals the scratch path to 1e-10 max(S, 1) in fp64."""
    dtype = DT[tag]
    s, g, ctx = _ctx("C_ecp", dtype, ecp=True)
    x = _pos(g, dtype)
    rot = torch.tensor(g["rot"], device="cuda", dtype=dtype)
    e = ctx.local_energy_ecp(x, rot=rot)
    torch.cuda.synchronize()
    pre, tol = ("", tol64) if dtype == torch.float64 else ("r32_", tol32)
    S = g[pre + "pp_S"]
    rep = Report("C_ecp", tag, "local_energy_ecp", g)
    rep.add("re", np.abs(_np(e.real) - g[pre + "pp_e_re"]), tol(S))
    rep.add("im", np.abs(_np(e.imag) - g[pre + "pp_e_im"]), tol(S))
    if dtype == torch.float64:
        ctx.set_proposal_reuse(False)
        e2 = ctx.local_energy_ecp(x, rot=rot)
        torch.cuda.synchronize()
        rep.add("reuse_vs_scratch", np.abs((e - e2).cpu().numpy()), 1e-10 * np.maximum(S, 1.0))
    rep.check()
