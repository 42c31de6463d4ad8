"""HIP kernels vs the float64 oracle (golden fixtures + live oracle), through the C-ABI.

Tolerances (north_star: local energies within 1e-6 Ha of the reference on
identical walkers):
  float64 kernels: |dE_L| <= 1e-6 Ha absolute (observed ~1e-10), log|psi| and
                   grad to 1e-9 relative.
  float32 kernels: the reference's own dtype; E_L within 2e-4 relative of the
                   float64 oracle (fp32 cancellation in the Laplacian of a
                   14-electron determinant), log|psi| within 1e-5 relative.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SYSTEMS = ["H2", "Be", "N2", "Ne", "C2", "O2", "C"]   # (2,2) (4,1) (14,2) (10,1) (12,2) (16,2) (6,1)


def _ctx(name, dtype):
    from oracle import system
    from aiqmc import _lib
    s = system.make_system(name)
    return s, _lib.Context.for_system(s, dtype)


def _golden(golden_dir, name):
    return dict(np.load(os.path.join(golden_dir, f"{name}.npz")))


@pytest.mark.parametrize("name", SYSTEMS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_logpsi_grad_golden(golden_dir, name, dtype):
    g = _golden(golden_dir, name)
    s, ctx = _ctx(name, dtype)
    ctx.set_params(g["params_flat"])
    pos = torch.tensor(g["pos"], dtype=dtype, device="cuda")
    logabs, phase = ctx.logpsi(pos)
    la2, grad = ctx.logpsi_grad(pos)
    torch.cuda.synchronize()
    la, ph, gr = logabs.double().cpu().numpy(), phase.double().cpu().numpy(), grad.double().cpu().numpy()
    if dtype == torch.float64:
        np.testing.assert_allclose(la, g["logabs"], rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(np.cos(ph), np.cos(g["phase"]), atol=1e-9)
        np.testing.assert_allclose(np.sin(ph), np.sin(g["phase"]), atol=1e-9)
        np.testing.assert_allclose(gr, g["grad"], rtol=1e-8, atol=1e-8)
    else:
        np.testing.assert_allclose(la, g["logabs"], rtol=1e-5, atol=2e-4)
        scale = np.abs(g["grad"]).max(axis=1, keepdims=True)
        assert np.all(np.abs(gr - g["grad"]) <= 2e-3 * scale + 1e-4)
    np.testing.assert_array_equal(la2.cpu().numpy(), logabs.cpu().numpy())


@pytest.mark.parametrize("name", SYSTEMS)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_local_energy_golden(golden_dir, name, dtype):
    g = _golden(golden_dir, name)
    s, ctx = _ctx(name, dtype)
    ctx.set_params(g["params_flat"])
    pos = torch.tensor(g["pos"], dtype=dtype, device="cuda")
    el, la, gr = ctx.local_energy(pos, want_logabs=True, want_grad=True)
    torch.cuda.synchronize()
    el = el.double().cpu().numpy()
    if dtype == torch.float64:
        assert np.max(np.abs(el - g["e_l"])) <= 1e-6, (el, g["e_l"])
        np.testing.assert_allclose(la.cpu().numpy(), g["logabs"], rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(gr.cpu().numpy(), g["grad"], rtol=1e-8, atol=1e-8)
    else:
        np.testing.assert_allclose(el, g["e_l"], rtol=2e-4, atol=2e-3)


@pytest.mark.parametrize("name", SYSTEMS)
def test_mc_step_host_draws_golden(golden_dir, name):
    g = _golden(golden_dir, name)
    s, ctx = _ctx(name, torch.float64)
    ctx.set_params(g["params_flat"])
    N = s.nelectrons
    pos = torch.tensor(g["pos"], dtype=torch.float64, device="cuda").contiguous()
    g2 = torch.tensor(g["mc_gauss2"]).reshape(2, pos.shape[0], N, N, 3)
    idx = torch.arange(N)
    g2d = g2[:, :, idx, idx, :].contiguous()
    ctx.mc_step(pos, 2, float(g["mc_tstep"]), gauss1=torch.tensor(g["mc_gauss1"]), gauss2=g2d,
                u=torch.tensor(g["mc_u"]))
    torch.cuda.synchronize()
    np.testing.assert_allclose(pos.cpu().numpy(), g["mc_pos_out"], rtol=1e-9, atol=1e-9)
