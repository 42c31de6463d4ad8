"""Stochastic reconfiguration on the GPU: the Gram kernel (aiqmc_sr_gram) against the numpy fp64
Gram product with derived bounds, its structure (symmetry, reproducibility, accumulation), the
Fisher matrix and one SR step against the oracle's Jacobians, invariants of a step on the benched
systems in fp32, and the reference driver's call sequence (main/main_pp.py:160-206)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 17), (5, 16), (255, 33), (256, 64), (257, 65), (600, 130)]


def _inputs(B, P, dtype, seed):
    rng = np.random.default_rng(seed)
    npdt = np.float32 if dtype == torch.float32 else np.float64
    scale = rng.uniform(0.1, 4.0, size=P)
    o_re = (rng.normal(0.7, 1.0, size=(B, P)) * scale).astype(npdt)
    o_im = (rng.normal(-0.4, 1.0, size=(B, P)) * scale[::-1]).astype(npdt)
    c_re = (o_re.astype(np.float64).mean(axis=0) + 0.05 * scale * rng.normal(size=P)).astype(npdt)
    c_im = (o_im.astype(np.float64).mean(axis=0) + 0.05 * scale[::-1] * rng.normal(size=P)).astype(npdt)
    return o_re, o_im, c_re, c_im


def _dev(a):
    return None if a is None else torch.tensor(a, device="cuda")


def _split(out, P):
    v = out.cpu().numpy()
    return v[:P * P].reshape(P, P), v[P * P:P * P + P], v[P * P + P:P * P + 2 * P], v[P * P + 2 * P]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B,P", SHAPES)
def test_gram_matches_numpy(B, P, dtype):
    """fp64: 1e-12 (|A|^T |A|) + 1e-300 entrywise.  fp32: (SR_CHUNK + 2) 2^-24 (|A - c|^T |A - c|)
    entrywise -- a chain of SR_CHUNK fmaf's of products of operands that each carry the one
    rounding of the centring; the fp64 combination of the chunks is negligible against it.  The
    column sums hold to the same bounds with sum_b |.| in place of the product."""
    from aiqmc import _lib
    o_re, o_im, c_re, c_im = _inputs(B, P, dtype, 1000 * B + P)
    for cplx in (False, True):
        for centred in (False, True):
            oi = o_im if cplx else None
            cr, ci = (c_re, c_im if cplx else None) if centred else (None, None)
            out = _lib.sr_gram(_dev(o_re), _dev(oi), _dev(cr), _dev(ci))
            torch.cuda.synchronize()
            G, s_re, s_im, n = _split(out, P)
            a = o_re.astype(np.float64) - (cr.astype(np.float64) if centred else 0.0)
            b = (o_im.astype(np.float64) - (ci.astype(np.float64) if centred else 0.0)) if cplx else np.zeros_like(a)
            G_ref = a.T @ a + b.T @ b
            if dtype == torch.float64:
                A_re, A_im = np.abs(o_re), (np.abs(o_im) if cplx else np.zeros_like(a))
                bound = 1e-12 * (A_re.T @ A_re + A_im.T @ A_im) + 1e-300
                sb_re, sb_im = 1e-12 * A_re.sum(axis=0) + 1e-300, 1e-12 * A_im.sum(axis=0) + 1e-300
            else:
                u = (_lib.SR_CHUNK + 2) * 2.0 ** -24
                bound = u * (np.abs(a).T @ np.abs(a) + np.abs(b).T @ np.abs(b))
                sb_re, sb_im = u * np.abs(a).sum(axis=0), u * np.abs(b).sum(axis=0)
            tag = (B, P, dtype, cplx, centred)
            assert n == B, tag
            err = np.abs(G - G_ref)
            assert np.all(err <= bound), (tag, float((err / bound).max()))
            assert np.all(np.abs(s_re - a.sum(axis=0)) <= sb_re), tag
            assert np.all(np.abs(s_im - b.sum(axis=0)) <= sb_im), tag
            assert np.array_equal(G, G.T), tag


def test_gram_empty_batch_writes_and_adds_zeros():
    from aiqmc import _lib
    P = 70
    o = torch.zeros(0, P, dtype=torch.float32, device="cuda")
    out = _lib.sr_gram(o)
    assert float(out.abs().max()) == 0.0
    full = torch.full((P * P + 2 * P + 1,), 3.0, dtype=torch.float64, device="cuda")
    _lib.sr_gram(o, out=full, accumulate=True)
    assert bool((full == 3.0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_gram_structure(dtype):
    """Symmetric and reproducible to the bit; a batch of 2 SR_CHUNK walkers in two accumulated
    blocks equals the one call."""
    from aiqmc import _lib
    B, P = 2 * _lib.SR_CHUNK, 130
    o_re, o_im, c_re, c_im = (_dev(a) for a in _inputs(B, P, dtype, 77))
    one = _lib.sr_gram(o_re, o_im, c_re, c_im)
    two = _lib.sr_gram(o_re, o_im, c_re, c_im)
    h = _lib.SR_CHUNK
    acc = _lib.sr_gram(o_re[:h], o_im[:h], c_re, c_im)
    acc = _lib.sr_gram(o_re[h:], o_im[h:], c_re, c_im, out=acc, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(one, two)
    G = one[:P * P].reshape(P, P)
    assert torch.equal(G, G.T)
    np.testing.assert_allclose(acc.cpu().numpy(), one.cpu().numpy(), rtol=1e-13)
    with pytest.raises(ValueError):
        _lib.sr_gram(o_re, o_im[:h])
    with pytest.raises(ValueError):
        _lib.sr_gram(o_re, accumulate=True)


# -- the optimizer on real wavefunctions ----------------------------------------------------------

def _vmc(name, dtype, B, seed):
    from oracle import system
    from aiqmc.Energy import hamiltonian as H
    from aiqmc.Loss import loss as L
    from aiqmc.wavefunction_Ynlm import nn
    from aiqmc import systems
    s = system.make_system(name)
    network = systems.make_system(name).make_network()
    rng = np.random.default_rng(seed)
    params = system.init_params(rng, s, randomize_aux=True)
    pos = system.init_electrons(rng, s.atoms, s.charges, B, 1.0)
    data = nn.AINetData(positions=torch.tensor(pos, dtype=dtype, device="cuda").contiguous(), spins=s.spins,
                        atoms=s.atoms, charges=s.charges)
    le = H.local_energy(f=network.apply, charges=s.charges, nspins=s.spins)
    ev = L.make_loss(network=network.apply, local_energy=le, clip_local_energy=5.0, clip_from_median=False,
                     center_at_clipped_energy=True, complex_output=True)
    return s, network, params, pos, data, ev


_ORACLE_JAC = {}


def _oracle_jacobians(name, s, params, pos):
    """Computed once per system and shared (read-only) by the tests below."""
    if name not in _ORACLE_JAC:
        from oracle import loss as oloss, network as onet
        net = onet.Network(s)
        x = torch.tensor(pos)
        _ORACLE_JAC[name] = (oloss.logabs_param_grad(net, params, x), oloss.phase_param_grad(net, params, x))
    return _ORACLE_JAC[name]


def _cov(o):
    return np.cov(o, rowvar=False, bias=True)


@pytest.mark.parametrize("name", ["H2", "Be"])
def test_fisher_matches_oracle_covariance(name):
    """S against the covariance of the oracle's Jacobian rows: 1e-7 of max|S_ref| entrywise (the
    Jacobians themselves agree to 1e-8, tests/test_gpu_pgrad.py)."""
    from aiqmc.Optimizer import sr
    s, network, params, pos, data, ev = _vmc(name, torch.float64, 16, 41)
    Oa, Op = _oracle_jacobians(name, s, params, pos)
    for cplx in (False, True):
        S, n = sr.fisher(ev, params, data, cplx)
        torch.cuda.synchronize()
        S_ref = _cov(Oa) + (_cov(Op) if cplx else 0.0)
        assert float(n) == 16.0 and S.is_cuda and S.dtype == torch.float64
        assert np.abs(S.cpu().numpy() - S_ref).max() <= 1e-7 * np.abs(S_ref).max(), (name, cplx)


def _np_step(theta, g, S, lam, lr, norm_constraint):
    delta = np.linalg.solve(S + lam * np.eye(S.shape[0]), g)
    coef = min(1.0, np.sqrt(norm_constraint / (lr * lr * (delta @ g))))
    return theta - coef * lr * delta


def test_one_step_matches_numpy_rule():
    """Be, fp64, 64 walkers, damping 0.1: the new parameters against the rule in numpy, fed (a)
    with the device's own O, e_l and g (rtol 1e-9) and (b) with the oracle's Jacobians
    (10 kappa 1e-8 relative in the 2-norm, of the parameters and, stricter, of the update; kappa
    the condition number of the reference S + lambda I)."""
    from oracle import loss as oloss, system
    from aiqmc.Optimizer import sr
    s, network, params, pos, data, ev = _vmc("Be", torch.float64, 64, 5)
    lr, nc, lam = 0.05, 1e-3, 0.1
    opt = sr.Optimizer(ev, l2_reg=0.0, norm_constraint=nc, value_func_has_aux=True, value_func_has_rng=True,
                       learning_rate_schedule=lambda t: lr, curvature_ema=0.95, inverse_update_period=1,
                       min_damping=1e-4, num_burnin_steps=0)
    state = opt.init(params, 0, data)
    new_params, new_state, stats = opt.step(params, state, 0, data, momentum=0.0, damping=lam)
    torch.cuda.synchronize()
    theta = system.flatten_params(params)
    got = system.flatten_params(new_params)
    ctx = network.apply._aiqmc_network.bind(params, s.atoms, torch.float64)
    x = data.positions
    Oa, Op = ctx.logpsi_param_grad(x).cpu().numpy(), ctx.phase_param_grad(x).cpu().numpy()
    el = ctx.local_energy(x)[0].cpu().numpy()
    g_dev = stats["grad"].cpu().numpy()
    # (a) the device's own quantities
    _, _, g_a = oloss.energy_gradient(el, Oa, clip_scale=5.0)
    np.testing.assert_allclose(g_dev, g_a, rtol=1e-9, atol=1e-11 * np.abs(g_a).max())
    ref_a = _np_step(theta, g_dev, _cov(Oa) + _cov(Op), lam, lr, nc)
    np.testing.assert_allclose(got, ref_a, rtol=1e-9)
    # (b) the oracle's Jacobians
    Oa_o, Op_o = _oracle_jacobians("Be64", s, params, pos)
    _, _, g_b = oloss.energy_gradient(el, Oa_o, clip_scale=5.0)
    A = _cov(Oa_o) + _cov(Op_o) + lam * np.eye(theta.size)
    kappa = np.linalg.cond(A)
    ref_b = _np_step(theta, g_b, A - lam * np.eye(theta.size), lam, lr, nc)
    tol = 10.0 * kappa * 1e-8
    rel_theta = np.linalg.norm(got - ref_b) / np.linalg.norm(ref_b)
    rel_update = np.linalg.norm((got - theta) - (ref_b - theta)) / np.linalg.norm(ref_b - theta)
    print(f"kappa {kappa:.3e}  rel(theta) {rel_theta:.3e}  rel(update) {rel_update:.3e}  tol {tol:.3e}")
    assert rel_theta <= tol and rel_update <= tol, (rel_theta, rel_update, tol)
    assert new_state.step == 1 and float(stats["cholesky_info"]) == 0


@pytest.mark.parametrize("name", ["H2", "Be", "N2"])
def test_step_invariants_fp32(name):
    from aiqmc.Optimizer import sr
    from aiqmc.wavefunction_Ynlm.nn import flatten_params
    s, network, params, pos, data, ev = _vmc(name, torch.float32, 64, 9)
    lr, nc, lam = 0.05, 1e-3, 1e-3
    opt = sr.Optimizer(ev, norm_constraint=nc, learning_rate_schedule=lambda t: lr, curvature_ema=0.95,
                       min_damping=1e-4)
    state = opt.init(params, 0, data)
    new_params, state, stats = opt.step(params, state, 0, data, momentum=0.0, damping=lam)
    S, n = sr.fisher(ev, params, data, True)
    torch.cuda.synchronize()
    g = stats["grad"].cpu().numpy()
    d_theta = flatten_params(new_params) - flatten_params(params)
    assert np.isfinite(flatten_params(new_params)).all() and np.isfinite(g).all()
    assert bool(torch.isfinite(S).all()) and np.isfinite(float(stats["loss"]))
    assert float(g @ d_theta) < 0.0
    coef, dg = float(stats["coef"]), float(stats["delta_dot_grad"])
    assert dg > 0.0 and lr * lr * dg * coef * coef <= nc * (1.0 + 1e-6)
    ev_ = np.linalg.eigvalsh(S.cpu().numpy())
    assert ev_[0] >= -1e-5 * ev_[-1], (ev_[0], ev_[-1])
    assert torch.equal(S, S.T) and float(stats["cholesky_info"]) == 0


def test_reference_driver_sequence_c_ecp():
    """main/main_pp.py:160-206 with aiqmc.Optimizer.sr.Optimizer in the place of
    kfac_jax.Optimizer: Optimizer(...), init, make_kfac_training_step, then mc_step + step_kfac
    three times on the C atom with ccECP, 64 walkers."""
    from aiqmc import constants, systems
    from aiqmc.Energy import pphamiltonian
    from aiqmc.Loss import loss as L
    from aiqmc.Optimizer import sr
    from aiqmc.Optimizer.kfac import make_kfac_training_step
    from aiqmc.VMC import VMCmcstep
    from aiqmc.wavefunction_Ynlm import nn
    from aiqmc.initial_electrons_positions.init import init_electrons
    B = 64
    s = systems.make_system("C_ecp")
    network = s.make_network()
    params = network.init(4)
    e = systems.ccecp_tables("C_ecp")
    log_network = nn.make_log_network(network.apply)
    le = pphamiltonian.local_energy(f=network.apply, lognetwork=log_network, charges=s.charges, nspins=s.spins,
                                    rn_local=e.rn_local, local_coes=e.local_coes, local_exps=e.local_exps,
                                    rn_non_local=e.rn_non_local, non_local_coes=e.non_local_coes,
                                    non_local_exps=e.non_local_exps, natoms=1, nelectrons=4, ndim=3, list_l=2)
    evaluate_loss = L.make_loss(network=log_network, local_energy=le, clip_local_energy=5.0, clip_from_median=False,
                                center_at_clipped_energy=True, complex_output=True)

    def learning_rate_schedule(t_, rate=0.05, delay=1.0, decay=10000):
        return rate * (1.0 / (1.0 + (t_ / delay))) ** decay

    optimizer = sr.Optimizer(evaluate_loss, l2_reg=0.0, norm_constraint=0.001, value_func_has_aux=True,
                             value_func_has_rng=True, learning_rate_schedule=learning_rate_schedule,
                             curvature_ema=0.95, inverse_update_period=1, min_damping=1.0e-4, num_burnin_steps=0,
                             register_only_generic=False, estimation_mode='fisher_exact', multi_device=True,
                             pmap_axis_name=constants.PMAP_AXIS_NAME,
                             auto_register_kwargs=dict(graph_patterns=None))
    mc_step = VMCmcstep.main_monte_carlo(f=network.apply, tstep=0.05, ndim=3, nelectrons=4, nsteps=10, batch_size=B)
    pos, sp = init_electrons(17, None, s.atoms, s.charges, s.spins, B, 1.0)
    data = nn.AINetData(positions=pos.to("cuda", torch.float32).contiguous(), spins=sp, atoms=s.atoms,
                        charges=s.charges)
    opt_state = optimizer.init(params=params, rng=VMCmcstep.PhiloxKey(23, 0), batch=data)
    step_kfac = make_kfac_training_step(damping=0.001, optimizer=optimizer, reset_if_nan=False)
    first = nn.flatten_params(params)
    for t in range(3):
        data = mc_step(params, data, VMCmcstep.PhiloxKey(19, 10 * t))
        data, params, opt_state, loss, aux_data = step_kfac(data, params, opt_state, VMCmcstep.PhiloxKey(23, 1 + t))
    torch.cuda.synchronize()
    assert opt_state.step == 3 and np.isfinite(float(loss.real))
    template = network.init(4)
    got, want = nn.tree_leaves(params), nn.tree_leaves(template)
    assert sorted(params.keys()) == sorted(template.keys()) and len(got) == len(want)
    assert [tuple(l.shape) for l in got] == [tuple(np.shape(w)) for w in want]
    assert all(isinstance(l, torch.Tensor) and l.is_cuda and l.dtype == torch.float64 for l in got)
    assert all(l._base is got[0]._base for l in got)             # views of one device vector
    last = nn.flatten_params(params)
    assert np.isfinite(last).all() and np.abs(last - first).max() > 0.0
