"""Stochastic reconfiguration (aiqmc.Optimizer.sr / .kfac) without a GPU: the exported Gram entry
point, the Fisher-matrix formulas on host tensors, the update rule against a numpy restatement
written here, the NaN rollback of the training step, and two gloo ranks against the concatenated
batch.

The loss is a stand-in with the attributes of a ``make_loss`` result that the optimizer reads
(``value_and_pmean_grad``, ``unflatten``, ``complex_output``) plus synthetic per-walker Jacobians
(``per_walker_jacobian``): loss = mean e, g = (2/B) sum_b (e_b - mean e) O_re_b, pmean'd.
"""
import math
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import support
from conftest import ROOT

P = 23


class StubLoss:
    """What Optimizer.sr reads of a make_loss result, on synthetic host data."""

    def __init__(self, complex_output=True):
        self.complex_output = complex_output

    def value_and_pmean_grad(self, params, key, data):
        from aiqmc import constants
        e, O = data.e, data.o_re
        loss = constants.pmean(e.mean())
        g = constants.pmean((2.0 / e.numel()) * ((e - loss) @ O))
        return (loss, "aux"), g

    def per_walker_jacobian(self, params, data, lo, hi):
        return data.o_re[lo:hi], (data.o_im[lo:hi] if self.complex_output else None)

    def unflatten(self, params, flat):
        from aiqmc.Loss.loss import _unflatten_like
        return _unflatten_like(params, flat)


def _batch(seed, B=96, dtype=np.float64, nan=False):
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.2, 3.0, size=P)
    e = rng.normal(-14.6, 0.5, size=B)
    if nan:
        e[5] = np.nan
    return types.SimpleNamespace(positions=torch.zeros(B, 3, dtype=torch.float64), atoms=None,
                                 e=torch.tensor(e),
                                 o_re=torch.tensor((rng.normal(0.3, 1.0, size=(B, P)) * scale).astype(dtype)),
                                 o_im=torch.tensor((rng.normal(-0.1, 1.0, size=(B, P)) * scale[::-1]).astype(dtype)))


def _slice(d, lo, hi):
    return types.SimpleNamespace(positions=d.positions[lo:hi], atoms=None, e=d.e[lo:hi], o_re=d.o_re[lo:hi],
                                 o_im=d.o_im[lo:hi])


def _params(seed=3):
    rng = np.random.default_rng(seed)
    return {"a": rng.normal(size=(4, 3)), "b": [rng.normal(size=(5,)), rng.normal(size=(2, 3))]}   # 12 + 5 + 6 = P


def _flat(params):
    from aiqmc.wavefunction_Ynlm.nn import flatten_params
    return flatten_params(params)


def _np_cov(o_re, o_im=None):
    a = np.asarray(o_re, np.float64)
    S = np.cov(a, rowvar=False, bias=True)
    if o_im is not None:
        S = S + np.cov(np.asarray(o_im, np.float64), rowvar=False, bias=True)
    return S


def _assert_cov_close(S, o_re, o_im, S_ref, rtol=1e-12):
    """rtol entrywise, plus a few ulps of the entry's own terms: S_ij is a mean of products
    a_i a_j that cancel, and each product is rounded at 2^-53 |a_i a_j|, so an entry that cancels
    to nearly zero is known only to ~2^-52 mean|a_i a_j| <= 2^-52 sqrt(M_ii M_jj), M the (uncentred)
    second moments."""
    m = np.mean(np.asarray(o_re, np.float64) ** 2, axis=0)
    if o_im is not None:
        m = m + np.mean(np.asarray(o_im, np.float64) ** 2, axis=0)
    atol = 8 * 2.0 ** -52 * np.sqrt(np.outer(m, m))
    err = np.abs(np.asarray(S) - S_ref)
    assert np.all(err <= rtol * np.abs(S_ref) + atol), float((err / (rtol * np.abs(S_ref) + atol)).max())


def test_gram_symbol_is_exported_and_resolves():
    from aiqmc import _lib
    assert "aiqmc_sr_gram" in _lib.EXPORTED_SYMBOLS
    assert _lib.load().aiqmc_sr_gram is not None
    hdr = open(os.path.join(ROOT, "include", "aiqmc.h")).read()
    assert int(re.search(r"#define\s+AIQMC_SR_CHUNK\s+(\d+)", hdr).group(1)) == _lib.SR_CHUNK
    assert _lib.SR_CHUNK % 4 == 0


def test_modules_import():
    from aiqmc.Optimizer import kfac, sr
    assert callable(kfac.make_kfac_training_step) and callable(sr.fisher) and callable(sr.Optimizer)
    assert sr.BLOCK <= 4096


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("block", [4096, 32])
def test_host_fisher_equals_numpy_cov(cplx, dtype, block, monkeypatch):
    """One block and several (96 walkers in blocks of 32: the two-pass path)."""
    from aiqmc.Optimizer import sr
    monkeypatch.setattr(sr, "BLOCK", block)
    d = _batch(11, dtype=dtype)
    S, n = sr.fisher(StubLoss(cplx), _params(), d, cplx)
    assert S.dtype == torch.float64 and float(n) == 96.0
    oi = d.o_im.numpy() if cplx else None
    _assert_cov_close(S.numpy(), d.o_re.numpy(), oi, _np_cov(d.o_re.numpy(), oi))


def _np_rule(theta, batches, *, l2_reg, norm_constraint, lr, ema, period, min_damping, momentum, damping,
             burnin=0, burn_batch=None):
    """The update rule of the sr module docstring, restated."""
    E, w, u, L = np.zeros((P, P)), 0.0, np.zeros(P), None
    for _ in range(burnin):
        E = ema * E + (1 - ema) * _np_cov(burn_batch.o_re.numpy(), burn_batch.o_im.numpy())
        w = ema * w + (1 - ema)
    out = []
    for t, d in enumerate(batches):
        e, O = d.e.numpy(), d.o_re.numpy()
        g = (2.0 / e.size) * ((e - e.mean()) @ O) + l2_reg * theta
        E = ema * E + (1 - ema) * _np_cov(d.o_re.numpy(), d.o_im.numpy())
        w = ema * w + (1 - ema)
        lam = max(damping, min_damping)
        if t % period == 0:
            L = np.linalg.cholesky(E / w + lam * np.eye(P))
        delta = np.linalg.solve(L.T, np.linalg.solve(L, g))
        coef = 1.0 if norm_constraint is None else min(1.0, math.sqrt(norm_constraint / (lr(t) ** 2 * (delta @ g))))
        u = momentum * u - coef * lr(t) * delta
        theta = theta + u
        out.append((theta.copy(), coef, g))
    return out


RULES = {
    "constraint_active": dict(l2_reg=0.0, norm_constraint=1e-6, ema=0.0, period=1, min_damping=1e-4, momentum=0.0,
                              damping=1e-3),
    "constraint_inactive": dict(l2_reg=0.0, norm_constraint=1e3, ema=0.0, period=1, min_damping=1e-4, momentum=0.0,
                                damping=1e-3),
    "no_constraint": dict(l2_reg=0.0, norm_constraint=None, ema=0.0, period=1, min_damping=1e-4, momentum=0.0,
                          damping=1e-3),
    "ema_momentum": dict(l2_reg=0.0, norm_constraint=1e-2, ema=0.95, period=1, min_damping=1e-4, momentum=0.7,
                         damping=1e-2),
    "min_damping_floor": dict(l2_reg=0.0, norm_constraint=1e-2, ema=0.5, period=1, min_damping=0.3, momentum=0.0,
                              damping=1e-6),
    "l2_reg": dict(l2_reg=0.25, norm_constraint=1e-2, ema=0.5, period=1, min_damping=1e-4, momentum=0.3,
                   damping=1e-2),
    "stale_factor": dict(l2_reg=0.0, norm_constraint=1e-2, ema=0.9, period=2, min_damping=1e-4, momentum=0.0,
                         damping=1e-2),
    "burnin": dict(l2_reg=0.0, norm_constraint=1e-2, ema=0.9, period=1, min_damping=1e-4, momentum=0.0,
                   damping=1e-2, burnin=2),
}


@pytest.mark.parametrize("name", sorted(RULES))
def test_update_rule_equals_numpy_restatement(name):
    from aiqmc.Optimizer import sr
    r = dict(RULES[name])
    lr = lambda t: 0.05 / (1.0 + t)
    burnin = r.pop("burnin", 0)
    opt = sr.Optimizer(StubLoss(True), l2_reg=r["l2_reg"], norm_constraint=r["norm_constraint"],
                       value_func_has_aux=True, value_func_has_rng=True, learning_rate_schedule=lr,
                       curvature_ema=r["ema"], inverse_update_period=r["period"], min_damping=r["min_damping"],
                       num_burnin_steps=burnin, register_only_generic=False, estimation_mode="fisher_exact",
                       multi_device=True, pmap_axis_name="qmc_pmap_axis", auto_register_kwargs=dict(graph_patterns=()))
    batches = [_batch(20 + t) for t in range(3)]
    params = _params()
    ref = _np_rule(_flat(params), batches, lr=lr, burnin=burnin, burn_batch=batches[0], **r)
    state = opt.init(params, None, batches[0])
    assert state.step == 0 and state.count == burnin
    coefs = []
    for t, d in enumerate(batches):
        old_flat = _flat(params).copy()
        new_params, new_state, stats = opt.step(params, state, None, d, momentum=r["momentum"], damping=r["damping"])
        np.testing.assert_array_equal(_flat(params), old_flat)        # the inputs are left as they were
        assert state.step == t and new_state.step == t + 1
        assert stats["aux"] == "aux" and abs(float(stats["loss"]) - float(d.e.mean())) < 1e-13
        # a sum of 96 products in another order: rounding of the size of the largest entry
        np.testing.assert_allclose(stats["grad"].numpy(), ref[t][2], rtol=1e-12, atol=1e-13 * np.abs(ref[t][2]).max())
        np.testing.assert_allclose(_flat(new_params), ref[t][0], rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(float(stats["coef"]), ref[t][1], rtol=1e-11)
        leaves = [new_params["a"], *new_params["b"]]
        assert all(isinstance(l, torch.Tensor) and l.dtype == torch.float64 for l in leaves)
        assert [tuple(l.shape) for l in leaves] == [(4, 3), (5,), (2, 3)]
        assert all(l._base is leaves[0]._base for l in leaves)        # views of one vector
        coefs.append(ref[t][1])
        params, state = new_params, new_state
    if name == "constraint_active":
        assert all(c < 1.0 for c in coefs)
    if name == "constraint_inactive":
        assert all(c == 1.0 for c in coefs)


def test_optimizer_needs_a_make_loss_result_and_a_schedule():
    from aiqmc.Optimizer import sr
    with pytest.raises(TypeError):
        sr.Optimizer(lambda p, k, d: 0.0, learning_rate_schedule=lambda t: 0.1)
    with pytest.raises(ValueError):
        sr.Optimizer(StubLoss(True))


@pytest.mark.parametrize("reset", [True, False])
def test_training_step_nan_rollback(reset):
    from aiqmc.Optimizer import kfac, sr
    opt = sr.Optimizer(StubLoss(True), norm_constraint=1e-3, learning_rate_schedule=lambda t: 0.05,
                       curvature_ema=0.9, min_damping=1e-4)
    step = kfac.make_kfac_training_step(damping=1e-3, optimizer=opt, reset_if_nan=reset)
    params = _params()
    state = opt.init(params, None, _batch(30))
    d0 = _batch(30)
    data, p1, s1, loss, aux = step(d0, params, state, None)
    assert data is d0 and aux == "aux" and s1.step == 1 and math.isfinite(float(loss))
    assert np.abs(_flat(p1) - _flat(params)).max() > 0
    _, p2, s2, loss2, _ = step(_batch(31, nan=True), p1, s1, None)
    assert math.isnan(float(loss2))
    if reset:
        assert p2 is p1 and s2 is s1
        _, p3, s3, loss3, _ = step(_batch(32), p2, s2, None)          # training goes on from the kept state
        assert s3.step == 2 and np.isfinite(_flat(p3)).all() and math.isfinite(float(loss3))
    else:
        assert np.isnan(_flat(p2)).any() and s2.step == 2


# -- two gloo ranks against the concatenated batch -----------------------------------------------

B_RANK = 48
OPT_KW = dict(norm_constraint=1e-2, curvature_ema=0.9, min_damping=1e-4, l2_reg=0.01)


def _run_steps(batches):
    from aiqmc.Optimizer import sr
    loss = StubLoss(True)
    opt = sr.Optimizer(loss, learning_rate_schedule=lambda t: 0.05, **OPT_KW)
    params = _params()
    state = opt.init(params, None, batches[0])
    S, n = sr.fisher(loss, params, batches[0], True)
    flats = []
    for d in batches:
        params, state, _ = opt.step(params, state, None, d, momentum=0.5, damping=1e-2)
        flats.append(_flat(params))
    return S.numpy(), float(n), flats


def _worker(rank, world, port, q):
    import sys
    from conftest import PKG
    sys.path.insert(0, PKG)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from aiqmc import constants
    c0 = constants.ALLREDUCE_CALLS
    from aiqmc.Optimizer import sr
    full = _batch(40, B=B_RANK * world)
    S, n = sr.fisher(StubLoss(True), _params(), _slice(full, B_RANK * rank, B_RANK * (rank + 1)), True)
    calls = constants.ALLREDUCE_CALLS - c0
    batches = [_slice(_batch(40 + t, B=B_RANK * world), B_RANK * rank, B_RANK * (rank + 1)) for t in range(2)]
    q.put((rank, _run_steps(batches), calls))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_the_concatenated_batch():
    world = 2
    port = support.free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    S_ref, n_ref, flats_ref = _run_steps([_batch(40 + t, B=B_RANK * world) for t in range(2)])
    assert n_ref == B_RANK * world
    for rank, (S, n, flats), calls in res:
        assert calls == 2                      # the centre, then [G, s_re, s_im, n]
        assert n == n_ref
        full = _batch(40, B=B_RANK * world)
        _assert_cov_close(S, full.o_re.numpy(), full.o_im.numpy(), S_ref)
        for a, b in zip(flats, flats_ref):
            np.testing.assert_allclose(a, b, rtol=1e-12)
