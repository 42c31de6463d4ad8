"""Stochastic reconfiguration (SR): the second-order optimizer of the drop-in API, in the place
the reference's drivers give to ``kfac_jax.Optimizer`` (main/main_pp.py:160-189).

KFAC approximates the Fisher matrix of the wavefunction by Kronecker blocks.  The network here
has a few thousand parameters, so the matrix itself is affordable and is used EXACTLY:

    S = Cov_b(O_b) = <(O_re - c_re)(O_re - c_re)^T> + <(O_im - c_im)(O_im - c_im)^T>,

the real part of the quantum geometric tensor, with O_re = d log|psi| / d theta and O_im =
d phase / d theta the per-walker Jacobians (aiqmc_logpsi_param_grad / aiqmc_phase_param_grad
without weights; O_im only with ``complex_output``) and c their means over all walkers of all
ranks.  ``fisher`` forms it: the centre from one sum all-reduce of [sum O_re, sum O_im, n], the
Gram product sum_b (O_b - c)(O_b - c)^T on the matrix cores (aiqmc_sr_gram: fixed summation
order, float chunks of ``_lib.SR_CHUNK`` walkers combined in fp64, bitwise reproducible), one sum
all-reduce of [G, s_re, s_im, n], then S = G/n - (s_re s_re^T + s_im s_im^T)/n^2 in fp64 (exact
for any centre; the centre only keeps the float products small).  Walkers go through in blocks of
at most ``BLOCK`` so that the Jacobian of a large batch is never resident at once; with more than
one block the Jacobian pass runs once for the centre and once for the Gram product.

Update rule of ``Optimizer.step(params, state, rng, batch, momentum, damping)``, all in fp64 on
the device of the gradient:

    g      = value_and_pmean_grad(params, rng, batch) + l2_reg * theta
    E_t    = curvature_ema * E_{t-1} + (1 - curvature_ema) * S_t,   E_0 = 0
    Sbar_t = E_t / (1 - curvature_ema^t)            (bias-corrected; curvature_ema = 0: S_t itself)
    lambda = max(damping, min_damping)
    delta  = (Sbar_t + lambda I)^-1 g               (Cholesky factor, refreshed when
                                                     step % inverse_update_period == 0)
    lr     = learning_rate_schedule(step)           (step = 0, 1, ..: steps taken so far)
    coef   = min(1, sqrt(norm_constraint / (lr^2 delta^T g)))
    u_t    = momentum * u_{t-1} - coef * lr * delta,   u_0 = 0
    theta <- theta + u_t

``init`` runs ``num_burnin_steps`` curvature estimates on its batch (E and t advance, the
parameters do not move).  The step never changes its inputs: ``state`` and ``params`` of before
stay valid (Optimizer.kfac's NaN rollback keeps them by reference).  The new parameters are views
of one float64 device vector, as Optimizer.adam returns them.

The Jacobian pass runs twice per step (weighted inside the loss, per walker here).
"""
from __future__ import annotations

import dataclasses
from typing import Any, Callable, Optional

import torch

from .. import constants
from ..wavefunction_Ynlm.nn import as_positions, flatten_params_device, network_of

# walkers per Jacobian block: a multiple of _lib.SR_CHUNK (asserted on the device path), so that a
# batch cut into blocks sums in the same chunks as the batch in one piece
BLOCK = 4096


def _is_device(o: torch.Tensor) -> bool:
    return o.is_cuda and o.dtype in (torch.float32, torch.float64)


def _column_sums(o_re, o_im, P, dev):
    """[sum_b O_re (P), sum_b O_im (P), n] of one block, float64."""
    v = torch.zeros(2 * P + 1, dtype=torch.float64, device=dev)
    v[:P] = o_re.sum(dim=0, dtype=torch.float64)
    if o_im is not None:
        v[P:2 * P] = o_im.sum(dim=0, dtype=torch.float64)
    v[2 * P] = float(o_re.shape[0])
    return v


def _host_gram(o_re, o_im, c_re, c_im, out):
    """aiqmc_sr_gram restated in torch float64 (host/gloo ranks): adds one block into out."""
    P = o_re.shape[1]
    a = o_re.to(torch.float64) - c_re
    G = a.T @ a
    out[P * P:P * P + P] += a.sum(dim=0)
    if o_im is not None:
        b = o_im.to(torch.float64) - c_im
        G = G + b.T @ b
        out[P * P + P:P * P + 2 * P] += b.sum(dim=0)
    out[:P * P] += G.reshape(-1)
    out[P * P + 2 * P] += float(o_re.shape[0])


def fisher_from_jacobian(blocks: Callable[[], Any]):
    """(S [P, P] float64, n) from this rank's per-walker Jacobian.  ``blocks()`` returns an
    iterable of (o_re [b, P], o_im [b, P] or None) walker blocks; it is called once when it yields
    one block and twice otherwise (centre pass, Gram pass).  Device float32/float64 blocks run
    aiqmc_sr_gram, anything else the same formulas in torch float64."""
    sums = None
    kept, nblocks = None, 0
    for o_re, o_im in blocks():
        v = _column_sums(o_re, o_im, o_re.shape[1], o_re.device)
        sums = v if sums is None else sums + v
        kept = (o_re, o_im)
        nblocks += 1
    if sums is None:
        raise ValueError("fisher: no walkers")
    P = (sums.numel() - 1) // 2
    dev = sums.device
    constants.all_reduce_(sums)
    c_re = sums[:P] / sums[2 * P]
    c_im = sums[P:2 * P] / sums[2 * P]
    out = None
    again = [kept] if nblocks == 1 else blocks()   # one block: the Jacobian is still here
    kept = None
    for o_re, o_im in again:
        if _is_device(o_re):
            from .. import _lib
            assert BLOCK % _lib.SR_CHUNK == 0
            out = _lib.sr_gram(o_re, o_im, c_re, c_im if o_im is not None else None, out=out,
                               accumulate=out is not None)
        else:
            if out is None:
                out = torch.zeros(P * P + 2 * P + 1, dtype=torch.float64, device=dev)
            _host_gram(o_re, o_im, c_re, c_im, out)
    constants.all_reduce_(out)
    n = out[P * P + 2 * P]
    s_re, s_im = out[P * P:P * P + P] / n, out[P * P + P:P * P + 2 * P] / n
    S = out[:P * P].reshape(P, P) / n
    S = S - torch.outer(s_re, s_re) - torch.outer(s_im, s_im)
    return S, n


def fisher(evaluate_loss, params, data, complex_output: bool):
    """(S [P, P] float64 on the device, n): the exact Fisher matrix of the wavefunction over the
    walkers ``data.positions`` of all ranks (module docstring).  ``evaluate_loss`` is the
    ``make_loss`` result; its network's kernels give the per-walker Jacobians.  An
    ``evaluate_loss.per_walker_jacobian(params, data, lo, hi) -> (o_re, o_im or None)`` attribute
    replaces them (another wavefunction, or synthetic Jacobians on host ranks)."""
    pos = as_positions(data.positions)
    jac = getattr(evaluate_loss, "per_walker_jacobian", None)
    if jac is None:
        ctx, _ = network_of(evaluate_loss, "fisher").bind_positions(params, pos, data.atoms)
        x = pos.reshape(-1, pos.shape[-1])

        def jac(params_, data_, lo, hi):
            xb = x[lo:hi]
            return ctx.logpsi_param_grad(xb), (ctx.phase_param_grad(xb) if complex_output else None)
    B = pos.numel() // pos.shape[-1]

    def blocks():
        for lo in range(0, B, BLOCK):
            yield jac(params, data, lo, min(B, lo + BLOCK))
    return fisher_from_jacobian(blocks)


@dataclasses.dataclass(frozen=True)
class State:
    """Optimizer state; a step returns a new one and leaves the old one as it was."""
    step: int = 0                 # parameter updates taken (the schedule's argument)
    count: int = 0                # curvature estimates in the EMA (burn-in included)
    ema: Any = None               # E_t [P, P] float64
    weight: float = 0.0           # 1 - curvature_ema^count
    factor: Any = None            # Cholesky factor (lower) of Sbar + lambda I at the last refresh
    velocity: Any = None          # u_t [P] float64


class Optimizer:
    """The keyword set the reference hands to ``kfac_jax.Optimizer`` (main_pp.py:160-176), driving
    the exact-Fisher update of the module docstring.  ``value_and_grad_func`` is the ``make_loss``
    result (the reference passes ``jax.value_and_grad`` of it).  ``value_func_has_aux``,
    ``value_func_has_rng``, ``register_only_generic``, ``estimation_mode``, ``multi_device``,
    ``pmap_axis_name`` and ``auto_register_kwargs`` are accepted and ignored: they configure KFAC's
    block registration and pmap, which have no counterpart here.  ``complex_output`` (not a
    kfac_jax keyword) overrides the loss's own setting of whether the phase Jacobian enters S."""

    def __init__(self, value_and_grad_func, l2_reg: float = 0.0, norm_constraint: Optional[float] = None,
                 value_func_has_aux: bool = False, value_func_has_rng: bool = False,
                 learning_rate_schedule: Optional[Callable] = None, curvature_ema: float = 0.95,
                 inverse_update_period: int = 1, min_damping: float = 1e-8, num_burnin_steps: int = 0,
                 register_only_generic: bool = False, estimation_mode: str = "fisher_exact",
                 multi_device: bool = False, pmap_axis_name: Optional[str] = None,
                 auto_register_kwargs: Optional[dict] = None, complex_output: Optional[bool] = None):
        del value_func_has_aux, value_func_has_rng, register_only_generic, estimation_mode
        del multi_device, pmap_axis_name, auto_register_kwargs
        self._vg = getattr(value_and_grad_func, "value_and_pmean_grad", None)
        if self._vg is None:
            raise TypeError("Optimizer: the first argument must come from aiqmc.Loss.loss.make_loss")
        if learning_rate_schedule is None:
            raise ValueError("Optimizer: learning_rate_schedule is required")
        if not 0.0 <= curvature_ema < 1.0:
            raise ValueError("Optimizer: curvature_ema must be in [0, 1)")
        if inverse_update_period < 1:
            raise ValueError("Optimizer: inverse_update_period must be >= 1")
        self._loss = value_and_grad_func
        if complex_output is None:
            complex_output = getattr(value_and_grad_func, "complex_output", None)
        if complex_output is None:
            raise TypeError("Optimizer: the loss does not say whether it is complex_output; pass complex_output=")
        self.complex_output = bool(complex_output)
        self.l2_reg = float(l2_reg)
        self.norm_constraint = None if norm_constraint is None else float(norm_constraint)
        self.learning_rate_schedule = learning_rate_schedule
        self.curvature_ema = float(curvature_ema)
        self.inverse_update_period = int(inverse_update_period)
        self.min_damping = float(min_damping)
        self.num_burnin_steps = int(num_burnin_steps)

    def _curvature(self, state: State, params, batch) -> State:
        S, _ = fisher(self._loss, params, batch, self.complex_output)
        b = self.curvature_ema
        ema = (1.0 - b) * S if state.ema is None else b * state.ema + (1.0 - b) * S
        return dataclasses.replace(state, ema=ema, weight=b * state.weight + (1.0 - b), count=state.count + 1)

    def init(self, params, rng, batch) -> State:
        del rng
        state = State()
        for _ in range(self.num_burnin_steps):
            state = self._curvature(state, params, batch)
        return state

    def step(self, params, state: State, rng, batch, momentum=0.0, damping=0.0):
        """One update: (new params, new state, stats).  stats: 'loss', 'aux' of the loss, and the
        step's own numbers ('step', 'learning_rate', 'damping', device scalars 'coef' and
        'delta_dot_grad', the device vectors 'grad' (g) and 'update' (u_t), 'cholesky_info')."""
        (loss, aux), grad = self._vg(params, rng, batch)
        theta = flatten_params_device(params, grad.device)
        g = grad.detach().to(torch.float64)
        if self.l2_reg != 0.0:
            g = g + self.l2_reg * theta
        state = self._curvature(state, params, batch)
        lam = max(float(damping), self.min_damping)
        factor, info = state.factor, None
        if factor is None or state.step % self.inverse_update_period == 0:
            A = state.ema / state.weight
            A.diagonal().add_(lam)
            factor, info = torch.linalg.cholesky_ex(A)
        delta = torch.cholesky_solve(g[:, None], factor)[:, 0]
        lr = float(self.learning_rate_schedule(state.step))
        dg = torch.dot(delta, g)
        if self.norm_constraint is not None:
            coef = torch.clamp(torch.sqrt(self.norm_constraint / (lr * lr * dg)), max=1.0)
        else:
            coef = torch.ones((), dtype=torch.float64, device=g.device)
        u = -(coef * lr) * delta
        if state.velocity is not None and float(momentum) != 0.0:
            u = float(momentum) * state.velocity + u
        new_flat = (theta + u).detach()
        new_state = dataclasses.replace(state, step=state.step + 1, factor=factor, velocity=u)
        stats = {"loss": loss, "aux": aux, "step": state.step, "learning_rate": lr, "damping": lam, "coef": coef,
                 "delta_dot_grad": dg, "grad": g, "update": u, "cholesky_info": info}
        return self._loss.unflatten(params, new_flat), new_state, stats
