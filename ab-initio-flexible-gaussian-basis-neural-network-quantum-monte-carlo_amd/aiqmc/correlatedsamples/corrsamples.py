"""Space-warp coordinate transform (drop-in for AIQMCrelease3/correlatedsamples/corrsamples.py).

``correlated_samples(atoms, new_atoms, pos)`` has the reference's signature (corrsamples.py:23-47)
and result for one configuration ``pos [3N]``: every electron follows the nuclei with the weights
of Filippi and Umrigar,

    r' = r + sum_a w_a (R'_a - R_a),   w_a = r_a^-4 / sum_b r_b^-4,   r_a = |r - R_a|.

It also takes a batch ``pos [B, 3N]`` and several geometries ``new_atoms [M, A, 3]``; the result is
``[3N]``, ``[B, 3N]``, ``[M, 3N]`` or ``[M, B, 3N]`` accordingly.  Pure torch on the device and in
the dtype of ``pos`` (the geometry difference is formed in float64), differentiable, and with the
forms the HIP launch ``aiqmc_space_warp`` uses, which stay finite next to a nucleus:

* w_a = q_a / sum_b q_b with q_a = (r_min / r_a)^4, r_min = min_a r_a (r^-4 itself overflows float32
  below r ~ 2e-10); for r_min = 0 the weight is 1/k on the k atoms at zero distance;
* the displacement is evaluated as dR_n + sum_a w_a (dR_a - dR_n), n the nearest atom: equal because
  sum_a w_a = 1, and a rigid translation of all atoms moves every electron by exactly that vector;
* grad w_a = 4 w_a sum_{b != a} w_b (g_b - g_a), g_a = (r - R_a) / r_a^2 (0 for r_min = 0): the
  form sum_b w_b g_b - g_a cancels catastrophically next to a nucleus.
"""
from __future__ import annotations

import numpy as np
import torch


def _tensor(x, like: torch.Tensor = None, dtype=None) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if like is not None:
        t = t.to(like.device)
    return t if dtype is None else t.to(dtype)


def _shapes(atoms, new_atoms, pos):
    """(atoms [A,3] f64, dR [M,A,3] f64, pos [B,3N], squeeze_m, squeeze_b)."""
    p = _tensor(pos)
    if not p.is_floating_point():
        p = p.to(torch.float64)
    a = _tensor(atoms, p, torch.float64).reshape(-1, 3)
    na = _tensor(new_atoms, p, torch.float64)
    sq_m, sq_b = na.dim() == 2, p.dim() == 1
    na = na.reshape(-1, a.shape[0], 3)
    p2 = p.reshape(-1, p.shape[-1])
    if p2.shape[-1] % 3:
        raise ValueError("positions must hold 3N coordinates")
    return a, na - a[None], p2, sq_m, sq_b


def warp_terms(atoms: torch.Tensor, dR: torch.Tensor, pos: torch.Tensor):
    """For atoms [A,3] and dR [M,A,3] (float64) and pos [B,3N]: the electron positions x [B,N,3],
    the nearest atom's displacement Dn [M,B,N,3], the relative displacements rel [M,B,N,A,3] =
    dR_a - dR_n (both cast to the dtype of pos), the weights w [B,N,A] and their gradients
    gw [B,N,A,3]."""
    B = pos.shape[0]
    dt = pos.dtype
    x = pos.reshape(B, -1, 3)
    d = x[:, :, None, :] - atoms.to(dt)[None, None]
    r2 = (d * d).sum(-1)
    zero = r2 == 0
    r2s = torch.where(zero, torch.ones_like(r2), r2)
    rs = torch.sqrt(r2s)
    r = torch.where(zero, torch.zeros_like(r2), rs)
    rmin, nn = r.min(dim=-1)
    on = (rmin == 0)[..., None]
    t = rmin[..., None] / rs
    t2 = t * t
    q = torch.where(on, zero.to(dt), t2 * t2)
    w = q / q.sum(-1, keepdim=True)
    Dn = dR[:, nn]                                            # [M,B,N,3]
    rel = (dR[:, None, None] - Dn[:, :, :, None, :]).to(dt)   # [M,B,N,A,3]
    g = d / r2s[..., None]
    A = atoms.shape[0]
    off = ~torch.eye(A, dtype=torch.bool, device=pos.device)
    pair = g[:, :, None, :, :] - g[:, :, :, None, :]          # [B,N,a,b,3] = g_b - g_a
    pair = torch.where(off[None, None, :, :, None], pair, torch.zeros_like(pair))
    G = (w[:, :, None, :, None] * pair).sum(-2)
    gw = torch.where(on[..., None], torch.zeros_like(G), 4.0 * w[..., None] * G)
    return x, Dn.to(dt), rel, w, gw


def correlated_samples(atoms, new_atoms, pos):
    """See the module docstring (corrsamples.py:23-47)."""
    a, dR, p, sq_m, sq_b = _shapes(atoms, new_atoms, pos)
    x, Dn, rel, w, _ = warp_terms(a, dR, p)
    mv = (w[None, ..., None] * rel).sum(-2)
    out = (x[None] + (Dn + mv)).reshape(dR.shape[0], p.shape[0], -1)
    if sq_b:
        out = out[:, 0]
    return out[0] if sq_m else out
