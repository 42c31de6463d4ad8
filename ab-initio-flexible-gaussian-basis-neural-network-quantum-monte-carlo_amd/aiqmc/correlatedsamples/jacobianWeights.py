"""Jacobian of the space-warp transform (AIQMCrelease3/correlatedsamples/jacobianWeights.py).

``weights_jacobian(pos, atoms, new_atoms)`` has the reference's signature (jacobianWeights.py:22)
and returns prod_i det J_i, the determinant of d x' / d x of ``corrsamples.correlated_samples``:
the transform moves every electron on its own, so the 3N x 3N Jacobian is block diagonal with

    J_i[k][l] = delta_kl + sum_a (R'_a - R_a)[k] d_l w_a(r_i),
    grad w_a  = 4 w_a sum_{b != a} w_b (g_b - g_a),   g_a = (r - R_a) / |r - R_a|^2,

and the 3 x 3 determinants in closed form.  ``log_weights_jacobian`` returns
sum_i log|det J_i| (electrons added in ascending order), what the estimator and the HIP launch
``aiqmc_space_warp`` use.  Nothing is clamped: a singular block gives 0 (log: -inf).

Departure from the reference: its function carries a "to be continued" docstring and multiplies,
per Cartesian component, sum_a dR_a[0] c_a / sum_a c_a + 1 with c_a = -4 |x - X_a|^-5 (1 - X_a)
(jacobianWeights.py:29-47): ``1 - atoms`` is a coordinate, not a derivative, only dR's x component
enters, and the mixed derivatives are missing.  It is not the Jacobian of the transform (the
autograd test in tests/test_corrsamples_host.py is what this one is held to), so it is not
reproduced.

Batched like ``correlated_samples``: pos [3N] or [B, 3N], new_atoms [A, 3] or [M, A, 3] -> a
scalar, [B], [M] or [M, B].
"""
from __future__ import annotations

import torch

from .corrsamples import _shapes, warp_terms


def block_determinants(pos, atoms, new_atoms):
    """det J_i for every geometry, walker and electron: [M, B, N] (no squeezing), plus the flags
    (single geometry, single configuration)."""
    a, dR, p, sq_m, sq_b = _shapes(atoms, new_atoms, pos)
    _, _, rel, _, gw = warp_terms(a, dR, p)
    J = torch.einsum("mbnak,bnal->mbnkl", rel, gw)
    J = J + torch.eye(3, dtype=J.dtype, device=J.device)
    det = (J[..., 0, 0] * (J[..., 1, 1] * J[..., 2, 2] - J[..., 1, 2] * J[..., 2, 1])
           - J[..., 0, 1] * (J[..., 1, 0] * J[..., 2, 2] - J[..., 1, 2] * J[..., 2, 0])
           + J[..., 0, 2] * (J[..., 1, 0] * J[..., 2, 1] - J[..., 1, 1] * J[..., 2, 0]))
    return det, sq_m, sq_b


def _squeeze(v, sq_m, sq_b):
    if sq_b:
        v = v[:, 0]
    return v[0] if sq_m else v


def weights_jacobian(pos, atoms, new_atoms):
    """prod_i det J_i of the space warp (see the module docstring)."""
    det, sq_m, sq_b = block_determinants(pos, atoms, new_atoms)
    return _squeeze(det.prod(-1), sq_m, sq_b)


def log_weights_jacobian(pos, atoms, new_atoms):
    """sum_i log|det J_i|, electrons in ascending slot order."""
    det, sq_m, sq_b = block_determinants(pos, atoms, new_atoms)
    ld = torch.log(torch.abs(det))
    s = ld[..., 0]
    for i in range(1, ld.shape[-1]):
        s = s + ld[..., i]
    return _squeeze(s, sq_m, sq_b)
