"""ctypes binding of libaiqmc_hip.so (the C-ABI declared in include/aiqmc.h).

The product path has no CPU fallback: if the shared library is missing or a
call fails, this module raises.  torch is imported before the library is
loaded so that the process uses ONE HIP runtime (torch's libamdhip64.so.7
satisfies the library's NEEDED entry by SONAME).
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import functools
import os
from typing import Optional, Sequence

import numpy as np
import torch  # noqa: F401  (must precede loading the HIP library)

AIQMC_F32 = 0
AIQMC_F64 = 1
AIQMC_EHIP = -3
AIQMC_RNG_HOST = 0
AIQMC_RNG_PHILOX = 1

# AIQMC_LIB_VARIANT=phaseprof selects the diagnostics build (make -C csrc phaseprof)
_VARIANT = os.environ.get("AIQMC_LIB_VARIANT", "")
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                        "libaiqmc_hip.so" if not _VARIANT else f"libaiqmc_hip_{_VARIANT}.so")

PROF_MC_PROPOSAL = 0   # proposal value+gradient launches of aiqmc_mc_step
PROF_MC_WALKER = 1     # walker gradient launches of aiqmc_mc_step
PROF_LOCAL_ENERGY = 2  # aiqmc_local_energy launches
PROF_ECP_QUAD = 3      # value-only launches over the ECP quadrature configurations
ECP_NQ = 50            # quadrature points per (electron, atom) (pseudopotential.py:181-225)
SR_CHUNK = 256         # AIQMC_SR_CHUNK: walkers summed in the operand dtype before the fp64 combine (aiqmc_sr_gram)


class AiqmcCfg(ctypes.Structure):
    _fields_ = [
        ("nelectrons", ctypes.c_int32),
        ("natoms", ctypes.c_int32),
        ("nspins", ctypes.c_int32 * 2),
        ("dtype", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("atoms", ctypes.POINTER(ctypes.c_double)),
        ("charges", ctypes.POINTER(ctypes.c_double)),
        ("spin_up_indices", ctypes.POINTER(ctypes.c_int32)),
        ("spin_down_indices", ctypes.POINTER(ctypes.c_int32)),
        ("parallel_indices", ctypes.POINTER(ctypes.c_int32)),
        ("n_parallel", ctypes.c_int32),
        ("antiparallel_indices", ctypes.POINTER(ctypes.c_int32)),
        ("n_antiparallel", ctypes.c_int32),
        ("hidden_dims", (ctypes.c_int32 * 2) * 3),
        ("hidden_dims_ynlm", ctypes.c_int32 * 3),
    ]


class AiqmcEcp(ctypes.Structure):
    _fields_ = [
        ("list_l", ctypes.c_int32),
        ("n_local", ctypes.c_int32),
        ("n_nonlocal", ctypes.c_int32),
        ("rn_local", ctypes.POINTER(ctypes.c_double)),
        ("local_coes", ctypes.POINTER(ctypes.c_double)),
        ("local_exps", ctypes.POINTER(ctypes.c_double)),
        ("rn_non_local", ctypes.POINTER(ctypes.c_double)),
        ("non_local_coes", ctypes.POINTER(ctypes.c_double)),
        ("non_local_exps", ctypes.POINTER(ctypes.c_double)),
    ]


# the six pseudopotential tables in set_ecp's argument order; Context.ecp reports them with list_l
ECP_TABLE_NAMES = ("rn_local", "local_coes", "local_exps", "rn_non_local", "non_local_coes", "non_local_exps")
EcpView = collections.namedtuple("EcpView", ECP_TABLE_NAMES + ("list_l",))


class AiqmcDensityCfg(ctypes.Structure):
    """aiqmc_density_cfg: a family with a zero count is absent."""
    _fields_ = [
        ("grid_lo", ctypes.c_double * 3),
        ("grid_hi", ctypes.c_double * 3),
        ("grid_n", ctypes.c_int32 * 3),
        ("rad_max", ctypes.c_double),
        ("rad_n", ctypes.c_int32),
        ("pair_max", ctypes.c_double),
        ("pair_n", ctypes.c_int32),
    ]


DENSITY_LDS_WORDS = 4096       # AIQMC_DENSITY_LDS_WORDS: privatisation limit of radial + pair
DENSITY_MAX_BINS = 1 << 20     # AIQMC_DENSITY_MAX_BINS
DENSITY_MAX_WORDS = 1 << 28    # AIQMC_DENSITY_MAX_WORDS
DENSITY_FIELDS = ("total", "skipped", "grid", "grid_out", "radial", "radial_out", "pair", "pair_out")
BLOCKING_MAX_SERIES = 8        # AIQMC_BLOCKING_MAX_SERIES
BLOCKING_MAX_LEVELS = 32       # AIQMC_BLOCKING_MAX_LEVELS
# rows of aiqmc_energy_components, in the order of the AIQMC_COMP_* macros (AIQMC_NCOMPONENTS = 8)
RDM_GROUP = 32                 # AIQMC_RDM_GROUP: walkers per contraction workgroup (aiqmc_rdm_accumulate)
RDM_MAX_AO, RDM_MAX_ORB, RDM_MAX_PRIM, RDM_MAX_Q = 128, 64, 512, 16   # AIQMC_RDM_MAX_*
COMPONENT_NAMES = ("total", "kinetic", "kinetic_grad", "v_ee", "v_en", "v_nn", "v_pp_local", "v_pp_nonlocal")


class AiqmcRdmBasis(ctypes.Structure):
    """aiqmc_rdm_basis: shells, optional MO coefficients and the mixture q."""
    _fields_ = [
        ("nshell", ctypes.c_int32),
        ("shell_l", ctypes.POINTER(ctypes.c_int32)),
        ("shell_nprim", ctypes.POINTER(ctypes.c_int32)),
        ("shell_center", ctypes.POINTER(ctypes.c_double)),
        ("exps", ctypes.POINTER(ctypes.c_double)),
        ("coefs", ctypes.POINTER(ctypes.c_double)),
        ("norb", ctypes.c_int32),
        ("mo_coeff", ctypes.POINTER(ctypes.c_double)),
        ("nq", ctypes.c_int32),
        ("q_center", ctypes.POINTER(ctypes.c_double)),
        ("q_sigma", ctypes.POINTER(ctypes.c_double)),
        ("q_prob", ctypes.POINTER(ctypes.c_double)),
    ]


def density_cfg(grid=None, radial=None, pair=None) -> AiqmcDensityCfg:
    """grid = (lo[3], hi[3], n[3]), radial = (r_max, n), pair = (r_max, n); None: absent."""
    cfg = AiqmcDensityCfg()
    if grid is not None:
        lo, hi, n = grid
        for d in range(3):
            cfg.grid_lo[d], cfg.grid_hi[d], cfg.grid_n[d] = float(lo[d]), float(hi[d]), int(n[d])
    if radial is not None:
        cfg.rad_max, cfg.rad_n = float(radial[0]), int(radial[1])
    if pair is not None:
        cfg.pair_max, cfg.pair_n = float(pair[0]), int(pair[1])
    return cfg


_vp, _i32, _i64, _u64, _dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
_int, _str = ctypes.c_int, ctypes.c_char_p


def _p(t):
    return ctypes.POINTER(t)


# The C-ABI of include/aiqmc.h, declared once: name -> (restype, argtypes); load() applies it.
# argtypes None: the function takes no argument and ctypes' default is left alone.
_SIGNATURES = {
    "aiqmc_create": (_int, [_p(AiqmcCfg), _p(_vp)]),
    "aiqmc_destroy": (_int, [_vp]),
    "aiqmc_param_count": (_i64, [_vp]),
    "aiqmc_workspace_bytes": (_i64, [_vp]),
    "aiqmc_last_error": (_str, None),
    "aiqmc_supported_shapes": (_str, None),
    "aiqmc_set_params": (_int, [_vp, _p(_dbl), _i64, _vp]),
    "aiqmc_set_params_device": (_int, [_vp, _vp, _i64, _vp]),
    "aiqmc_logpsi": (_int, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "aiqmc_logpsi_grad": (_int, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "aiqmc_orbitals": (_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "aiqmc_local_energy": (_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "aiqmc_local_energy_complex": (_int, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "aiqmc_mc_step": (_int, [_vp, _vp, _i32, _i32, _dbl, _i32, _vp, _vp, _vp, _u64, _u64, _vp, _vp]),
    "aiqmc_logpsi_param_grad": (_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "aiqmc_phase_param_grad": (_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "aiqmc_param_grad_weighted": (_int, [_vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    "aiqmc_set_ecp": (_int, [_vp, _p(AiqmcEcp)]),
    "aiqmc_local_energy_ecp": (_int, [_vp, _vp, _i32, _i32, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp]),
    "aiqmc_local_energy_ecp_complex": (_int, [_vp, _vp, _i32, _i32, _vp, _u64, _u64, _vp, _vp, _vp]),
    "aiqmc_dmc_drift_diffusion": (_int, [_vp, _vp, _i32, _dbl, _i32, _vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    "aiqmc_dmc_weights": (_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _dbl, _dbl, _dbl, _dbl, _vp, _vp]),
    "aiqmc_dmc_weights_ex": (_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _dbl, _vp, _vp, _dbl, _dbl, _dbl, _vp, _vp,
                                    _vp]),
    "aiqmc_dmc_cut_minima": (_int, [_vp, _i32, _vp, _vp, _vp, _dbl, _dbl, _vp, _vp]),
    "aiqmc_dmc_branch": (_int, [_vp, _i32, _vp, _dbl, _vp, _vp, _vp]),
    "aiqmc_dmc_tmoves": (_int, [_vp, _vp, _i32, _dbl, _i32, _vp, _vp, _vp, _u64, _u64, _vp, _vp]),
    "aiqmc_spin_squared": (_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "aiqmc_dipole": (_int, [_vp, _vp, _i32, _vp, _vp]),
    "aiqmc_energy_components": (_int, [_vp, _vp, _i32, _i32, _i32, _vp, _u64, _u64, _vp, _vp]),
    "aiqmc_density_layout": (_int, [_vp, _p(AiqmcDensityCfg), _p(_i64), _p(_i64), _p(_i32)]),
    "aiqmc_density_accumulate": (_int, [_vp, _p(AiqmcDensityCfg), _vp, _i32, _vp, _vp, _vp]),
    "aiqmc_set_rdm_basis": (_int, [_vp, _p(AiqmcRdmBasis)]),
    "aiqmc_rdm_accumulate": (_int, [_vp, _vp, _i32, _i32, _i32, _vp, _u64, _u64, _vp, _vp, _i32, _vp, _vp, _vp]),
    "aiqmc_rdm_basis_values": (_int, [_vp, _vp, _i32, _i32, _vp, _vp]),
    "aiqmc_space_warp": (_int, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp]),
    "aiqmc_corr_level": (_int, [_i32, _i32, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "aiqmc_corr_final": (_int, [_vp, _vp, _i32, _vp, _vp]),
    "aiqmc_blocking_layout": (_int, [_i64, _i32, _i32, _p(_i64), _p(_i64), _p(_i64)]),
    "aiqmc_blocking_update": (_int, [_vp, _i32, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "aiqmc_profile_enable": (_int, [_vp, _i32]),
    "aiqmc_profile_read": (_int, [_vp, _i32, _p(_dbl), _p(_i64)]),
    "aiqmc_energy_stats": (_int, [_vp, _i32, _i64, _vp, _i32, _vp]),
    "aiqmc_energy_stats_final": (_int, [_vp, _vp]),
    "aiqmc_loss_weights": (_int, [_vp, _vp, _i32, _i64, _dbl, _i32, _dbl, _vp, _vp, _vp, _vp, _vp, _vp]),
    "aiqmc_loss_level": (_int, [_i32, _vp, _vp, _i32, _i64, _vp, _vp, _dbl, _dbl, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "aiqmc_loss_pack": (_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "aiqmc_loss_final": (_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "aiqmc_sr_gram": (_int, [_vp, _vp, _i32, _i64, _i32, _vp, _vp, _vp, _i32, _vp]),
    "aiqmc_debug_logpsi_grad_forward": (_int, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "aiqmc_debug_local_energy_forward": (_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "aiqmc_debug_limdrift_factor": (_int, [_vp, _vp, _i32, _dbl, _i32, _p(_dbl), _vp]),
    "aiqmc_debug_launch_lds": (_int, [_i32, _i32, _i32, _i32, _p(_i32), _p(_i32)]),
    "aiqmc_debug_launch_row": (_int, [_vp, _i32, _i32, _p(_i32)]),
    "aiqmc_debug_phase_cycles": (_int, [_vp, _vp]),
    "aiqmc_debug_set_ablate": (_int, [_vp, _i32]),
    "aiqmc_debug_set_fuse_accept": (_int, [_vp, _i32]),
    "aiqmc_debug_set_walker_pivots": (_int, [_vp, _i32]),
    "aiqmc_debug_set_packed_walkers": (_int, [_vp, _i32]),
    "aiqmc_debug_set_quad_pivoted": (_int, [_vp, _i32]),
    "aiqmc_debug_set_fuse_reduce": (_int, [_vp, _i32]),
    "aiqmc_debug_set_lap_waves": (_int, [_vp, _i32]),
    "aiqmc_debug_set_proposal_reuse": (_int, [_vp, _i32]),
    "aiqmc_debug_set_obs_chunk": (_int, [_vp, _i32]),
    "aiqmc_debug_read_draws": (_int, [_vp, _i32, _vp, _i64, _vp]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


_lib: Optional[ctypes.CDLL] = None


def library_sha16(path: Optional[str] = None) -> Optional[str]:
    """First 16 hex digits of the SHA-256 of the shared library file (default: the one this
    module loads).  PMC summaries under profiles/ carry it, and bench.py reports their counters
    only when it matches the library it is running (stale counters are set to null)."""
    import hashlib
    f = path or LIB_PATH
    if not os.path.exists(f):
        return None
    h = hashlib.sha256()
    with open(f, "rb") as fh:
        for chunk in iter(lambda: fh.read(1 << 20), b""):
            h.update(chunk)
    return h.hexdigest()[:16]


def load() -> ctypes.CDLL:
    """Load the HIP library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make -C <pkg>/csrc` or __graft_entry__.build(); "
            "the AIQMC hot path has no CPU fallback")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        if argtypes is not None:
            fn.argtypes = argtypes
    _lib = lib
    return lib


def last_error() -> str:
    return load().aiqmc_last_error().decode()


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {last_error()}")


def _dt(t) -> int:
    """AIQMC_F32 / AIQMC_F64 of a tensor or of a torch dtype."""
    return AIQMC_F32 if getattr(t, "dtype", t) == torch.float32 else AIQMC_F64


LDS_KINDS = ("proposal", "walker", "adjoint", "lap", "pgrad", "fwdlap")   # AIQMC_LDS_* order


# AIQMC_LAUNCH_* order: what a walker launch is (csrc/launch_route.h)
LAUNCH_KINDS = ("walker_value", "walker_orbitals", "walker_grad", "sweep_walker", "proposal", "quadrature",
                "lap_forward", "grad_forward")


def launch_lds(nelectrons: int, natoms: int, dtype=torch.float32) -> dict:
    """Dynamic LDS bytes and waves per workgroup of the launches of one shape (host only)."""
    lib = load()
    out = {}
    for k, name in enumerate(LDS_KINDS):
        b, w = ctypes.c_int32(0), ctypes.c_int32(0)
        check(lib.aiqmc_debug_launch_lds(int(nelectrons), int(natoms), _dt(dtype), k, ctypes.byref(b),
                                         ctypes.byref(w)), "aiqmc_debug_launch_lds")
        out[name] = {"dyn_lds_bytes_per_wg": b.value, "waves_per_wg": w.value}
    return out


def supported_shapes():
    s = load().aiqmc_supported_shapes().decode()
    return [tuple(int(v) for v in p.split(":")) for p in s.split(",") if p]


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _call(name: str, *args, device=None, stream: bool = True, raw: bool = False):
    """The one call path into the library: symbol `name` with args (a tensor or None goes through
    _ptr, anything else as it is; _SIGNATURES converts Python numbers), then the current stream of
    `device` (default: the first tensor argument's) when `stream` is set, with that device current
    for the call and the caller's restored after it.  check()s the return code; raw: returns the
    library's return value unchecked instead."""
    if device is None:
        device = next(a.device for a in args if isinstance(a, torch.Tensor))
    args = [_ptr(a) if a is None or isinstance(a, torch.Tensor) else a for a in args]
    if stream:
        args.append(_stream(device))
    with torch.cuda.device(device):
        rc = getattr(load(), name)(*args)
    if not raw:
        check(rc, name)
    return rc


def energy_stats(e_l: torch.Tensor, finalize: bool = True) -> torch.Tensor:
    """aiqmc_energy_stats on a device tensor of local energies (float32/float64): a float64 device
    tensor [sum |e - m|^2, n m, n m^2, n, mean, variance] (the last two only with finalize)."""
    if not e_l.is_cuda or e_l.dtype not in (torch.float32, torch.float64):
        raise ValueError("energy_stats: a float32/float64 device tensor is required")
    e = e_l.contiguous().reshape(-1)
    out = torch.empty(6, dtype=torch.float64, device=e.device)
    _call("aiqmc_energy_stats", e, _dt(e), e.numel(), out, 1 if finalize else 0)
    return out


def loss_weights(e_l: torch.Tensor, clip_scale: float, center_at_clipped: bool, wscale: float,
                 want_imag: bool):
    """aiqmc_loss_weights (one rank): for device local energies (real, or complex: re/im), the
    energy-gradient weights w_re = wscale Re(diff), w_im = wscale Im(diff + aux) (None unless
    want_imag), aux.clipped_energy (same dtype as e_l) and float64 device stats
    [Re mean, Im mean, variance, Re centre, Im centre]."""
    cplx = torch.is_complex(e_l)
    er = (e_l.real if cplx else e_l).contiguous().reshape(-1)
    if not er.is_cuda or er.dtype not in (torch.float32, torch.float64):
        raise ValueError("loss_weights: float32/float64 (or complex64/128) device energies are required")
    ei = e_l.imag.contiguous().reshape(-1) if cplx else None
    n = er.numel()
    wr = torch.empty_like(er)
    wi = torch.empty_like(er) if want_imag else None
    cr = torch.empty_like(er)
    ci = torch.empty_like(er) if cplx else None
    st = torch.empty(5, dtype=torch.float64, device=er.device)
    _call("aiqmc_loss_weights", er, ei, _dt(er), n, float(clip_scale), 1 if center_at_clipped else 0, float(wscale),
          wr, wi, cr, ci, st)
    clipped = torch.complex(cr, ci) if cplx else cr
    return wr, wi, clipped.reshape(e_l.shape), st


def loss_level(level: int, er: torch.Tensor, ei: Optional[torch.Tensor], L1=None, L2=None,
               clip_scale: float = 0.0, wscale: float = 1.0, g0: bool = False, want_phase: bool = False):
    """aiqmc_loss_level on this rank's device energies (er, ei: contiguous 1-D, float32/float64).
    level 1 -> L1 [6] float64; level 2 -> L2 [2]; level 3 -> (w [1 or 2, n], wp [n] or None,
    clipped_re, clipped_im or None, head [2] float64 = sums of the clipped energies)."""
    n = er.numel()
    dev = er.device
    if level in (1, 2):
        out = torch.empty(6 if level == 1 else 2, dtype=torch.float64, device=dev)
        _call("aiqmc_loss_level", level, er, ei, _dt(er), n, L1, None, 0.0, 0.0, 0, None, None, None, None, out)
        return out
    w = torch.empty(2 if g0 else 1, n, dtype=er.dtype, device=dev)
    wp = torch.empty_like(er) if want_phase else None
    cr = torch.empty_like(er)
    ci = torch.empty_like(er) if ei is not None else None
    head = torch.empty(2, dtype=torch.float64, device=dev)
    _call("aiqmc_loss_level", 3, er, ei, _dt(er), n, L1, L2, float(clip_scale), float(wscale), 1 if g0 else 0,
          w, wp, cr, ci, head)
    return w, wp, cr, ci, head


def loss_pack(g: torch.Tensor, gp: Optional[torch.Tensor], g0: Optional[torch.Tensor], head: torch.Tensor):
    """L3 = [head (2), g + gp (P), g0 (P, if given)] as one float64 device vector."""
    P = g.numel()
    L3 = torch.empty(2 + P * (2 if g0 is not None else 1), dtype=torch.float64, device=g.device)
    L3[:2].copy_(head)
    _call("aiqmc_loss_pack", g, gp, g0, _dt(g), P, L3)
    return L3


def loss_final(L1: torch.Tensor, L3: torch.Tensor, P: int, g0: bool, center_at_clipped: bool, world: int,
               dtype: torch.dtype):
    """(grad [P] of dtype, stats [6] float64) from the summed level vectors."""
    grad = torch.empty(P, dtype=dtype, device=L1.device)
    stats = torch.empty(6, dtype=torch.float64, device=L1.device)
    _call("aiqmc_loss_final", L1, L3, P, 1 if g0 else 0, 1 if center_at_clipped else 0, int(world), _dt(dtype), grad,
          stats)
    return grad, stats


def sr_gram(o_re: torch.Tensor, o_im: Optional[torch.Tensor] = None, center_re: Optional[torch.Tensor] = None,
            center_im: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
            accumulate: bool = False) -> torch.Tensor:
    """aiqmc_sr_gram on per-walker Jacobians [B, P] (float32/float64 device tensors; o_im: the
    phase Jacobian or None): the float64 device vector [G (P*P), s_re (P), s_im (P), n] of the
    Gram product centred at center_re / center_im ([P], converted to the Jacobian's dtype; None =
    0).  `out`: written in place, added to with accumulate=True (walker blocks)."""
    if not (o_re.is_cuda and o_re.dim() == 2 and o_re.dtype in (torch.float32, torch.float64)):
        raise ValueError("sr_gram: a [B, P] float32/float64 device tensor is required")
    B, P = o_re.shape
    if P <= 0:
        raise ValueError("sr_gram: P must be positive")
    dev, dt = o_re.device, o_re.dtype

    def same(t, shape, what):
        if t is None:
            return None
        t = t.to(dev, dt).contiguous()
        if tuple(t.shape) != shape:
            raise ValueError(f"sr_gram: {what} must have shape {shape}, got {tuple(t.shape)}")
        return t

    a = o_re.contiguous()
    b = same(o_im, (B, P), "o_im")
    cr, ci = same(center_re, (P,), "center_re"), same(center_im, (P,), "center_im")
    n_out = P * P + 2 * P + 1
    if out is None:
        if accumulate:
            raise ValueError("sr_gram: accumulate needs the vector to add to")
        out = torch.empty(n_out, dtype=torch.float64, device=dev)
    elif not (out.is_cuda and out.device == dev and out.dtype == torch.float64 and out.is_contiguous()
              and out.numel() == n_out):
        raise ValueError(f"sr_gram: out must be a contiguous float64 device vector of {n_out} entries")
    _call("aiqmc_sr_gram", a, b, _dt(a), B, P, cr, ci, out, 1 if accumulate else 0)
    return out


def _corr_args(logabs0, e0, logabs1, logjac, e1):
    """The level inputs as contiguous tensors of one dtype and device: logabs0 / e0 [n],
    logabs1 / logjac / e1 [M, n] (e0 / e1 may be None at level 1)."""
    la1 = logabs1 if logabs1.dim() == 2 else logabs1.reshape(1, -1)
    M, n = la1.shape
    dt = la1.dtype if la1.dtype in (torch.float32, torch.float64) else torch.float64
    fix = lambda t, shape: None if t is None else t.to(la1.device, dt).reshape(shape).contiguous()
    return (fix(logabs0, (n,)), fix(e0, (n,)), fix(la1, (M, n)), fix(logjac, (M, n)), fix(e1, (M, n))), M, n


def corr_level(level: int, logabs0: torch.Tensor, e0: Optional[torch.Tensor], logabs1: torch.Tensor,
               logjac: torch.Tensor, e1: Optional[torch.Tensor], L1: Optional[torch.Tensor] = None,
               L2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """aiqmc_corr_level on this rank's walkers: logabs0 / e0 [n], logabs1 / logjac / e1 [M, n]
    (float32 or float64), lw = 2 (logabs1 - logabs0) + logjac.  Returns float64
    level 1 -> [M] max_b lw (combine ranks with MAX); level 2 -> [M, 5] = [n, sum e0, sum w,
    sum w e1, sum w^2], w = exp(lw - L1) (SUM); level 3 -> [M, 2] = [sum d, sum d^2],
    d = (w n / sum w)(e1 - E_m) - (e0 - E_0) from L1 and the summed L2 (SUM).
    Device tensors run the kernels; host tensors take the same formulas in torch float64."""
    if level not in (1, 2, 3):
        raise ValueError("corr_level: level must be 1, 2 or 3")
    if level >= 2 and (e0 is None or e1 is None or L1 is None):
        raise ValueError("corr_level: levels 2 and 3 need e0, e1 and the combined L1")
    if level == 3 and L2 is None:
        raise ValueError("corr_level: level 3 needs the summed L2")
    (a0, x0, a1, lj, x1), M, n = _corr_args(logabs0, e0, logabs1, logjac, e1)
    if n == 0:
        raise ValueError("corr_level: empty batch")
    if a1.is_cuda:
        dev = a1.device
        out = torch.empty((M,) if level == 1 else (M, 5 if level == 2 else 2), dtype=torch.float64, device=dev)
        l1 = None if L1 is None else L1.to(dev, torch.float64).contiguous()
        l2 = None if L2 is None else L2.to(dev, torch.float64).contiguous()
        _call("aiqmc_corr_level", level, _dt(a1), n, M, a0, x0, a1, lj, x1, l1, l2, out)
        return out
    lw = 2.0 * (a1.double() - a0.double()[None]) + lj.double()
    if level == 1:
        return lw.max(dim=1).values
    w = torch.exp(lw - L1.double().reshape(M, 1))
    x0, x1 = x0.double(), x1.double()
    if level == 2:
        cnt = torch.full((M,), float(n), dtype=torch.float64)
        return torch.stack([cnt, x0.sum().expand(M), w.sum(1), (w * x1).sum(1), (w * w).sum(1)], dim=1)
    l2 = L2.double().reshape(M, 5)
    E0, Em, scale = l2[:, 1] / l2[:, 0], l2[:, 3] / l2[:, 2], l2[:, 0] / l2[:, 2]
    d = (w * scale[:, None]) * (x1 - Em[:, None]) - (x0[None] - E0[:, None])
    return torch.stack([d.sum(1), (d * d).sum(1)], dim=1)


def corr_final(L2: torch.Tensor, L3: torch.Tensor) -> torch.Tensor:
    """aiqmc_corr_final: [M, 5] = [E_0, E_m, E_m - E_0, err_m, ESS_m] (float64) from the summed
    level vectors L2 [M, 5] and L3 [M, 2]; host tensors take the same formulas in torch."""
    M = L2.shape[0]
    if L2.is_cuda:
        l2, l3 = L2.to(torch.float64).contiguous(), L3.to(L2.device, torch.float64).contiguous()
        res = torch.empty(M, 5, dtype=torch.float64, device=L2.device)
        _call("aiqmc_corr_final", l2, l3, M, res)
        return res
    l2, l3 = L2.double().reshape(M, 5), L3.double().reshape(M, 2)
    n, sd, sd2 = l2[:, 0], l3[:, 0], l3[:, 1]
    E0, Em = l2[:, 1] / n, l2[:, 3] / l2[:, 2]
    err = torch.sqrt((sd2 - sd * sd / n) / (n * (n - 1.0)))
    return torch.stack([E0, Em, Em - E0, err, l2[:, 2] * l2[:, 2] / l2[:, 4]], dim=1)


@functools.lru_cache(maxsize=64)
def _blocking_words(B: int, K: int, L: int) -> tuple:
    a, p, s = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    check(load().aiqmc_blocking_layout(B, K, L, ctypes.byref(a), ctypes.byref(p), ctypes.byref(s)),
          "aiqmc_blocking_layout")
    return a.value, p.value, s.value


def blocking_layout(B: int, K: int, L: int) -> dict:
    """aiqmc_blocking_layout (host only): the doubles of {"acc", "pend", "scratch"} for B chains,
    K series and L levels."""
    return dict(zip(("acc", "pend", "scratch"), _blocking_words(int(B), int(K), int(L))))


def blocking_update(x: torch.Tensor, L: int, acc: torch.Tensor, pend: torch.Tensor, scratch: torch.Tensor) -> None:
    """aiqmc_blocking_update: one sample x [K, B] (contiguous float32/float64 on the device) into
    the float64 device buffers acc / pend / scratch of blocking_layout(B, K, L), in place on the
    current stream (two launches, no host synchronisation)."""
    if not (x.is_cuda and x.dim() == 2 and x.is_contiguous() and x.dtype in (torch.float32, torch.float64)):
        raise ValueError("blocking_update: a contiguous [K, B] float32/float64 device tensor is required")
    K, B = x.shape
    for t, n, what in zip((acc, pend, scratch), _blocking_words(B, K, int(L)), ("acc", "pend", "scratch")):
        if not (t.dtype == torch.float64 and t.device == x.device and t.is_contiguous() and t.numel() == n):
            raise ValueError(f"blocking_update: {what} must be a contiguous float64 tensor of {n} words on {x.device}")
    _call("aiqmc_blocking_update", x, _dt(x), B, K, int(L), acc, pend, scratch)


def energy_stats_final(out: torch.Tensor) -> torch.Tensor:
    """aiqmc_energy_stats_final: out[4..5] = [mean, variance] from a summed out[0..3], in place."""
    _call("aiqmc_energy_stats_final", out)
    return out


class Context:
    """One aiqmc_ctx: a system/network configuration bound to one GPU and dtype.

    Every method reaches the library through _call, which makes the context's device current for
    the call and restores the caller's afterwards: after any Context call the current torch device
    is what it was before it.  A method stages its inputs with the vocabulary below (_pos, _inplace,
    _dev, _grad_arg, _rng, _weights, _acc, _obs_chunk), allocates its outputs with _new and makes
    one _call; it adds nothing else."""

    def __init__(self, nelectrons: int, natoms: int, nspins: Sequence[int], atoms, charges,
                 spin_up_indices, spin_down_indices, parallel_indices, antiparallel_indices,
                 dtype: torch.dtype = torch.float32, device: int = 0):
        lib = load()
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("dtype must be torch.float32 or torch.float64")
        self.dtype = dtype
        self.device = torch.device("cuda", device)
        self.N = int(nelectrons)
        self.A = int(natoms)
        self.nspins = (int(nspins[0]), int(nspins[1]))
        self._keep = []
        self._ecp_keep, self._ecp_token = None, None   # set_ecp: the uploaded tables and their identity

        def dbl(a):
            a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
            self._keep.append(a)
            return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

        def i32(a):
            a = np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))
            self._keep.append(a)
            return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

        par = np.asarray(parallel_indices, dtype=np.int32).reshape(2, -1)
        anti = np.asarray(antiparallel_indices, dtype=np.int32).reshape(2, -1)
        cfg = AiqmcCfg()
        cfg.nelectrons = self.N
        cfg.natoms = self.A
        cfg.nspins[0], cfg.nspins[1] = int(nspins[0]), int(nspins[1])
        cfg.dtype = _dt(dtype)
        cfg.device = int(device)
        cfg.atoms = dbl(atoms)
        cfg.charges = dbl(charges)
        cfg.spin_up_indices = i32(spin_up_indices)
        cfg.spin_down_indices = i32(spin_down_indices)
        cfg.parallel_indices = i32(par)
        cfg.n_parallel = par.shape[1]
        cfg.antiparallel_indices = i32(anti)
        cfg.n_antiparallel = anti.shape[1]
        for l in range(3):
            cfg.hidden_dims[l][0] = 4
            cfg.hidden_dims[l][1] = 4
            cfg.hidden_dims_ynlm[l] = 6
        h = ctypes.c_void_p()
        _call("aiqmc_create", ctypes.byref(cfg), ctypes.byref(h), device=self.device, stream=False)
        self._h = h
        self._lib = lib
        self.nparams = int(self._call("aiqmc_param_count", stream=False, raw=True))

    @classmethod
    def for_system(cls, system, dtype: torch.dtype = torch.float32, device: int = 0, atoms=None) -> "Context":
        """The context of a system description: anything with nelectrons, natoms, nspins, atoms,
        charges and tables() (aiqmc.systems.System, oracle.system's).  atoms: another geometry."""
        t = system.tables()
        return cls(system.nelectrons, system.natoms, system.nspins, system.atoms if atoms is None else atoms,
                   system.charges, t["spin_up_indices"], t["spin_down_indices"], t["parallel_indices"],
                   t["antiparallel_indices"], dtype=dtype, device=device)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._lib.aiqmc_destroy(h)
            except Exception:
                pass
            self._h = None

    # -- the call path -----------------------------------------------------
    def _call(self, name: str, *args, stream: bool = True, raw: bool = False):
        """The module's _call on this context: the handle first, on the context's device."""
        return _call(name, self._h, *args, device=self.device, stream=stream, raw=raw)

    # -- the argument vocabulary -------------------------------------------
    def _new(self, *shape, dtype=None) -> torch.Tensor:
        """An output: an uninitialised tensor on the context's device, in its dtype by default."""
        return torch.empty(*shape, dtype=dtype or self.dtype, device=self.device)

    def _pos(self, pos: torch.Tensor) -> torch.Tensor:
        if not isinstance(pos, torch.Tensor):
            pos = torch.as_tensor(np.asarray(pos))
        pos = pos.to(device=self.device, dtype=self.dtype).contiguous()
        if pos.shape[-1] != 3 * self.N:
            raise ValueError(f"positions must have trailing dim 3N={3 * self.N}, got {tuple(pos.shape)}")
        return pos.reshape(-1, 3 * self.N)

    def _inplace(self, pos: torch.Tensor, who: str, note: str = " (updated in place)") -> int:
        """The walker count B of positions a sweep updates in place."""
        if not (pos.is_cuda and pos.dtype == self.dtype and pos.is_contiguous()):
            raise ValueError(f"{who} needs a contiguous device tensor of the context dtype{note}")
        return pos.numel() // (3 * self.N)

    def _dev(self, t, n: Optional[int], what: Optional[str] = None, real: bool = False) -> torch.Tensor:
        """An input, converted: t as a contiguous tensor of the context's dtype on its device, of n
        values when n is given (what: its name in the error); real: a complex t gives its real part."""
        t = torch.as_tensor(t)
        if real and torch.is_complex(t):
            t = t.real
        t = t.to(self.device, self.dtype).contiguous()
        if n is not None and t.numel() != n:
            raise ValueError(f"{what}: expected {n} values, got {t.numel()}" if what else
                             f"expected {n} values, got {t.numel()}")
        return t

    def _grad_arg(self, g: torch.Tensor, B: int, what: str) -> torch.Tensor:
        """An input that is refused instead of converted (apart from _dev for that reason alone): a
        gradient [B, 3N] that an earlier call returned is already a device tensor of the context
        dtype, and anything else is a mistake that a conversion would hide."""
        if not (isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == self.dtype):
            raise ValueError(f"{what} must be a device tensor of the context dtype {self.dtype}")
        if g.numel() != B * 3 * self.N:
            raise ValueError(f"{what}: expected {B * 3 * self.N} values, got {g.numel()}")
        return g.contiguous()

    def _rng(self, what: str, **draws):
        """The draws of a sampling call, name=(tensor or None, values expected): (rng mode, staged
        draws in the given order).  All None: Philox, (None, ...); all given: host mode, each
        through _dev; anything between is refused."""
        given = [k for k, (t, _) in draws.items() if t is not None]
        if given and len(given) != len(draws):
            names = list(draws)
            raise ValueError(f"{', '.join(names[:-1])} and {names[-1]} are injected together or not at all")
        mode = AIQMC_RNG_HOST if given else AIQMC_RNG_PHILOX
        return mode, tuple(self._dev(t, n, f"{what}: {k}") if given else None for k, (t, n) in draws.items())

    def _weights(self, weights, B: int) -> Optional[torch.Tensor]:
        """Per-walker weights [B] in the context's dtype on its device, or None."""
        if weights is None:
            return None
        w = torch.as_tensor(weights).to(self.device, self.dtype).contiguous().reshape(-1)
        if w.numel() != B:
            raise ValueError("weights must have one entry per walker")
        return w

    def _acc(self, acc, n: int, dtype: torch.dtype, who: str) -> torch.Tensor:
        """A caller-owned accumulator, written in place: never converted, so it is refused unless it
        is contiguous, of dtype, on the context's device and n words long."""
        if not (isinstance(acc, torch.Tensor) and acc.dtype == dtype and acc.device == self.device
                and acc.is_contiguous() and acc.numel() == n):
            raise ValueError(f"{who}: acc must be a contiguous {str(dtype).replace('torch.', '')} tensor of {n} "
                             f"words on {self.device}")
        return acc

    @contextlib.contextmanager
    def _obs_chunk(self, chunk: Optional[int]):
        """The configurations per value launch of the observables (spin_squared, rdm_accumulate) set
        to chunk inside the block and back to the default after it; None: left alone."""
        if chunk is None:
            yield
            return
        if int(chunk) <= 0:
            raise ValueError("chunk must be positive")
        self._call("aiqmc_debug_set_obs_chunk", int(chunk), stream=False)
        try:
            yield
        finally:
            self._call("aiqmc_debug_set_obs_chunk", 0, stream=False)

    # -- kernel timing (HIP events on the launch stream) -------------------
    def profile(self, on: bool = True):
        self._call("aiqmc_profile_enable", 1 if on else 0, stream=False)

    def profile_read(self, slot: int):
        """(summed kernel ms, launches) recorded in `slot` since the last read."""
        ms = ctypes.c_double()
        n = ctypes.c_int64()
        self._call("aiqmc_profile_read", int(slot), ctypes.byref(ms), ctypes.byref(n), stream=False)
        return ms.value, n.value

    def workspace_bytes(self) -> int:
        return int(self._call("aiqmc_workspace_bytes", stream=False, raw=True))

    def set_params(self, flat: np.ndarray):
        flat = np.ascontiguousarray(np.asarray(flat, dtype=np.float64).reshape(-1))
        if flat.size != self.nparams:
            raise ValueError(f"expected {self.nparams} parameters, got {flat.size}")
        self._call("aiqmc_set_params", flat.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), flat.size)

    def set_params_device(self, flat: torch.Tensor):
        """Canonical parameters already on this context's device (float64, tree_flatten order):
        repacked into the kernel layout on the device, stream-ordered (no host copy, no sync)."""
        if not (isinstance(flat, torch.Tensor) and flat.is_cuda and flat.dtype == torch.float64
                and flat.is_contiguous() and flat.device == self.device):
            raise ValueError("set_params_device needs a contiguous float64 tensor on the context's device")
        if flat.numel() != self.nparams:
            raise ValueError(f"expected {self.nparams} parameters, got {flat.numel()}")
        self._call("aiqmc_set_params_device", flat, flat.numel())
        self._flat_keep = flat   # the repack reads it later on the stream: keep it alive until then

    def logpsi(self, pos: torch.Tensor, with_phase: bool = True):
        p = self._pos(pos)
        B = p.shape[0]
        logabs = self._new(B)
        phase = self._new(B) if with_phase else None
        self._call("aiqmc_logpsi", p, B, logabs, phase)
        return logabs, phase

    def orbitals(self, pos: torch.Tensor):
        """The complex orbital matrix [B, N, N] (make_orbitals.apply, nn.py:409-506)."""
        p = self._pos(pos)
        B = p.shape[0]
        out = self._new(B, self.N, self.N, 2)
        self._call("aiqmc_orbitals", p, B, out, None, None)
        return torch.view_as_complex(out)

    # -- observables (aiqmc/observables.py) ---------------------------------
    def spin_squared(self, pos: torch.Tensor, want_pairs: bool = False, chunk: Optional[int] = None):
        """The S^2 estimator of each walker for this context's fixed spin assignment
        (aiqmc_spin_squared): a complex tensor [B] (complex64 for a float32 context; the imaginary
        part averages to zero).  want_pairs: also (dlogabs, dphase) [B, n_up, n_down], log|psi| and
        phase at the walker with up slot i and down slot j exchanged minus those at the walker.
        chunk: configurations per value launch for this call (diagnostics; default 4096, whole
        walkers, at least one); the result does not depend on it."""
        p = self._pos(pos)
        B = p.shape[0]
        re, im = self._new(B), self._new(B)
        dl = self._new(B, *self.nspins) if want_pairs else None
        dp = self._new(B, *self.nspins) if want_pairs else None
        with self._obs_chunk(chunk):
            self._call("aiqmc_spin_squared", p, B, re, im, dl, dp)
        s2 = torch.complex(re, im)
        return (s2, dl, dp) if want_pairs else s2

    def dipole(self, pos: torch.Tensor) -> torch.Tensor:
        """Dipole moment [B, 3] in atomic units: sum_a Z_a R_a - sum_i r_i (aiqmc_dipole; Z_a the
        context charges, Z_eff under an ECP)."""
        p = self._pos(pos)
        B = p.shape[0]
        mu = self._new(B, 3)
        self._call("aiqmc_dipole", p, B, mu)
        return mu

    def energy_components(self, pos: torch.Tensor, complex_output: bool = False, rot: Optional[torch.Tensor] = None,
                          seed: int = 0, offset: int = 0) -> torch.Tensor:
        """What the local energy of each walker is made of (aiqmc_energy_components): a real tensor
        [8, B], rows in the order of COMPONENT_NAMES; row 0 is the bits of local_energy /
        local_energy_complex(...).real, under an ECP of local_energy_ecp(...).real with the same
        rot / seed / offset (ignored without an ECP).  One sample for a make_blocking(nseries=8)
        accumulator (aiqmc/Energy/components.py)."""
        p = self._pos(pos)
        B = p.shape[0]
        out = self._new(len(COMPONENT_NAMES), B)
        mode, (r,) = self._rng("energy_components", rot=(rot, 9 * B))
        self._call("aiqmc_energy_components", p, B, 1 if complex_output else 0, mode, r, seed, offset, out)
        return out

    def density_layout(self, cfg: AiqmcDensityCfg) -> dict:
        """aiqmc_density_layout (host only): {"offsets": {name: first word}, "sizes": {name: words},
        "n_words", "privatised"} of the int64 accumulator for cfg (density_cfg) on this context;
        names in DENSITY_FIELDS order.  privatised: radial + pair take the LDS path."""
        off = (ctypes.c_int64 * 8)()
        nw, priv = ctypes.c_int64(0), ctypes.c_int32(0)
        self._call("aiqmc_density_layout", ctypes.byref(cfg), off, ctypes.byref(nw), ctypes.byref(priv), stream=False)
        ends = list(off[1:]) + [nw.value]
        return {"offsets": dict(zip(DENSITY_FIELDS, off)),
                "sizes": {k: e - o for k, o, e in zip(DENSITY_FIELDS, off, ends)},
                "n_words": nw.value, "privatised": bool(priv.value)}

    def density_accumulate(self, pos: torch.Tensor, acc: torch.Tensor, cfg: AiqmcDensityCfg,
                           weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        """aiqmc_density_accumulate: bins the walkers pos [B, 3N] (weights [B] or None) into acc, a
        contiguous int64 tensor of density_layout(cfg)["n_words"] words on this context's device
        (zeroed by the caller before the first call), in place on the current stream."""
        p = self._pos(pos)
        B = p.shape[0]
        acc = self._acc(acc, self.density_layout(cfg)["n_words"], torch.int64, "density_accumulate")
        self._call("aiqmc_density_accumulate", ctypes.byref(cfg), p, B, self._weights(weights, B), acc)
        return acc

    # -- one-body density matrix (aiqmc/observables.py make_density_matrix) ------
    def set_rdm_basis(self, shell_l, shell_nprim, shell_center, exps, coefs, mo_coeff, q_center, q_sigma, q_prob,
                      token=None) -> None:
        """aiqmc_set_rdm_basis: shells (l [nshell], primitives per shell [nshell], centres
        [nshell, 3], concatenated exponents and coefficients), mo_coeff [2, nao, norb] or None (the
        functions themselves) and the mixture q (centres [nq, 3], sigmas, probabilities).  token:
        anything comparable that identifies these tables; a call with the token of the tables
        already uploaded does nothing."""
        if token is not None and token == getattr(self, "_rdm_token", None):
            return
        i32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))
        dbl = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
        pi = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        pd = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        l, npr, cen, ex, co = i32(shell_l), i32(shell_nprim), dbl(shell_center), dbl(exps), dbl(coefs)
        qc, qs, qp = dbl(q_center), dbl(q_sigma), dbl(q_prob)
        nao = int(((l + 1) * (l + 2) // 2).sum())
        if cen.size != 3 * l.size or npr.size != l.size or ex.size != co.size or ex.size != int(npr.sum()):
            raise ValueError("set_rdm_basis: shell tables of inconsistent sizes")
        if qc.size != 3 * qs.size or qp.size != qs.size:
            raise ValueError("set_rdm_basis: q tables of inconsistent sizes")
        b = AiqmcRdmBasis()
        b.nshell, b.shell_l, b.shell_nprim, b.shell_center, b.exps, b.coefs = l.size, pi(l), pi(npr), pd(cen), pd(ex), pd(co)
        mo = None
        if mo_coeff is not None:
            mo = np.asarray(mo_coeff, dtype=np.float64)
            if mo.ndim != 3 or mo.shape[0] != 2 or mo.shape[1] != nao:
                raise ValueError(f"set_rdm_basis: mo_coeff must be [2, nao={nao}, norb]")
            b.norb = mo.shape[2]
            mo = np.ascontiguousarray(mo.reshape(-1))
            b.mo_coeff = pd(mo)
        else:
            b.norb = nao
        b.nq, b.q_center, b.q_sigma, b.q_prob = qs.size, pd(qc), pd(qs), pd(qp)
        self._rdm_token = None
        self._call("aiqmc_set_rdm_basis", ctypes.byref(b), stream=False)
        self._rdm_token, self.rdm_norb = token, int(b.norb)

    def clear_rdm_basis(self) -> None:
        self._rdm_token = None
        self._call("aiqmc_set_rdm_basis", None, stream=False)

    def rdm_basis_values(self, points: torch.Tensor, spin: int = 0) -> torch.Tensor:
        """aiqmc_rdm_basis_values: the basis functions (MO-contracted with spin's coefficients when
        set) at points [M, 3] -> [M, norb] of the context dtype."""
        p = self._dev(points, None).reshape(-1, 3)
        M = p.shape[0]
        out = self._new(M, int(getattr(self, "rdm_norb", 0)))
        self._call("aiqmc_rdm_basis_values", p, M, int(spin), out)
        return out

    def rdm_accumulate(self, pos: torch.Tensor, samples: int, rprime: Optional[torch.Tensor] = None, seed: int = 0,
                       step: int = 0, weights: Optional[torch.Tensor] = None, acc: Optional[torch.Tensor] = None,
                       accumulate: bool = False, want_points: bool = False, want_ratios: bool = False,
                       chunk: Optional[int] = None):
        """aiqmc_rdm_accumulate: acc (float64 [1 + 2 K K 2] on this device; None: a new one) receives
        W = sum of the weights and the sums [2, K, K, (re, im)] over walkers, points and electrons of
        the channel; accumulate adds into acc.  rprime [B, S, 3]: the injected points (None: drawn
        from q by Philox (seed, step)).  Returns acc, then rprime_out [B, S, 3] (want_points) and
        ratio_out [B, S, N, 2] (want_ratios).  chunk: as in spin_squared.  No host synchronisation."""
        p = self._pos(pos)
        B, S = p.shape[0], int(samples)
        K = int(getattr(self, "rdm_norb", 0))
        n = 1 + 4 * K * K
        if acc is None:
            acc = torch.zeros(n, dtype=torch.float64, device=self.device)
        else:
            self._acc(acc, n, torch.float64, "rdm_accumulate")
        mode, (r,) = self._rng("rdm_accumulate", rprime=(rprime, B * max(S, 0) * 3))
        w = self._weights(weights, B)
        rp = self._new(B, max(S, 0), 3) if want_points else None
        ro = self._new(B, max(S, 0), self.N, 2) if want_ratios else None
        with self._obs_chunk(chunk):
            self._call("aiqmc_rdm_accumulate", p, B, S, mode, r, seed, step, w, acc, 1 if accumulate else 0, rp, ro)
        out = (acc,) + ((rp,) if want_points else ()) + ((ro,) if want_ratios else ())
        return out if len(out) > 1 else acc

    # -- correlated sampling (aiqmc/correlatedsamples) ------------------------
    def space_warp(self, pos: torch.Tensor, new_atoms):
        """The space-warp transform of the walkers from this context's atoms to the geometries
        new_atoms [M, A, 3] (aiqmc_space_warp): (newpos [M, B, 3N], logjac [M, B]) of the context
        dtype, logjac = sum_i log|det J_i|."""
        p = self._pos(pos)
        B = p.shape[0]
        na = torch.as_tensor(np.asarray(new_atoms.detach().cpu()) if isinstance(new_atoms, torch.Tensor) else
                             np.asarray(new_atoms), dtype=torch.float64)
        if na.dim() == 2:
            na = na[None]
        if na.dim() != 3 or tuple(na.shape[1:]) != (self.A, 3):
            raise ValueError(f"new_atoms must be [M, {self.A}, 3], got {tuple(na.shape)}")
        M = na.shape[0]
        na = na.to(self.device).contiguous()   # float64 whatever the context's dtype: not _dev
        newpos, logjac = self._new(M, B, 3 * self.N), self._new(M, B)
        if M and B:
            self._call("aiqmc_space_warp", p, B, na, M, newpos, logjac)
        return newpos, logjac

    def _logpsi_grad(self, name: str, pos: torch.Tensor):
        p = self._pos(pos)
        B = p.shape[0]
        logabs, grad = self._new(B), torch.empty_like(p)
        self._call(name, p, B, logabs, grad)
        return logabs, grad

    def logpsi_grad(self, pos: torch.Tensor):
        return self._logpsi_grad("aiqmc_logpsi_grad", pos)

    def logpsi_grad_forward_mode(self, pos: torch.Tensor):
        """Diagnostics: the same quantity through the forward-mode kernel (cross-check)."""
        return self._logpsi_grad("aiqmc_debug_logpsi_grad_forward", pos)

    def set_lap_waves(self, waves: int):
        """Waves per walker of the local energy's first-derivative pass (0 = by batch size)."""
        self._call("aiqmc_debug_set_lap_waves", int(waves), stream=False)

    def set_fuse_accept(self, on: bool):
        """Diagnostics: fused (default) or separate per-sweep acceptance launch in mc_step."""
        self._call("aiqmc_debug_set_fuse_accept", int(bool(on)), stream=False)

    def set_walker_pivots(self, reuse: bool):
        """Diagnostics: walker launches after an mc_step's first sweep re-use the previous sweep's
        Gauss-Jordan pivot order (default) or run partial pivoting every sweep."""
        self._call("aiqmc_debug_set_walker_pivots", int(bool(reuse)), stream=False)

    def set_packed_walkers(self, on: bool):
        """Diagnostics: walker launches of N <= 8 several per wave (default) or one wave each."""
        self._call("aiqmc_debug_set_packed_walkers", int(bool(on)), stream=False)

    def launch_row(self, kind, nconf: int) -> int:
        """Diagnostics: the row (1..8) of the walker-launch table of csrc/shape.hip that a launch of
        `kind` (a LAUNCH_KINDS name or its index) over nconf configurations reaches with this
        context's current switches.  Launches nothing."""
        k = LAUNCH_KINDS.index(kind) if isinstance(kind, str) else int(kind)
        row = ctypes.c_int32(0)
        self._call("aiqmc_debug_launch_row", k, int(nconf), ctypes.byref(row), stream=False)
        return row.value

    def set_quad_pivoted(self, on: bool):
        """Diagnostics: the N <= 8 ECP quadrature launch factors every configuration with partial
        pivoting (on) instead of the walker's recorded order with a per-configuration fallback."""
        self._call("aiqmc_debug_set_quad_pivoted", int(bool(on)), stream=False)

    def set_fuse_reduce(self, mode):
        """Diagnostics: fp32 mc_step limdrift sums fused into the walker / proposal launches as
        exact integer accumulations: 1 (default) and 2 always,
        0 never (reduction launches summing the same integers: the same bits), 3 never with the
        fp64 tree-sum launch (k_taueff).  True/False map to 2/0."""
        m = 2 if mode is True else (0 if mode is False else int(mode))
        self._call("aiqmc_debug_set_fuse_reduce", m, stream=False)

    def limdrift_factor(self, sumsq: torch.Tensor, tstep: float, mode: int) -> float:
        """Diagnostics: the fp32 limdrift factor of the per-configuration |grad|^2 values `sumsq`
        (float32 on this context's device) through mc_step's reductions: 0 = fused integer
        accumulators, 1 = k_taueff_part partials, 2 = the fp64 tree sum (k_taueff)."""
        if sumsq.dtype != torch.float32 or sumsq.device != self.device or sumsq.dim() != 1:
            raise TypeError("sumsq must be a 1-D float32 tensor on the context's device")
        x = sumsq.contiguous()
        out = ctypes.c_double(0.0)
        self._call("aiqmc_debug_limdrift_factor", x, int(x.numel()), float(tstep), int(mode), ctypes.byref(out))
        return out.value

    def set_ablate(self, mask: int):
        """Development builds (-DAQ_ABLATE) only: skip proposal phases to time them."""
        self._call("aiqmc_debug_set_ablate", int(mask), stream=False)

    def set_proposal_reuse(self, on: bool):
        """Diagnostics: proposals from the walker cache (default) or recomputed from scratch."""
        self._call("aiqmc_debug_set_proposal_reuse", 1 if on else 0, stream=False)

    def _read_draws(self, which: int, shape) -> torch.Tensor:
        out = self._new(shape)
        self._call("aiqmc_debug_read_draws", int(which), out, out.numel())
        return out

    def last_draws(self, B: int):
        """Diagnostics: the draws the last Philox sweep of B walkers left in the context
        (mc_step's last sweep, dmc_drift_diffusion): (gauss1 [B, 3N], gauss2 [B, N, 3], u [B, N]),
        copied on the current stream."""
        B, N = int(B), self.N
        return self._read_draws(0, (B, 3 * N)), self._read_draws(1, (B, N, 3)), self._read_draws(2, (B, N))

    def last_rotations(self, B: int) -> torch.Tensor:
        """Diagnostics: the Haar rotations [B, 3, 3] of the last Philox local_energy_ecp or
        dmc_tmoves call on B walkers, copied on the current stream."""
        return self._read_draws(3, (int(B), 3, 3))

    def phase_cycles(self):
        """Diagnostics (AQ_PHASE_PROF builds): per-phase cycle sums [32], then cleared."""
        out = np.zeros(32, dtype=np.uint64)
        self._call("aiqmc_debug_phase_cycles", out.ctypes.data, stream=False)
        return out

    def _local_energy(self, name: str, pos: torch.Tensor, want_logabs: bool, want_grad: bool,
                      out: Optional[torch.Tensor] = None):
        p = self._pos(pos)
        B = p.shape[0]
        el = out if out is not None else self._new(B)
        logabs = self._new(B) if want_logabs else None
        grad = torch.empty_like(p) if want_grad else None
        self._call(name, p, B, el, logabs, grad)
        return el, logabs, grad

    def local_energy(self, pos: torch.Tensor, want_logabs: bool = False, want_grad: bool = False,
                     out: Optional[torch.Tensor] = None):
        return self._local_energy("aiqmc_local_energy", pos, want_logabs, want_grad, out)

    def local_energy_complex(self, pos: torch.Tensor) -> torch.Tensor:
        """complex_output=True local energy (hamiltonian.py:110-130): V - 1/2 [lap log|psi| + i lap theta
        + |grad log|psi||^2 - |grad theta|^2 + 2 i grad log|psi| . grad theta], theta = arg psi; a
        complex tensor [B] (complex64 for a float32 context)."""
        p = self._pos(pos)
        B = p.shape[0]
        re, im = self._new(B), self._new(B)
        self._call("aiqmc_local_energy_complex", p, B, re, im)
        return torch.complex(re, im)

    def local_energy_forward_mode(self, pos: torch.Tensor, want_logabs: bool = False, want_grad: bool = False):
        """Diagnostics: the same quantity through the single-launch forward-Laplacian kernel."""
        return self._local_energy("aiqmc_debug_local_energy_forward", pos, want_logabs, want_grad)

    def _param_grad(self, name: str, pos: torch.Tensor, weights: Optional[torch.Tensor], want_value: bool):
        p = self._pos(pos)
        B = p.shape[0]
        w = self._weights(weights, B)
        out = self._new(self.nparams) if w is not None else self._new(B, self.nparams)
        val = self._new(B) if want_value else None
        self._call(name, p, B, w, out, val)
        return (out, val) if want_value else out

    def logpsi_param_grad(self, pos: torch.Tensor, weights: Optional[torch.Tensor] = None,
                          want_logabs: bool = False):
        """d log|psi| / d theta in canonical (tree_flatten) order: [B, P] per walker, or [P] =
        sum_b weights[b] d log|psi_b| / d theta when weights [B] are given."""
        return self._param_grad("aiqmc_logpsi_param_grad", pos, weights, want_logabs)

    def phase_param_grad(self, pos: torch.Tensor, weights: Optional[torch.Tensor] = None,
                         want_phase: bool = False):
        """d phase / d theta (phase = arg det A), same conventions as logpsi_param_grad."""
        return self._param_grad("aiqmc_phase_param_grad", pos, weights, want_phase)

    def param_grad_weighted(self, pos: torch.Tensor, weights: torch.Tensor, phase: bool = False) -> torch.Tensor:
        """[K, P] = weights [K, B] times d f / d theta (f = log|psi|, or the phase), one gradient pass."""
        p = self._pos(pos)
        B = p.shape[0]
        w = self._dev(weights, None)
        if w.dim() != 2 or w.shape[1] != B:
            raise ValueError("weights must be [K, B]")
        out = self._new(w.shape[0], self.nparams)
        self._call("aiqmc_param_grad_weighted", p, B, 1 if phase else 0, w, w.shape[0], out, None)
        return out

    # -- DMC (DMC/drift_diffusion.py, S_matrix.py, dmc.py, branch.py) -------------
    def dmc_drift_diffusion(self, pos: torch.Tensor, tstep: float, gauss1=None, gauss2=None, u=None, seed: int = 0,
                            offset: int = 0):
        """In-place drift-diffusion step; returns (grad_eff_old, grad_new_eff, tdamp[3] float64)."""
        B = self._inplace(pos, "dmc_drift_diffusion", note="")
        N = self.N
        if B * 3 * N != pos.numel():
            raise ValueError(f"positions must hold whole walkers of 3N={3 * N} coordinates")
        # gauss1 [1, B, 3N], gauss2 [1, B, N, 3] (diagonal blocks), u [1, B, N]
        mode, (g1, g2, uu) = self._rng("dmc_drift_diffusion", gauss1=(gauss1, B * 3 * N), gauss2=(gauss2, B * N * 3),
                                       u=(u, B * N))
        go, gn = self._new(B, 3 * N), self._new(B, 3 * N)
        td = torch.zeros(3, dtype=torch.float64, device=self.device)
        self._call("aiqmc_dmc_drift_diffusion", pos, B, float(tstep), mode, g1, g2, uu, seed, offset, go, gn, td)
        return go, gn, td

    def dmc_weights(self, weights: torch.Tensor, eloc_old, eloc_new, grad_eff_old, grad_new_eff, tdamp, tstep: float,
                    e_trial, e_est, branchcut: float, cut_minima: Optional[torch.Tensor] = None):
        """weights *= exp(tau tdamp (S_new + S_old) / 2), in place (S_matrix.py:4-24, dmc.py:88-92).
        e_trial / e_est: scalars, or per-walker [B] values (the driver's first block);
        cut_minima: optional device float64[2] global e_cut minima (multi-GPU, dmc_cut_minima)."""
        B = weights.numel()
        if not (weights.is_cuda and weights.dtype == self.dtype and weights.is_contiguous()):
            raise ValueError("weights must be a contiguous device tensor of the context dtype (updated in place)")
        eo = self._dev(eloc_old, B, "eloc_old", real=True)
        en = self._dev(eloc_new, B, "eloc_new", real=True)
        go = self._grad_arg(grad_eff_old, B, "grad_eff_old")
        gn = self._grad_arg(grad_new_eff, B, "grad_new_eff")
        if not (isinstance(tdamp, torch.Tensor) and tdamp.is_cuda and tdamp.dtype == torch.float64 and tdamp.numel() == 3):
            raise ValueError("tdamp must be the device float64[3] of dmc_drift_diffusion")
        et_b = ee_b = None
        if torch.is_tensor(e_trial) and e_trial.numel() > 1:
            et_b = self._dev(e_trial, B, "e_trial", real=True)
            e_trial = 0.0
        if torch.is_tensor(e_est) and e_est.numel() > 1:
            ee_b = self._dev(e_est, B, "e_est", real=True)
            e_est = 0.0
        e_trial = complex(e_trial).real if not torch.is_tensor(e_trial) else complex(e_trial.item()).real
        e_est = complex(e_est).real if not torch.is_tensor(e_est) else complex(e_est.item()).real
        cm = None
        if cut_minima is not None:
            if not (cut_minima.is_cuda and cut_minima.dtype == torch.float64 and cut_minima.numel() == 2):
                raise ValueError("cut_minima must be a device float64[2]")
            cm = cut_minima.contiguous()
        self._call("aiqmc_dmc_weights_ex", B, eo, en, go, gn, tdamp, float(tstep), et_b, ee_b, float(e_trial),
                   float(e_est), float(branchcut), cm, weights)
        return weights

    def dmc_cut_minima(self, eloc_old, eloc_new, e_est, branchcut: float) -> torch.Tensor:
        """This batch's e_cut minima [2] (float64, device) for eloc_old / eloc_new (S_matrix.py:21-22);
        a multi-GPU driver all-reduces them with MIN (the reference's jnp.min spans all devices)."""
        eo = self._dev(eloc_old, None, real=True)
        B = eo.numel()
        en = self._dev(eloc_new, B, "eloc_new", real=True)
        ee_b = None
        if torch.is_tensor(e_est) and e_est.numel() > 1:
            ee_b = self._dev(e_est, B, "e_est", real=True)
            e_est = 0.0
        e_est = complex(e_est).real if not torch.is_tensor(e_est) else complex(e_est.item()).real
        out = self._new(2, dtype=torch.float64)
        self._call("aiqmc_dmc_cut_minima", B, eo, en, ee_b, float(e_est), float(branchcut), out)
        return out

    def dmc_branch(self, weights: torch.Tensor, u: float):
        """Stochastic comb (branch.py:10-33): (new uniform weight [1], newinds [B] int32)."""
        w = self._dev(weights, None)
        B = w.numel()
        idx, wo = self._new(B, dtype=torch.int32), self._new(1)
        self._call("aiqmc_dmc_branch", B, w, float(u), idx, wo)
        return wo, idx

    def dmc_tmoves(self, pos: torch.Tensor, tstep: float, rot=None, u_sel=None, u_acc=None, seed: int = 0,
                   offset: int = 0):
        """In-place T-moves (DMC/Tmoves.py:32-225) on `pos`; returns the acceptance [B, N].
        rot [B,3,3], u_sel [B], u_acc [B,N]: injected draws (parity mode); all None: Philox."""
        B = self._inplace(pos, "dmc_tmoves")
        mode, (r, us, ua) = self._rng("dmc_tmoves", rot=(rot, 9 * B), u_sel=(u_sel, B), u_acc=(u_acc, B * self.N))
        acc = self._new(B, self.N)
        self._call("aiqmc_dmc_tmoves", pos, B, float(tstep), mode, r, us, ua, seed, offset, acc)
        return acc

    def _ecp_arrays(self, tables, list_l: int):
        """The six tables as private read-only float64 arrays in the C-ABI's shapes ([A][KL],
        [A][list_l+1][KN]), and their identity: list_l and the arrays' bytes."""
        shapes = [(self.A, -1)] * 3 + [(self.A, int(list_l) + 1, -1)] * 3
        arr = [np.array(a, dtype=np.float64, order="C").reshape(sh) for a, sh in zip(tables, shapes)]
        if len({a.shape for a in arr[:3]}) != 1 or len({a.shape for a in arr[3:]}) != 1:
            raise ValueError("ECP tables of one kind must share their shape")
        for a in arr:
            a.flags.writeable = False
        return arr, (int(list_l),) + tuple(a.tobytes() for a in arr)

    def _upload_ecp(self, arr, token) -> None:
        e = AiqmcEcp()
        e.list_l = token[0]
        e.n_local = arr[0].shape[1]
        e.n_nonlocal = arr[3].shape[2]
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        e.rn_local, e.local_coes, e.local_exps = (dp(a) for a in arr[:3])
        e.rn_non_local, e.non_local_coes, e.non_local_exps = (dp(a) for a in arr[3:])
        rc = self._call("aiqmc_set_ecp", ctypes.byref(e), stream=False, raw=True)   # raw: the code is looked at first
        if rc == AIQMC_EHIP:   # the library dropped its tables; a refused argument leaves the old ones in place
            self._ecp_keep, self._ecp_token = None, None
        check(rc, "aiqmc_set_ecp")
        self._ecp_keep, self._ecp_token = arr, token

    def set_ecp(self, rn_local, local_coes, local_exps, rn_non_local, non_local_coes, non_local_exps,
                list_l: int):
        """Pseudopotential tables in the reference drivers' shapes (single_atom_C.py:13-23):
        rn_local/local_coes/local_exps [A][KL], rn_non_local/... [A][list_l+1][KN].  Uploads them
        and records what this context now holds (ecp, ensure_ecp)."""
        self._upload_ecp(*self._ecp_arrays((rn_local, local_coes, local_exps, rn_non_local, non_local_coes,
                                            non_local_exps), list_l))

    def set_ecp_tables(self, e):
        """set_ecp from an object with the seven fields (aiqmc.systems.EcpTables, oracle.pphamiltonian's, EcpView)."""
        self.set_ecp(*(getattr(e, k) for k in ECP_TABLE_NAMES), e.list_l)

    def ensure_ecp(self, rn_local, local_coes, local_exps, rn_non_local, non_local_coes, non_local_exps,
                   list_l: int) -> bool:
        """set_ecp unless the context already holds exactly these tables; True when it uploaded.
        The drop-in closures call it on every evaluation: only the context knows what it holds,
        so a set_ecp from anywhere else in between is seen."""
        arr, token = self._ecp_arrays((rn_local, local_coes, local_exps, rn_non_local, non_local_coes,
                                       non_local_exps), list_l)
        if token == self._ecp_token:
            return False
        self._upload_ecp(arr, token)
        return True

    @property
    def ecp(self) -> Optional[EcpView]:
        """The tables this context holds, by name (read-only arrays in the C-ABI's shapes), or None."""
        return None if self._ecp_token is None else EcpView(*self._ecp_keep, self._ecp_token[0])

    def local_energy_ecp(self, pos: torch.Tensor, rot: Optional[torch.Tensor] = None, seed: int = 0,
                         offset: int = 0, want_quadrature: bool = False, complex_output: bool = False):
        """Complex pseudopotential local energy [B] (pphamiltonian.py:177-188).  rot [B,3,3]:
        injected rotations (parity mode); None: Philox Haar draws from (seed, offset).
        complex_output: with the kinetic energy's phase terms (pphamiltonian.py:84-104)."""
        p = self._pos(pos)
        B = p.shape[0]
        er, ei = self._new(B), self._new(B)
        mode, (r,) = self._rng("local_energy_ecp", rot=(rot, 9 * B))
        if complex_output:
            if want_quadrature:
                raise ValueError("want_quadrature is not available with complex_output")
            self._call("aiqmc_local_energy_ecp_complex", p, B, mode, r, seed, offset, er, ei)
            return torch.complex(er, ei)
        q = (B, self.N, self.A, ECP_NQ)
        lq, pq = (self._new(q), self._new(q)) if want_quadrature else (None, None)
        self._call("aiqmc_local_energy_ecp", p, B, mode, r, seed, offset, er, ei, lq, pq)
        e = torch.complex(er, ei)
        return (e, lq, pq) if want_quadrature else e

    def mc_step(self, pos: torch.Tensor, nsteps: int, tstep: float, gauss1=None, gauss2=None, u=None,
                seed: int = 0, offset: int = 0, count_accepts: bool = False):
        """In-place Metropolis on `pos` (must be a contiguous device tensor of ctx dtype)."""
        B = self._inplace(pos, "mc_step")
        n = int(nsteps) * B * self.N
        mode, (g1, g2, uu) = self._rng("mc_step", gauss1=(gauss1, 3 * n), gauss2=(gauss2, 3 * n), u=(u, n))
        acc = torch.zeros(B, dtype=torch.int32, device=self.device) if count_accepts else None
        self._call("aiqmc_mc_step", pos, B, int(nsteps), float(tstep), mode, g1, g2, uu, seed, offset, acc)
        return acc


