"""Observables other than the energy (names and signatures of ferminet/observables.py, which the
reference tree vendors: ``make_s2`` :98-227, ``make_dipole`` :230-272).

``make_s2(signed_network, nspins, assign_spin=True, states=0)`` returns
``s2_estimator(params, data, state=None)``: for every walker of ``data.positions [B, 3N]`` the
spin-squared estimator of the fixed spin assignment,

    S2_L(x) = (na - nb)/2 ((na - nb)/2 + 1) + nb - sum_{i in up} sum_{j in down} psi(x_{i<->j}) / psi(x),

na = max(nspins), nb = min(nspins), x_{i<->j} = x with the coordinates of electron slots i and j
exchanged (the spin labels stay on the slots; i over the up slots ascending in the outer loop, j
over the down slots in the inner one).  psi is complex here, so the result is a COMPLEX tensor
[B] (complex64 for float32 positions) -- the package's convention for complex per-walker
quantities (``local_energy(..., complex_output=True)``); its imaginary part averages to zero.
Nothing is clamped: a walker on a node of psi gives an infinite or NaN value.

``make_dipole(signed_network, states=0)`` returns ``dipole_estimator(params, data, state=None)``
-> [B, 3], mu = sum_a Z_a R_a - sum_i r_i in atomic units (Z_a = ``data.charges`` for a generic
callable, the network's charges -- Z_eff under an ECP -- for an aiqmc network).

If ``signed_network`` is the ``apply`` of an aiqmc ``make_ai_net`` Network (the detection
``Energy.hamiltonian.local_energy`` uses), the estimators run in the HIP kernels of
csrc/observables.hip (``Context.spin_squared`` / ``Context.dipole``): n_up n_down + 1 value
forwards per walker.  Any other callable takes a batched torch path that builds the exchanged
positions and calls it once on the walkers and once on all B n_up n_down exchanged
configurations.  Such a callable follows this package's ``apply`` convention
``signed_network(params, positions [M, 3N], spins, atoms, charges) -> (phase [M], log|psi| [M])``
with the phase an angle in radians; a complex first output is taken as the unit-modulus sign
factor psi / |psi| instead.  Its spin slots come from ``data.spins`` (> 0 up, < 0 down, as
``spin_indices.spin_indices_h``), or are the first nspins[0] slots up when ``data.spins`` is None.

``make_density`` (density and pair-distance histograms) and ``make_density_matrix`` (the one-body
density matrix on a Gaussian basis supplied by the caller, ferminet's ``make_density_matrix``
:275-407 without its pyscf basis and Hartree-Fock chain; natural-orbital occupations) are
accumulators over sweeps: see their docstrings.

Batch means over several ranks go through ``constants.pmean`` / ``constants.pmean_stats``
(``batch_mean``, ``s2_stats``); no other collective is involved.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import torch

from . import constants
from .wavefunction_Ynlm.nn import as_positions, kernel_dtype, network_of


def _spin_slots(spins, nspins: Tuple[int, int], nelectrons: int):
    """(up slots, down slots) of the generic path."""
    if spins is None:
        up, dn = np.arange(nspins[0]), np.arange(nspins[0], nspins[0] + nspins[1])
    else:
        s = spins.detach().cpu().numpy() if isinstance(spins, torch.Tensor) else np.asarray(spins)
        s = np.asarray(s, dtype=np.float64)
        s = s.reshape(-1, s.shape[-1])[0]
        up, dn = np.nonzero(s > 0)[0], np.nonzero(s < 0)[0]
    if len(up) != nspins[0] or len(dn) != nspins[1] or len(up) + len(dn) != nelectrons:
        raise ValueError(f"spin slots ({len(up)} up, {len(dn)} down of {nelectrons} electrons) do not match "
                         f"nspins={tuple(nspins)}")
    return up, dn


def exchanged_positions(pos: torch.Tensor, up: Sequence[int], dn: Sequence[int]) -> torch.Tensor:
    """[B, n_up n_down, 3N]: pos [B, 3N] with the coordinates of slots up[ia] and dn[ib] exchanged,
    pair index ia * n_down + ib."""
    B, n3 = pos.shape
    N = n3 // 3
    perm = np.tile(np.arange(N), (len(up) * len(dn), 1))
    for ia, i in enumerate(up):
        for ib, j in enumerate(dn):
            perm[ia * len(dn) + ib, [i, j]] = [j, i]
    x = pos.reshape(B, N, 3)[:, torch.as_tensor(perm, device=pos.device), :]
    return x.reshape(B, perm.shape[0], n3)


def _s2_diagonal(nspins: Tuple[int, int]) -> float:
    na, nb = max(nspins), min(nspins)
    sz = 0.5 * (na - nb)
    return sz * (sz + 1.0) + nb


def make_s2(signed_network, nspins: Sequence[int], assign_spin: bool = True, states: int = 0):
    """See the module docstring.  The returned estimator also carries
    ``s2_estimator.pair_ratios(params, data)`` -> the complex ratios psi(x_{i<->j}) / psi(x),
    [B, n_up, n_down]."""
    if not assign_spin:
        raise NotImplementedError("make_s2: assign_spin=False (sampled spin configurations) is not built; the "
                                  "network's spin assignment is fixed by its spin tables")
    if states:
        raise NotImplementedError("make_s2: states != 0 (the excited-state machinery) is not built")
    nspins = (int(nspins[0]), int(nspins[1]))
    diag = _s2_diagonal(nspins)
    net = network_of(signed_network, None)

    if net is not None:
        if tuple(net.nspins) != nspins:
            raise ValueError(f"make_s2: nspins={nspins} differ from the network's {tuple(net.nspins)}")

        def _pairs(params, data):
            ctx, pos = net.bind_positions(params, data.positions, data.atoms)
            return pos, ctx.spin_squared(pos, want_pairs=True)

        def s2_estimator(params, data, state=None):
            del state
            ctx, pos = net.bind_positions(params, data.positions, data.atoms)
            return ctx.spin_squared(pos).reshape(pos.shape[:-1])

        def pair_ratios(params, data):
            pos, (_, dl, dp) = _pairs(params, data)
            r = torch.exp(dl) * torch.complex(torch.cos(dp), torch.sin(dp))
            return r.reshape(*pos.shape[:-1], *nspins)
    else:
        def pair_ratios(params, data):
            pos = as_positions(data.positions)
            n3 = pos.shape[-1]
            flat = pos.reshape(-1, n3)
            up, dn = _spin_slots(data.spins, nspins, n3 // 3)
            x = exchanged_positions(flat, up, dn)
            K = x.shape[1]
            s0, l0 = signed_network(params, flat, data.spins, data.atoms, data.charges)
            s1, l1 = signed_network(params, x.reshape(-1, n3), data.spins, data.atoms, data.charges)
            s0, l0, s1, l1 = (torch.as_tensor(t) for t in (s0, l0, s1, l1))
            s1, l1 = s1.reshape(-1, K), l1.reshape(-1, K)
            mag = torch.exp(l1 - l0[:, None])
            if torch.is_complex(s0) or torch.is_complex(s1):
                unit = s1 / s0[:, None]
            else:
                d = s1 - s0[:, None]
                unit = torch.complex(torch.cos(d), torch.sin(d))
            return (mag * unit).reshape(*pos.shape[:-1], *nspins)

        def s2_estimator(params, data, state=None):
            del state
            r = pair_ratios(params, data)
            return diag - r.sum(dim=(-2, -1))

    s2_estimator.pair_ratios = pair_ratios
    return s2_estimator


def make_dipole(signed_network, states: int = 0):
    """See the module docstring."""
    if states:
        raise NotImplementedError("make_dipole: states != 0 (the excited-state machinery) is not built")
    net = network_of(signed_network, None)

    def dipole_estimator(params, data, state=None):
        del params, state
        pos = as_positions(data.positions)
        if net is not None:
            ctx = net.context(data.atoms, kernel_dtype(pos))
            return ctx.dipole(pos).reshape(*pos.shape[:-1], 3)
        atoms = torch.as_tensor(np.asarray(data.atoms), dtype=pos.dtype, device=pos.device).reshape(-1, 3)
        charges = torch.as_tensor(np.asarray(data.charges), dtype=pos.dtype, device=pos.device).reshape(-1)
        nuc = (charges[:, None] * atoms).sum(0)
        return nuc - pos.reshape(*pos.shape[:-1], -1, 3).sum(-2)

    return dipole_estimator


def batch_mean(values: torch.Tensor) -> torch.Tensor:
    """Mean over the walkers (dim 0) of all ranks: constants.pmean of the rank mean (equal
    per-rank batches, as the drivers require)."""
    return constants.pmean(values.mean(dim=0))


def s2_stats(s2: torch.Tensor):
    """(<S^2>, variance of Re S2_L) over the walkers of all ranks, one all-reduce
    (constants.pmean_stats on the real part)."""
    re = s2.real if torch.is_complex(s2) else s2
    return constants.pmean_stats(re.reshape(-1).contiguous())


# ---- electron density and pair-correlation histograms --------------------------------------------
_ONE = 1 << 32                       # the fixed point of the accumulator words: units of 2^-32
_MAX_WEIGHT = 2147483648.0           # weights at or above 2^31 cannot be represented: skipped


def _density_cfg_checked(grid, radial, pair):
    """The checks of aiqmc_density_layout, with its messages, for the paths that have no context."""
    from . import _lib
    cfg = _lib.density_cfg(grid, radial, pair)
    for d in range(3):
        if cfg.grid_n[d] < 0:
            raise ValueError(f"make_density: negative grid_n[{d}]")
        if cfg.grid_n[d] > _lib.DENSITY_MAX_BINS:
            raise ValueError(f"make_density: grid_n[{d}] above {_lib.DENSITY_MAX_BINS}")
    for name, n in (("rad_n", cfg.rad_n), ("pair_n", cfg.pair_n)):
        if n < 0:
            raise ValueError(f"make_density: negative {name}")
        if n > _lib.DENSITY_MAX_BINS:
            raise ValueError(f"make_density: {name} above {_lib.DENSITY_MAX_BINS}")
    if all(cfg.grid_n[d] > 0 for d in range(3)):
        for d in range(3):
            w = cfg.grid_hi[d] - cfg.grid_lo[d]
            if not (w > 0 and np.isfinite(w)):
                raise ValueError(f"make_density: grid_hi[{d}] <= grid_lo[{d}] (finite bounds with hi > lo are required)")
    for name, n, r in (("rad_max", cfg.rad_n, cfg.rad_max), ("pair_max", cfg.pair_n, cfg.pair_max)):
        if n > 0 and not (r > 0 and np.isfinite(r)):
            raise ValueError(f"make_density: {name} must be positive and finite when its count is non-zero")
    return cfg


def _density_layout(cfg, natoms: int) -> dict:
    """aiqmc_density_layout's word layout for `natoms` atoms (the host path has no context)."""
    from . import _lib
    grid = all(cfg.grid_n[d] > 0 for d in range(3))
    ng = 2 * cfg.grid_n[0] * cfg.grid_n[1] * cfg.grid_n[2] if grid else 0
    nr, npair = 2 * natoms * cfg.rad_n, 3 * cfg.pair_n
    sizes = [1, 1, ng, 2 if grid else 0, nr, 2 * natoms if nr else 0, npair, 3 if npair else 0]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if int(off[-1]) > _lib.DENSITY_MAX_WORDS:
        raise ValueError(f"make_density: accumulator of {int(off[-1])} words is above {_lib.DENSITY_MAX_WORDS}")
    return {"offsets": dict(zip(_lib.DENSITY_FIELDS, (int(o) for o in off[:-1]))),
            "sizes": dict(zip(_lib.DENSITY_FIELDS, sizes)), "n_words": int(off[-1]),
            "privatised": int(off[-1] - off[4]) <= _lib.DENSITY_LDS_WORDS}


class DensityAccumulator:
    """See ``make_density``.  The state is ONE int64 tensor of fixed-point words (units of 2^-32)
    in the layout of include/aiqmc.h (``aiqmc_density_layout``), allocated at the first ``update``
    on the device of its walkers and only ever added to."""

    def __init__(self, signed_network, nspins, grid, radial, pair):
        self.nspins = (int(nspins[0]), int(nspins[1]))
        self._net = network_of(signed_network, None)
        if self._net is not None and tuple(self._net.nspins) != self.nspins:
            raise ValueError(f"make_density: nspins={self.nspins} differ from the network's {tuple(self._net.nspins)}")
        self.cfg = _density_cfg_checked(grid, radial, pair)
        self.natoms = None
        self.layout = None
        self.words = None

    # -- state ---------------------------------------------------------------------------------
    def _ensure(self, natoms: int, device) -> None:
        if self.words is None:
            self.natoms = int(natoms)
            self.layout = _density_layout(self.cfg, self.natoms)
            self.words = torch.zeros(self.layout["n_words"], dtype=torch.int64, device=device)
        elif int(natoms) != self.natoms:
            raise ValueError(f"density accumulator holds {self.natoms} atoms, the data has {int(natoms)}")
        elif self.words.device != torch.device(device):
            self.words = self.words.to(device)

    def _need(self):
        if self.words is None:
            raise RuntimeError("density accumulator is empty: call update() (or load_state_dict) first")

    @property
    def counts(self) -> dict:
        """Named int64 views of the words: total [1], skipped [1], grid [2, nx, ny, nz], grid_out [2],
        radial [2, A, rad_n], radial_out [2, A], pair [3, pair_n], pair_out [3] (absent families empty)."""
        self._need()
        c, A = self.cfg, self.natoms
        shapes = {"total": (1,), "skipped": (1,), "grid": (2, c.grid_n[0], c.grid_n[1], c.grid_n[2]), "grid_out": (2,),
                  "radial": (2, A, c.rad_n), "radial_out": (2, A), "pair": (3, c.pair_n), "pair_out": (3,)}
        out = {}
        for k, o in self.layout["offsets"].items():
            n = self.layout["sizes"][k]
            out[k] = self.words[o:o + n].view(shapes[k] if n else (0,))
        return out

    def reset(self) -> None:
        if self.words is not None:
            self.words.zero_()

    def _config_tensors(self, natoms: int) -> dict:
        c = self.cfg
        return {"natoms": torch.tensor(int(natoms)), "nspins": torch.tensor(self.nspins),
                "grid_lo": torch.tensor(list(c.grid_lo), dtype=torch.float64),
                "grid_hi": torch.tensor(list(c.grid_hi), dtype=torch.float64), "grid_n": torch.tensor(list(c.grid_n)),
                "radial": torch.tensor([c.rad_max, float(c.rad_n)], dtype=torch.float64),
                "pair": torch.tensor([c.pair_max, float(c.pair_n)], dtype=torch.float64)}

    def state_dict(self) -> dict:
        """Plain tensors (host copies), safe to checkpoint: the words and the configuration."""
        self._need()
        return {"words": self.words.detach().cpu().clone(), **self._config_tensors(self.natoms)}

    def load_state_dict(self, d: dict) -> None:
        """Restores the words; the configuration in `d` must be this accumulator's."""
        natoms = int(d["natoms"])
        for k, v in self._config_tensors(self.natoms if self.natoms is not None else natoms).items():
            if not torch.equal(torch.as_tensor(d[k]).to(v.dtype), v):
                raise ValueError(f"load_state_dict: {k} differs from this accumulator's configuration")
        w = torch.as_tensor(d["words"])
        if w.dtype != torch.int64 or w.numel() != _density_layout(self.cfg, natoms)["n_words"]:
            raise ValueError("load_state_dict: words must be the int64 tensor of this layout")
        self._ensure(natoms, self.words.device if self.words is not None else w.device)
        self.words.copy_(w.reshape(-1))

    # -- accumulation ----------------------------------------------------------------------------
    def update(self, params, data, weights=None) -> None:
        """Bins every walker of ``data.positions [..., 3N]`` (weights: one per walker, or None for
        unit weights).  No host synchronisation on the kernel path."""
        del params   # the density needs the walkers only
        pos = as_positions(data.positions)
        n3 = pos.shape[-1]
        if n3 != 3 * sum(self.nspins):
            raise ValueError(f"positions have {n3 // 3} electrons, nspins={self.nspins}")
        if self._net is not None:
            ctx = self._net.context(data.atoms, kernel_dtype(pos))
            self._ensure(ctx.A, ctx.device)
            ctx.density_accumulate(pos, self.words, self.cfg, weights)
            return
        flat = pos.reshape(-1, n3)
        if flat.dtype not in (torch.float32, torch.float64):
            flat = flat.to(torch.float32)
        atoms = torch.as_tensor(np.asarray(data.atoms.detach().cpu() if isinstance(data.atoms, torch.Tensor)
                                           else data.atoms, dtype=np.float64)).reshape(-1, 3)
        self._ensure(atoms.shape[0], flat.device)
        up, dn = _spin_slots(data.spins, self.nspins, n3 // 3)
        self._host_update(flat, atoms.to(flat.device, flat.dtype), up, dn, weights)

    def _host_update(self, pos, atoms, up, dn, weights) -> None:
        """The kernel's arithmetic in torch, in the dtype T of the positions: the same bin rule,
        the same fixed point, integer index_add_."""
        c, off, T, dev = self.cfg, self.layout["offsets"], pos.dtype, pos.device
        B, N, A = pos.shape[0], pos.shape[1] // 3, atoms.shape[0]
        if weights is None:
            q = torch.full((B,), _ONE, dtype=torch.int64, device=dev)
            ok = torch.ones(B, dtype=torch.bool, device=dev)
        else:
            w = torch.as_tensor(weights).to(dev, T).reshape(-1).double()
            if w.numel() != B:   # no context on the host path: the message of _lib.Context._weights
                raise ValueError("weights must have one entry per walker")
            ok = (w >= 0.0) & (w < _MAX_WEIGHT)
            q = torch.where(ok, torch.round(torch.where(ok, w, torch.zeros_like(w)) * float(_ONE)),
                            torch.zeros_like(w)).to(torch.int64)
        tt = lambda v: torch.tensor(v, dtype=T, device=dev)
        x = pos.reshape(B, N, 3)
        chan = torch.ones(N, dtype=torch.int64, device=dev)
        chan[torch.as_tensor(np.asarray(up), device=dev)] = 0
        idx, val = [torch.tensor([0, 1], device=dev)], [torch.stack([q.sum(), (~ok).sum()])]

        def binned(f, n):
            inside = (f >= 0) & (f < tt(float(n)))
            return inside, torch.floor(torch.where(inside, f, torch.zeros_like(f))).to(torch.int64)

        if self.layout["sizes"]["grid"]:
            ins, g = torch.ones(B, N, dtype=torch.bool, device=dev), chan.expand(B, N)
            for d in range(3):
                inv = c.grid_n[d] / (c.grid_hi[d] - c.grid_lo[d])
                i_d, b_d = binned((x[..., d] - tt(c.grid_lo[d])) * tt(inv), c.grid_n[d])
                ins, g = ins & i_d, g * c.grid_n[d] + b_d
            idx.append(torch.where(ins, off["grid"] + g, off["grid_out"] + chan.expand(B, N)))
            val.append(q[:, None].expand(B, N))
        if c.rad_n > 0:
            d = x[:, :, None, :] - atoms[None, None]
            r = torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])   # [B, N, A]
            ins, b = binned(r * tt(c.rad_n / c.rad_max), c.rad_n)
            ca = chan[None, :, None] * A + torch.arange(A, device=dev)[None, None, :]
            idx.append(torch.where(ins, off["radial"] + ca * c.rad_n + b, off["radial_out"] + ca.expand(B, N, A)))
            val.append(q[:, None, None].expand(B, N, A))
        if c.pair_n > 0 and N > 1:
            i, j = torch.triu_indices(N, N, offset=1, device=dev)
            d = x[:, i] - x[:, j]
            r = torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])   # [B, P]
            ins, b = binned(r * tt(c.pair_n / c.pair_max), c.pair_n)
            ch = torch.where(chan[i] == chan[j], chan[i], torch.full_like(chan[i], 2))[None].expand(B, -1)
            idx.append(torch.where(ins, off["pair"] + ch * c.pair_n + b, off["pair_out"] + ch))
            val.append(q[:, None].expand(B, i.numel()))
        self.words.index_add_(0, torch.cat([t.reshape(-1) for t in idx]), torch.cat([t.reshape(-1) for t in val]))

    def reduce(self) -> None:
        """SUM all-reduce of the words over the default process group, in place (the identity in
        a single process: ``constants._active()``).  Integer sums: the pooled words are the
        one-process words of the concatenated batch, bit for bit.  Afterwards EVERY rank holds the
        pooled counts, so call it once, when the accumulation is over (or ``reset`` after it)."""
        self._need()
        constants.all_reduce_(self.words)

    # -- normalised results ------------------------------------------------------------------------
    def result(self) -> dict:
        """float64 host tensors, each family's entries present only when the family is:

        ``total``            the summed walker weights, ``skipped`` the number of walkers refused
        ``grid``             [2, nx, ny, nz] density = count / (total dV): integrates to the electrons
                             of that spin inside the box; ``grid_centres`` (x [nx], y [ny], z [nz])
        ``radial``           [2, A, rad_n] = count / (total 4 pi / 3 (r_{k+1}^3 - r_k^3)), the spherically
                             averaged density about each atom; ``radial_centres`` [rad_n]
        ``pair``             [3, pair_n] = count / total, the mean number of pairs per walker in the bin
                             (the ideal-gas normalisation is the caller's); ``pair_centres`` [pair_n]
        ``*_outside``        out / total: the mean number of the channel's samples per walker that
                             fell outside (grid [2], radial [2, A], pair [3]), so that inside plus
                             outside is the channel's number of electrons (or pairs).
        """
        c = {k: v.detach().cpu().double() / float(_ONE) for k, v in self.counts.items() if k != "skipped"}
        total = c["total"][0]
        g = self.cfg
        res = {"total": total, "skipped": self.counts["skipped"].detach().cpu()[0]}
        centres = lambda lo, hi, n: lo + (torch.arange(n, dtype=torch.float64) + 0.5) * ((hi - lo) / n)
        if self.layout["sizes"]["grid"]:
            dv = np.prod([(g.grid_hi[d] - g.grid_lo[d]) / g.grid_n[d] for d in range(3)])
            res["grid"] = c["grid"] / (total * dv)
            res["grid_centres"] = tuple(centres(g.grid_lo[d], g.grid_hi[d], g.grid_n[d]) for d in range(3))
            res["grid_outside"] = c["grid_out"] / total
        if g.rad_n > 0:
            edges = torch.arange(g.rad_n + 1, dtype=torch.float64) * (g.rad_max / g.rad_n)
            shell = 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
            res["radial"] = c["radial"] / (total * shell)
            res["radial_centres"] = centres(0.0, g.rad_max, g.rad_n)
            res["radial_outside"] = c["radial_out"] / total
        if g.pair_n > 0:
            res["pair"] = c["pair"] / total
            res["pair_centres"] = centres(0.0, g.pair_max, g.pair_n)
            res["pair_outside"] = c["pair_out"] / total
        return res


def make_density(signed_network, nspins: Sequence[int], *, grid=None, radial=None, pair=None) -> DensityAccumulator:
    """Spin-resolved electron density and electron-electron pair-distance histograms, accumulated
    across sweeps without leaving the device.

    This is the DIAGONAL density n(r); it needs nothing but the walkers.  The off-diagonal one-body
    density matrix projected on a Gaussian basis is ``make_density_matrix`` below.

    ``grid = (lo[3], hi[3], n[3])`` a 3-D box, ``radial = (r_max, n)`` distances to every atom of
    ``data.atoms``, ``pair = (r_max, n)`` distances of the electron pairs i < j (channels up-up,
    down-down, up-down); None leaves a family out.  Bin rule (in the dtype of the positions):
    f = (x - lo) * (n / (hi - lo)), inside iff 0 <= f < n, bin floor(f); everything else, NaN
    included, goes to the channel's outside word.  The words are integers in units of 2^-32: a
    walker of weight w adds rint(w 2^32) per sample (1 << 32 without weights; capacity 2^31 units
    of weight per bin); a negative, non-finite or >= 2^31 weight skips the walker and is counted.
    Integer sums do not depend on the order: any batching, walker order or rank count gives the
    same bits.

    ``acc.update(params, data, weights=None)``, ``acc.counts``, ``acc.reduce()``, ``acc.result()``,
    ``acc.reset()``, ``acc.state_dict()`` / ``acc.load_state_dict(d)``: see DensityAccumulator.

    If ``signed_network`` is the ``apply`` of an aiqmc network (the detection of ``make_s2``),
    ``update`` runs the HIP kernel of csrc/density.hip on the context of ``data.atoms``; spin
    channels are the network's spin tables.  Any other callable takes a torch path with the same
    arithmetic on the device of the positions; its spin slots come from ``data.spins`` as in
    ``make_s2``.  The callable itself is never evaluated."""
    return DensityAccumulator(signed_network, nspins, grid, radial, pair)


# ---- one-body reduced density matrix in a Gaussian basis ----------------------------------------
_NCART = (1, 3, 6)                                      # functions of an l = 0, 1, 2 Cartesian shell
_CART = ((), ((0,), (1,), (2,)), ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)))   # 1 | x y z | xx xy xz yy yz zz
_KIND_RDM_NORMAL, _KIND_RDM_COMPONENT = 24, 25          # Philox kinds of the points r' 


def _philox_u4(seed: int, step: int, sid, kind: int) -> np.ndarray:
    """Host replica of the device draw philox_u4 (csrc/jets.h): four uniforms [4, n] on the 24-bit
    grid in (0, 1] from counter {sid, step lo, step hi, kind} and key {seed lo, seed hi},
    Philox4x32-10.  The grid values are exact in float32 and float64."""
    seed, step = int(seed), int(step)
    if not (0 <= seed < 2 ** 64 and 0 <= step < 2 ** 64):
        raise ValueError("seed and step are unsigned 64-bit")
    m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    sid = np.asarray(sid, dtype=np.uint64) & m32
    c = [sid, np.full_like(sid, step & 0xFFFFFFFF), np.full_like(sid, step >> 32), np.full_like(sid, kind)]
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return ((np.stack(c) >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24


def _philox_normal3(seed: int, step: int, sid, kind: int) -> np.ndarray:
    """Three standard normals [3, n]: Box-Muller on the four uniforms in float64, in the order of
    the device's philox_normal3f (r0 cos, r0 sin, r1 cos)."""
    u = _philox_u4(seed, step, sid, kind)
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    a0, a1 = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1)])


def _double_factorial(n: int) -> int:
    return 1 if n <= 0 else n * _double_factorial(n - 2)


def normalized_shell(l: int, exponents, coefs) -> np.ndarray:
    """The contraction coefficients with the primitive norms folded in: coefs[p] N(l, exponents[p]),
    N(l, a) = [(2a / pi)^{3/2} (4a)^l / (2l - 1)!!]^{1/2}, the norm of the primitive x^l exp(-a r^2).
    That ONE norm is used for every function of the shell, so for l = 2 the xx, yy, zz members of
    a single primitive have unit self-overlap and xy, xz, yz have 1/3 (the usual Cartesian
    convention).  The contraction as a whole is not renormalised."""
    l = int(l)
    if not 0 <= l <= 2:
        raise ValueError("normalized_shell: l must be 0, 1 or 2")
    a = np.asarray(exponents, dtype=np.float64).reshape(-1)
    c = np.asarray(coefs, dtype=np.float64).reshape(-1)
    if a.shape != c.shape or not np.all(a > 0):
        raise ValueError("normalized_shell: exponents (positive) and coefs must have the same length")
    return c * np.sqrt((2.0 * a / np.pi) ** 1.5 * (4.0 * a) ** l / _double_factorial(2 * l - 1))


class Shell:
    """A contracted Cartesian Gaussian shell: the functions x^a y^b z^c sum_p coefs[p] exp(-exponents[p] r^2)
    about `center` (any point, not necessarily an atom), in the order 1 | x y z | xx xy xz yy yz zz.
    The coefficients are applied as given (``normalized_shell`` folds the primitive norms in)."""

    def __init__(self, center, l: int, exponents, coefs):
        self.center = np.asarray(center, dtype=np.float64).reshape(3)
        self.l = int(l)
        self.exponents = np.asarray(exponents, dtype=np.float64).reshape(-1)
        self.coefs = np.asarray(coefs, dtype=np.float64).reshape(-1)
        if not 0 <= self.l <= 2:
            raise ValueError(f"Shell: l = {self.l} is not built (l must be 0, 1 or 2)")
        if self.exponents.size < 1 or self.exponents.shape != self.coefs.shape:
            raise ValueError("Shell: exponents and coefs must have the same, non-zero length")
        if not (np.all(np.isfinite(self.exponents)) and np.all(np.isfinite(self.coefs)) and np.all(self.exponents > 0)):
            raise ValueError("Shell: exponents must be positive, exponents and coefs finite")


class GaussianBasis:
    """Shells and optional MO coefficients.  ``mo_coeff`` [2, nao, norb] (per spin) or [nao, norb]
    (both spins) makes the functions phi^s_j = sum_a ao_a mo_coeff[s, a, j]; None: the nao shell
    functions themselves.  Limits (those of the kernels): nao <= 128, norb <= 64, at most 512
    primitives."""

    def __init__(self, shells: Sequence[Shell], mo_coeff=None):
        from . import _lib
        self.shells = list(shells)
        if not self.shells or not all(isinstance(s, Shell) for s in self.shells):
            raise ValueError("GaussianBasis: a non-empty sequence of Shell is required")
        self.shell_l = np.array([s.l for s in self.shells], dtype=np.int32)
        self.shell_nprim = np.array([s.exponents.size for s in self.shells], dtype=np.int32)
        self.shell_center = np.stack([s.center for s in self.shells])
        self.exps = np.concatenate([s.exponents for s in self.shells])
        self.coefs = np.concatenate([s.coefs for s in self.shells])
        self.nao = int(sum(_NCART[s.l] for s in self.shells))
        if self.nao > _lib.RDM_MAX_AO:
            raise ValueError(f"GaussianBasis: nao = {self.nao} above {_lib.RDM_MAX_AO}")
        if self.exps.size > _lib.RDM_MAX_PRIM:
            raise ValueError(f"GaussianBasis: {self.exps.size} primitives above {_lib.RDM_MAX_PRIM}")
        self.mo_coeff = None
        if mo_coeff is not None:
            mo = np.asarray(mo_coeff.detach().cpu() if isinstance(mo_coeff, torch.Tensor) else mo_coeff, dtype=np.float64)
            if mo.ndim == 2:
                mo = np.stack([mo, mo])
            if mo.ndim != 3 or mo.shape[0] != 2 or mo.shape[1] != self.nao:
                raise ValueError(f"GaussianBasis: mo_coeff must be [2, nao={self.nao}, norb] or [nao, norb]")
            self.mo_coeff = np.ascontiguousarray(mo)
        self.norb = self.nao if self.mo_coeff is None else int(self.mo_coeff.shape[2])
        if not 1 <= self.norb <= _lib.RDM_MAX_ORB:
            raise ValueError(f"GaussianBasis: norb = {self.norb} outside [1, {_lib.RDM_MAX_ORB}]")

    @property
    def alpha_min(self) -> float:
        return float(self.exps.min())

    def ao_values(self, points: torch.Tensor) -> torch.Tensor:
        """[..., nao] float64 values of the shell functions at points [..., 3] (torch, any device)."""
        p = points.to(torch.float64)
        out = []
        k = 0
        for s in self.shells:
            d = p - torch.as_tensor(s.center, device=p.device)
            r2 = (d * d).sum(-1)
            rad = torch.zeros_like(r2)
            for a, c in zip(s.exponents, s.coefs):
                rad = rad + float(c) * torch.exp(-float(a) * r2)
            for idx in (_CART[s.l] if s.l else ((),)):
                v = rad
                for ax in idx:
                    v = v * d[..., ax]
                out.append(v)
            k += _NCART[s.l]
        return torch.stack(out, dim=-1)

    def values(self, points: torch.Tensor, spin: int = 0) -> torch.Tensor:
        """[..., norb] float64: the functions of spin channel `spin` at points [..., 3]."""
        ao = self.ao_values(points)
        if self.mo_coeff is None:
            return ao
        return ao @ torch.as_tensor(self.mo_coeff[int(spin)], device=ao.device)

    def _tensors(self) -> dict:
        mo = self.mo_coeff if self.mo_coeff is not None else np.zeros((0,))
        return {"shell_l": torch.tensor(self.shell_l), "shell_nprim": torch.tensor(self.shell_nprim),
                "shell_center": torch.tensor(self.shell_center), "exps": torch.tensor(self.exps),
                "coefs": torch.tensor(self.coefs), "mo_coeff": torch.tensor(mo)}


class Mixture:
    """q(r) = sum_k p_k (2 pi s_k^2)^{-3/2} exp(-|r - c_k|^2 / (2 s_k^2)): see ``mixture``."""

    def __init__(self, centres, sigmas, probs=None):
        from . import _lib
        self.centres = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
        n = self.centres.shape[0]
        self.sigmas = np.broadcast_to(np.asarray(sigmas, dtype=np.float64).reshape(-1), (n,)).copy()
        self.probs = np.full(n, 1.0 / n) if probs is None else np.asarray(probs, dtype=np.float64).reshape(-1)
        if not 1 <= n <= _lib.RDM_MAX_Q:
            raise ValueError(f"mixture: {n} components (1 .. {_lib.RDM_MAX_Q} are allowed)")
        if self.probs.shape != (n,):
            raise ValueError("mixture: one probability per centre")
        if not (np.all(self.sigmas > 0) and np.all(np.isfinite(self.sigmas))):
            raise ValueError("mixture: every sigma must be positive and finite")
        if not np.all(self.probs > 0):
            raise ValueError("mixture: every probability must be positive")
        if not abs(float(np.sum(self.probs)) - 1.0) <= 1e-12:
            raise ValueError("mixture: the probabilities must sum to 1 (within 1e-12)")
        self.cum = np.cumsum(self.probs)      # sequential partial sums in float64, as the library forms them

    def density(self, r: torch.Tensor) -> torch.Tensor:
        """q at r [..., 3], float64."""
        r = r.to(torch.float64)
        q = torch.zeros(r.shape[:-1], dtype=torch.float64, device=r.device)
        for c, s, p in zip(self.centres, self.sigmas, self.probs):
            d = r - torch.as_tensor(c, device=r.device)
            v = 2.0 * np.pi * s * s
            q = q + float(p / (v * np.sqrt(v))) * torch.exp(-float(0.5 / (s * s)) * (d * d).sum(-1))
        return q

    def component(self, u) -> np.ndarray:
        """The smallest k with u < p_0 + .. + p_k; the last component takes what is left."""
        return np.minimum(np.searchsorted(self.cum, np.asarray(u, dtype=np.float64), side="right"), len(self.cum) - 1)

    def sample(self, seed: int, step: int, B: int, S: int) -> np.ndarray:
        """The points r' [B, S, 3] (float64) of the Philox mode: stream id b S + s; kind 25's first
        uniform picks the component, kind 24's three normals g give r' = c_k + s_k g.  Exact
        sampling of q: no chain, no burn-in."""
        sid = np.arange(B * S, dtype=np.uint64)
        g = _philox_normal3(seed, step, sid, _KIND_RDM_NORMAL)
        k = self.component(_philox_u4(seed, step, sid, _KIND_RDM_COMPONENT)[0])
        return (self.centres[k] + self.sigmas[k][:, None] * g.T).reshape(B, S, 3)

    def _tensors(self) -> dict:
        return {"q_center": torch.tensor(self.centres), "q_sigma": torch.tensor(self.sigmas),
                "q_prob": torch.tensor(self.probs)}


def mixture(centres, sigmas, probs=None) -> Mixture:
    """The importance density of the points r': a mixture of at most 16 isotropic Gaussians with
    centres [n, 3], widths sigmas (one, or one per centre) and probabilities probs (> 0, summing to
    1 within 1e-12; None: 1 / n each).  phi_j / q stays bounded iff sigma_k^2 >= 1 / (2 alpha_min)
    for the smallest exponent alpha_min of the basis (and some component covers each function's
    centre): choose the widths no smaller, or the estimator's variance is infinite."""
    return Mixture(centres, sigmas, probs)


def _moved_positions(pos: torch.Tensor, rprime: torch.Tensor) -> torch.Tensor:
    """[B, S, N, 3N]: pos [B, 3N] with electron slot e at rprime[b, s]."""
    B, n3 = pos.shape
    N, S = n3 // 3, rprime.shape[1]
    x = pos.reshape(B, 1, 1, N, 3).expand(B, S, N, N, 3).clone()
    e = torch.arange(N, device=pos.device)
    x[:, :, e, e, :] = rprime[:, :, None, :].expand(B, S, N, 3).to(pos.dtype)
    return x.reshape(B, S, N, n3)


class DensityMatrixAccumulator:
    """See ``make_density_matrix``.  The state is ONE float64 tensor: the number of updates, then
    the sum over updates of each update's vector v = [W, sums [2, K, K, (re, im)]] and the sum of
    its element-wise squares -- one SUM all-reduce pools it over ranks."""

    def __init__(self, signed_network, nspins, basis: GaussianBasis, q, samples: int):
        self.nspins = (int(nspins[0]), int(nspins[1]))
        if not isinstance(basis, GaussianBasis):
            raise TypeError("make_density_matrix: basis must be a GaussianBasis")
        if q is not None and not isinstance(q, Mixture):
            raise TypeError("make_density_matrix: q must be a mixture(...) or None")
        self.samples = int(samples)
        if self.samples < 1:
            raise ValueError("make_density_matrix: samples must be at least 1")
        self._f = signed_network
        self._net = network_of(signed_network, None)
        if self._net is not None and tuple(self._net.nspins) != self.nspins:
            raise ValueError(f"make_density_matrix: nspins={self.nspins} differ from the network's "
                             f"{tuple(self._net.nspins)}")
        self.basis, self.q = basis, q
        self.K = basis.norb
        self.n = 1 + 4 * self.K * self.K
        self.state = None
        self._last = None
        self.last_rprime = None
        self._token = None

    # -- state ---------------------------------------------------------------------------------
    def _ensure(self, atoms, device) -> None:
        if self.q is None:   # one component per atom, as wide as the most diffuse primitive needs
            a = np.asarray(atoms.detach().cpu() if isinstance(atoms, torch.Tensor) else atoms, dtype=np.float64)
            a = a.reshape(-1, a.shape[-2], 3)[0] if a.ndim == 3 else a.reshape(-1, 3)
            self.q = Mixture(a, np.sqrt(0.5 / self.basis.alpha_min))
        if self.state is None:
            self.state = torch.zeros(1 + 2 * self.n, dtype=torch.float64, device=device)
        elif self.state.device != torch.device(device):
            self.state = self.state.to(device)

    def _need(self):
        if self.state is None:
            raise RuntimeError("density-matrix accumulator is empty: call update() (or load_state_dict) first")

    def reset(self) -> None:
        if self.state is not None:
            self.state.zero_()
        self._last = None

    def _config_tensors(self) -> dict:
        if self.q is None:
            raise RuntimeError("density-matrix accumulator has no q yet: call update() first, or pass q")
        return {"nspins": torch.tensor(self.nspins), "samples": torch.tensor(self.samples),
                **self.basis._tensors(), **self.q._tensors()}

    def state_dict(self) -> dict:
        """Plain host tensors, safe to checkpoint: the state and the configuration (basis, q, samples)."""
        self._need()
        return {"state": self.state.detach().cpu().clone(), **self._config_tensors()}

    def load_state_dict(self, d: dict) -> None:
        """Restores the sums; the basis, q, samples and nspins in `d` must be this accumulator's."""
        if self.q is None:
            self.q = Mixture(np.asarray(d["q_center"]), np.asarray(d["q_sigma"]), np.asarray(d["q_prob"]))
        for k, v in self._config_tensors().items():
            o = torch.as_tensor(np.asarray(d[k])).to(v.dtype)
            if o.shape != v.shape or not torch.equal(o, v):
                raise ValueError(f"load_state_dict: {k} differs from this accumulator's configuration")
        st = torch.as_tensor(np.asarray(d["state"]))
        if st.dtype != torch.float64 or st.numel() != 1 + 2 * self.n:
            raise ValueError("load_state_dict: state must be the float64 tensor of this layout")
        dev = self.state.device if self.state is not None else st.device
        self.state = st.reshape(-1).clone().to(dev)
        self._last = None

    # -- accumulation ----------------------------------------------------------------------------
    def _key(self, key, B: int, pos: torch.Tensor):
        """(injected rprime [B, S, 3] or None, seed, step)."""
        from .VMC.VMCmcstep import philox_key
        if isinstance(key, (torch.Tensor, np.ndarray)):
            r = torch.as_tensor(key)
            if tuple(r.shape) != (B, self.samples, 3):
                raise ValueError(f"injected rprime must be [B={B}, S={self.samples}, 3], got {tuple(r.shape)}")
            return r.to(pos.device), 0, 0
        k = philox_key(key)
        return None, int(k.seed), int(k.offset)

    def update(self, params, data, key, weights=None) -> None:
        """One estimate from the walkers ``data.positions [..., 3N]`` (~ |psi|^2; weights: one per
        walker or None).  key: an int seed or a ``PhiloxKey`` (seed, offset) -- the points are drawn
        from q, a different (seed, offset) per update -- or a tensor of injected points
        rprime [B, S, 3].  No host synchronisation on the kernel path."""
        pos = as_positions(data.positions)
        n3 = pos.shape[-1]
        if n3 != 3 * sum(self.nspins):
            raise ValueError(f"positions have {n3 // 3} electrons, nspins={self.nspins}")
        B = pos.numel() // n3
        if self._net is not None:
            ctx, pos = self._net.bind_positions(params, pos, data.atoms)
            self._ensure(data.atoms, ctx.device)
            rprime, seed, step = self._key(key, B, pos)
            ctx.set_rdm_basis(self.basis.shell_l, self.basis.shell_nprim, self.basis.shell_center, self.basis.exps,
                              self.basis.coefs, self.basis.mo_coeff, self.q.centres, self.q.sigmas, self.q.probs,
                              token=self._table_token())
            v = ctx.rdm_accumulate(pos, self.samples, rprime=rprime, seed=seed, step=step, weights=weights)
        else:
            flat = pos.reshape(-1, n3)
            self._ensure(data.atoms, flat.device)
            rprime, seed, step = self._key(key, B, flat)
            if rprime is None:
                rprime = torch.as_tensor(self.q.sample(seed, step, B, self.samples)).to(flat.device)
            if flat.dtype in (torch.float32, torch.float64):
                rprime = rprime.to(flat.dtype)      # r' = c + sigma g, rounded once to the operand dtype
            self.last_rprime = rprime
            v = self._generic(params, data, flat, rprime, weights)
        self._last = v
        n = self.n
        self.state[0] += 1.0
        self.state[1:1 + n] += v
        self.state[1 + n:] += v * v

    def _table_token(self):
        if self._token is None:
            import hashlib
            h = hashlib.sha1()
            for t in self._config_tensors().values():
                h.update(t.numpy().tobytes())
                h.update(str(tuple(t.shape)).encode())
            self._token = h.hexdigest()
        return self._token

    def _generic(self, params, data, pos, rprime, weights) -> torch.Tensor:
        """The formula in torch (float64 / complex128) on the device of the positions: one call of
        the network on the walkers, one on all B S N moved configurations."""
        B, n3 = pos.shape
        N, S, K = n3 // 3, self.samples, self.K
        up, dn = _spin_slots(data.spins, self.nspins, N)
        x = _moved_positions(pos, rprime)
        s0, l0 = self._f(params, pos, data.spins, data.atoms, data.charges)
        s1, l1 = self._f(params, x.reshape(-1, n3), data.spins, data.atoms, data.charges)
        s0, l0, s1, l1 = (torch.as_tensor(t) for t in (s0, l0, s1, l1))
        s1, l1 = s1.reshape(B, S, N), l1.reshape(B, S, N)
        mag = torch.exp((l1 - l0[:, None, None]).to(torch.float64))
        if torch.is_complex(s0) or torch.is_complex(s1):
            unit = (s1 / s0[:, None, None]).to(torch.complex128)
        else:
            d = (s1 - s0[:, None, None]).to(torch.float64)
            unit = torch.complex(torch.cos(d), torch.sin(d))
        w = (torch.ones(B, dtype=torch.float64, device=pos.device) if weights is None
             else torch.as_tensor(weights).to(pos.device, torch.float64).reshape(-1))
        if w.numel() != B:
            raise ValueError("weights must have one entry per walker")
        rp = rprime.to(torch.float64)
        f = mag * unit * (w[:, None] / self.q.density(rp))[:, :, None]          # [B, S, N]
        r = pos.reshape(B, N, 3).to(torch.float64)
        out = torch.zeros(2, K, K, dtype=torch.complex128, device=pos.device)
        for sg, slots in enumerate((up, dn)):
            if len(slots) == 0:
                continue
            sl = torch.as_tensor(np.asarray(slots), device=pos.device)
            a = self.basis.values(r[:, sl], sg).to(torch.complex128)            # [B, ns, K]
            p = self.basis.values(rp, sg).to(torch.complex128)                  # [B, S, K]
            out[sg] = torch.einsum("bei,bsj,bse->ij", a, p, f[:, :, sl])
        return torch.cat([w.sum().reshape(1), torch.view_as_real(out).reshape(-1)])

    def last(self) -> torch.Tensor:
        """This update's normalised matrix [2, K, K], complex128."""
        if self._last is None:
            raise RuntimeError("density-matrix accumulator: no update since the last reset / load")
        v = self._last
        return torch.view_as_complex(v[1:].clone().reshape(2, self.K, self.K, 2)) / (v[0] * self.samples)

    def reduce(self) -> None:
        """SUM all-reduce of the state over the default process group, in place (the identity in a
        single process).  Afterwards EVERY rank holds the pooled sums, each (rank, update) counted
        as one update: call it once, when the accumulation is over (or ``reset`` after it)."""
        self._need()
        constants.all_reduce_(self.state)

    # -- normalised results ------------------------------------------------------------------------
    def result(self, natural_orbitals: bool = False) -> dict:
        """Host tensors:

        ``rho``          [2, K, K] complex128 = sums / (W S) over all updates
        ``rho_h``        its Hermitian part (rho + rho^H) / 2
        ``stderr``       [2, K, K] complex128: the standard error of the real part in .real, of the
                         imaginary part in .imag, from the spread of the per-update sums.  It ASSUMES
                         decorrelated updates (use every few correlation times, or treat it as a
                         lower bound) and equal total weight per update; NaN for a single update.
        ``trace``        [2] = Re tr rho_h: the electrons of the channel that the basis captures
        ``occupations``  [2, K] eigenvalues of rho_h (torch.linalg.eigvalsh, float64), descending
        ``natural_orbitals`` (on request) [2, K, K], column k the eigenvector of occupations[:, k]
        ``updates``, ``total_weight``
        """
        self._need()
        st = self.state.detach().cpu()
        n, K, S = self.n, self.K, self.samples
        cnt, tot, sq = float(st[0]), st[1:1 + n], st[1 + n:]
        W = tot[0]
        cx = lambda t: torch.view_as_complex(t.clone().reshape(2, K, K, 2))
        rho = cx(tot[1:]) / (W * S)
        rho_h = 0.5 * (rho + rho.conj().transpose(-1, -2))
        if cnt > 1:
            var = torch.clamp(sq[1:] / cnt - (tot[1:] / cnt) ** 2, min=0.0) * (cnt / (cnt - 1.0))
            err = cx(torch.sqrt(var / cnt)) / ((W / cnt) * S)
        else:
            err = torch.full((2, K, K), float("nan"), dtype=torch.complex128)
        res = {"rho": rho, "rho_h": rho_h, "stderr": err, "trace": torch.einsum("sii->s", rho_h).real,
               "updates": int(cnt), "total_weight": W}
        if natural_orbitals:
            ev, vec = torch.linalg.eigh(rho_h)
            res["occupations"], res["natural_orbitals"] = ev.flip(-1), vec.flip(-1)
        else:
            res["occupations"] = torch.linalg.eigvalsh(rho_h).flip(-1)
        return res


def make_density_matrix(signed_network, nspins: Sequence[int], basis: GaussianBasis, *, q: Mixture = None,
                        samples: int = 1, states: int = 0) -> DensityMatrixAccumulator:
    """One-body reduced density matrix rho(r, r') projected on a Gaussian basis supplied by the
    caller (the name and purpose of ferminet/observables.py ``make_density_matrix``; the SCF basis
    it takes from pyscf is replaced by ``basis``), accumulated across sweeps.

    For each spin channel s, functions phi_1..phi_K, walkers x_b ~ |psi|^2 with weights w_b and
    S = ``samples`` points r'_bs' per walker drawn from the known density q,

        rho^s_ij = 1 / (W S) sum_b w_b sum_s' sum_{e in s} phi_i(r_e) phi_j(r'_bs')
                   psi(x_b; r_e -> r'_bs') / psi(x_b) / q(r'_bs'),          W = sum_b w_b,

    summed over EVERY electron of the channel: this ansatz is not antisymmetric under same-spin
    exchange (per-electron convolution weights and envelopes), so ferminet's "first electron of
    each spin" would not be the density matrix of this psi.  The same point serves all N
    electrons of its walker: N S + 1 value forwards per walker.  psi is complex, so rho is (the
    package's convention for complex per-walker quantities).  For an orthonormal basis tr rho^s
    tends to the electrons of the channel as the basis becomes complete, and the eigenvalues of
    the Hermitian part are the natural-orbital occupations.

    ``q``: ``mixture(centres, sigmas, probs)``; None places one component on every atom of
    ``data.atoms`` with p = 1 / A and sigma^2 = 1 / (2 alpha_min), the smallest width for which
    phi_j / q stays bounded.  q is sampled exactly (Philox kinds 24 / 25, see ``Mixture.sample``),
    so there is no Markov chain for r' and no burn-in; ferminet's chain over the Hartree-Fock
    density is deliberately NOT reproduced.

    ``acc.update(params, data, key, weights=None)``, ``acc.last()``, ``acc.reduce()``,
    ``acc.result()``, ``acc.reset()``, ``acc.state_dict()`` / ``acc.load_state_dict(d)``: see
    DensityMatrixAccumulator.

    If ``signed_network`` is the ``apply`` of an aiqmc network (the detection of ``make_s2``),
    ``update`` runs the HIP kernels of csrc/rdm.hip on the context of ``data.atoms``; the channels
    are the network's spin tables.  Any other callable (the convention of ``make_s2``) takes a
    batched torch path with the same formula and the same points; its spin slots come from
    ``data.spins``."""
    if states:
        raise NotImplementedError("make_density_matrix: states != 0 (the excited-state machinery) is not built")
    return DensityMatrixAccumulator(signed_network, nspins, basis, q, samples)
