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
            if w.numel() != B:
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

    This is the DIAGONAL density n(r), not ferminet/observables.py's ``make_density_matrix``: that
    one projects the one-body density matrix on the orbitals of a pyscf SCF calculation, and that
    basis does not exist here.  The diagonal needs nothing but the walkers.

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
