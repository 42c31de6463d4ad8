"""Error bars for serially correlated Monte Carlo series: an online blocking accumulator.

A VMC or DMC run averages over consecutive sweeps of the same Markov chains, so its samples are
serially correlated and sqrt(variance / n) underestimates the error of the mean by sqrt(2 tau_int).
The blocking method (Flyvbjerg and Petersen, J. Chem. Phys. 91, 461 (1989)) replaces the series by
the means of blocks of 2^k consecutive samples; once the blocks are longer than the correlation
time the naive error of the block means stops growing and IS the error of the mean.  Here it runs
online, in O(log T) memory: nothing but per-level sums and one waiting block per level and chain.

    acc = statistics.make_blocking()            # one series, 24 levels
    for it in range(iterations):
        ...                                     # sweeps, local energy e_l [B] on the device
        acc.update(e_l)                         # two small launches, no host synchronisation
    acc.reduce()                                # multi-rank runs: pool the ranks' chains
    r = acc.result()
    print(r["mean"][0], "+/-", r["stderr_opt"], "2 tau_int =", r["inefficiency"])

Definitions (the same in include/aiqmc.h, csrc/blocking.hip and the torch path below).  A sample is
one call's values x[i][b], series i < K, chain b < B: the SAME chains in the same order at every
call.  With t the number of samples taken before this one,
    v_0 = x - shift completes level 0; for k = 0, 1, ..: stop if k + 1 == L; if bit k of t is set,
    v_{k+1} = (pend[k+1] + v_k) / 2 completes level k + 1, go on; otherwise pend[k+1] = v_k, stop.
A level-k block is the mean of 2^k consecutive samples of one chain, aligned to the first sample;
the top level L - 1 receives blocks of 2^(L-1) samples for ever.  Each completing level adds
n += B, S[i] += sum_b v_i, Q[i][j] += sum_b v_i v_j (i <= j).  All in float64, nothing clamped.

State (float64, on the device of the first sample): ``acc`` = [t, shift[K], then per level
[n, S[K], Q upper triangle row-major]], ``pend`` [L, K, B].  Device tensors go to
aiqmc_blocking_update on the current stream; other tensors take the same recurrence in torch.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import constants

MAX_SERIES = 8    # AIQMC_BLOCKING_MAX_SERIES
MAX_LEVELS = 32   # AIQMC_BLOCKING_MAX_LEVELS


def _qindex(i: int, j: int, K: int) -> int:
    """Position of Q[i][j], i <= j, in the row-major upper triangle."""
    i, j = (i, j) if i <= j else (j, i)
    return i * K - i * (i - 1) // 2 + (j - i)


class BlockingAccumulator:
    """See ``make_blocking``."""

    def __init__(self, nseries: int = 1, max_levels: int = 24, shift=None, names: Optional[Sequence[str]] = None):
        self.K, self.L = int(nseries), int(max_levels)
        if not 1 <= self.K <= MAX_SERIES:
            raise ValueError(f"make_blocking: nseries must be in 1..{MAX_SERIES}, got {nseries}")
        if not 1 <= self.L <= MAX_LEVELS:
            raise ValueError(f"make_blocking: max_levels must be in 1..{MAX_LEVELS}, got {max_levels}")
        self.M = 1 + self.K + self.K * (self.K + 1) // 2
        sh = np.zeros(self.K) if shift is None else np.asarray(shift, dtype=np.float64).reshape(-1)
        if sh.size == 1 and self.K > 1:
            sh = np.repeat(sh, self.K)
        if sh.size != self.K:
            raise ValueError(f"make_blocking: shift must have one entry per series ({self.K}), got {sh.size}")
        self.shift = torch.tensor(sh, dtype=torch.float64)
        self.names = None if names is None else tuple(str(n) for n in names)
        if self.names is not None and (len(self.names) != self.K or len(set(self.names)) != self.K):
            raise ValueError(f"make_blocking: names must be {self.K} distinct strings")
        iu = np.triu_indices(self.K)
        self._qi, self._qj = torch.tensor(iu[0]), torch.tensor(iu[1])
        self.B = None
        self.acc = self.pend = self._scratch = None

    # -- state ---------------------------------------------------------------------------------
    def _allocate(self, B: int, device) -> None:
        self.B = int(B)
        self.acc = torch.zeros(1 + self.K + self.L * self.M, dtype=torch.float64, device=device)
        self.acc[1:1 + self.K] = self.shift.to(device)
        self.pend = torch.zeros(self.L, self.K, self.B, dtype=torch.float64, device=device)
        self._scratch = None

    def _need(self) -> None:
        if self.acc is None:
            raise RuntimeError("blocking accumulator is empty: call update() (or load_state_dict) first")

    def reset(self) -> None:
        """Forgets every sample; the shift and the shape stay."""
        if self.acc is not None:
            self.acc.zero_()
            self.acc[1:1 + self.K] = self.shift.to(self.acc.device)
            self.pend.zero_()

    @property
    def count(self) -> int:
        """Samples taken so far (synchronises with the device)."""
        return 0 if self.acc is None else int(self.acc[0])

    def state_dict(self) -> dict:
        """Plain host tensors plus the configuration, safe to checkpoint; a run resumed from it
        continues bit for bit."""
        self._need()
        return {"acc": self.acc.detach().cpu().clone(), "pend": self.pend.detach().cpu().clone(),
                "nseries": self.K, "max_levels": self.L, "names": None if self.names is None else list(self.names)}

    def load_state_dict(self, d: dict) -> None:
        """Restores the sums, the waiting blocks, t and the shift; nseries and max_levels in `d`
        must be this accumulator's."""
        if int(d["nseries"]) != self.K or int(d["max_levels"]) != self.L:
            raise ValueError(f"load_state_dict: nseries / max_levels ({int(d['nseries'])}, {int(d['max_levels'])}) differ "
                             f"from this accumulator's ({self.K}, {self.L})")
        acc, pend = torch.as_tensor(d["acc"]), torch.as_tensor(d["pend"])
        if (acc.dtype != torch.float64 or pend.dtype != torch.float64 or acc.numel() != 1 + self.K + self.L * self.M
                or pend.dim() != 3 or tuple(pend.shape[:2]) != (self.L, self.K)):
            raise ValueError("load_state_dict: acc / pend are not the float64 tensors of this layout")
        dev = self.acc.device if self.acc is not None else torch.device("cpu")
        self.B = int(pend.shape[2])
        self.acc = acc.reshape(-1).clone().to(dev)
        self.pend = pend.clone().contiguous().to(dev)
        self.shift = self.acc[1:1 + self.K].detach().cpu().clone()
        self._scratch = None

    # -- accumulation ----------------------------------------------------------------------------
    def update(self, values) -> None:
        """One sample: ``values`` [B] (one series) or [K, B], float32 or float64.  No host
        synchronisation on the kernel path."""
        x = values if isinstance(values, torch.Tensor) else torch.as_tensor(np.asarray(values))
        if torch.is_complex(x):
            raise TypeError("blocking: complex values are refused; pass .real and .imag as two series")
        if x.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"blocking: values must be float32 or float64, got {x.dtype}")
        shape = tuple(x.shape)
        if x.dim() == 1:
            x = x[None]
        if x.dim() != 2 or x.shape[0] != self.K or x.shape[1] < 1:
            what = "[B] or [1, B]" if self.K == 1 else f"[{self.K}, B]"
            raise ValueError(f"blocking: values must be {what} with B >= 1, got {shape}")
        if self.acc is None:
            self._allocate(x.shape[1], x.device)
        elif x.shape[1] != self.B:
            raise ValueError(f"blocking: this accumulator holds {self.B} chains, the sample has {x.shape[1]} "
                             "(the same chains, in the same order, at every call)")
        if self.acc.device != x.device:   # e.g. a state restored on the host, continued on the device
            self.acc, self.pend, self._scratch = self.acc.to(x.device), self.pend.to(x.device), None
        if x.is_cuda:
            from . import _lib
            if self._scratch is None:
                n = _lib.blocking_layout(self.B, self.K, self.L)["scratch"]
                self._scratch = torch.zeros(n, dtype=torch.float64, device=x.device)
            _lib.blocking_update(x.detach().contiguous(), self.L, self.acc, self.pend, self._scratch)
        else:
            self._host_update(x.detach())

    def _host_update(self, x: torch.Tensor) -> None:
        """The kernel's recurrence in torch float64 (the sums over the chains in torch's order)."""
        K, L, M = self.K, self.L, self.M
        t = int(self.acc[0])
        v = x.to(torch.float64) - self.acc[1:1 + K, None]
        qi, qj = self._qi.to(x.device), self._qj.to(x.device)
        k = 0
        while True:
            w = self.acc[1 + K + k * M:1 + K + (k + 1) * M]
            w[0] += float(self.B)
            w[1:1 + K] += v.sum(1)
            w[1 + K:] += (v[qi] * v[qj]).sum(1)
            if k + 1 == L:
                break
            if (t >> k) & 1:
                v = (self.pend[k + 1] + v) / 2.0
            else:
                self.pend[k + 1].copy_(v)
                break
            k += 1
        self.acc[0] += 1.0

    def reblock(self, trace) -> "BlockingAccumulator":
        """Feeds a stored trace [T, B] or [T, K, B], one sample per row, and returns self."""
        tr = trace if isinstance(trace, torch.Tensor) else torch.as_tensor(np.asarray(trace))
        if tr.dim() not in (2, 3):
            raise ValueError(f"reblock: the trace must be [T, B] or [T, K, B], got {tuple(tr.shape)}")
        for row in tr:
            self.update(row)
        return self

    def reduce(self) -> None:
        """Pools the chains of all ranks: a SUM all-reduce of the level words (not t, not the shift)
        over the default process group, in place; the identity in a single process.  The ranks must
        have taken the same number of samples: t is exchanged first, and if the ranks disagree
        EVERY rank raises before the second collective.  Afterwards every rank holds the pooled
        sums, so call it once, when the accumulation is over (or ``reset`` after it)."""
        self._need()
        if not constants._active():
            return
        import torch.distributed as dist
        ts = torch.zeros(dist.get_world_size(), dtype=torch.float64, device=self.acc.device)
        ts[dist.get_rank()] = self.acc[0]
        constants.all_reduce_(ts)
        ts = ts.cpu()
        if bool((ts != ts[0]).any()):
            raise RuntimeError(f"blocking.reduce: the ranks hold different sample counts t = {ts.tolist()}")
        constants.all_reduce_(self.acc[1 + self.K:])

    # -- results -----------------------------------------------------------------------------------
    def _series(self, s) -> int:
        if isinstance(s, str):
            if self.names is None or s not in self.names:
                raise KeyError(f"blocking: no series named {s!r}")
            return self.names.index(s)
        s = int(s)
        if not 0 <= s < self.K:
            raise IndexError(f"blocking: series {s} outside 0..{self.K - 1}")
        return s

    def _words(self):
        """(words [levels reached, M], shift [K]) on the host as numpy float64."""
        self._need()
        a = self.acc.detach().cpu().numpy()
        w = a[1 + self.K:].reshape(self.L, self.M)
        return w[w[:, 0] > 0], a[1:1 + self.K]

    def _moments(self, w, i: int, j: int):
        """Per level: the block means of series i and j (without the shift) and their unbiased
        covariance (NaN below two blocks)."""
        n = w[:, 0]
        mi, mj = w[:, 1 + i] / n, w[:, 1 + j] / n
        with np.errstate(divide="ignore", invalid="ignore"):
            cov = (w[:, 1 + self.K + _qindex(i, j, self.K)] / n - mi * mj) * (n / (n - 1.0))
        return mi, mj, np.where(n >= 2, cov, np.nan)

    def covariance(self, level: int) -> torch.Tensor:
        """The unbiased covariance matrix [K, K] of the level's block means."""
        w, _ = self._words()
        if not 0 <= int(level) < len(w):
            raise IndexError(f"blocking: level {level} has no block yet ({len(w)} levels reached)")
        c = np.empty((self.K, self.K))
        for i in range(self.K):
            for j in range(i, self.K):
                c[i, j] = c[j, i] = self._moments(w[int(level):int(level) + 1], i, j)[2][0]
        return torch.tensor(c)

    def result(self, series=0) -> dict:
        """The blocking analysis of one series (index or name).  Per level reached (float64 host
        tensors): ``block_size`` 2^k, ``n_blocks`` (over all chains), ``mean`` = S / n + shift,
        ``stderr`` = sqrt(var_k / n_k) with var_k = (Q / n - (S / n)^2) n / (n - 1) (a negative
        rounding residue counts as 0; NaN below two blocks), ``stderr_err`` = stderr / sqrt(2 (n_k - 1)).
        Overall: ``naive_stderr`` (level 0), ``optimal_level``: the smallest k with n_k >= 2 and
        2^(3k) > 2 n_0 (stderr_k / stderr_0)^4 (the rule of Wolff and of Lee et al. that pyblock
        uses), None with ``converged`` False when no level qualifies; ``stderr_opt`` and
        ``inefficiency`` = (stderr_opt / stderr_0)^2 = 2 tau_int (NaN when not converged)."""
        s = self._series(series)
        w, shift = self._words()
        n = w[:, 0]
        m, _, var = self._moments(w, s, s)
        var = np.where(var < 0.0, 0.0, var)
        with np.errstate(divide="ignore", invalid="ignore"):
            err = np.sqrt(var / n)
            err_err = err / np.sqrt(2.0 * (n - 1.0))
            crit = 2.0 * n[0] * (err / err[0]) ** 4
        size = 2.0 ** np.arange(len(n))
        ok = np.nonzero((n >= 2) & (size ** 3 > crit))[0]
        opt = int(ok[0]) if ok.size else None
        e_opt = float(err[opt]) if opt is not None else float("nan")
        with np.errstate(divide="ignore", invalid="ignore"):
            ineff = float(np.float64(e_opt) / err[0]) ** 2
        return {"block_size": torch.tensor(size), "n_blocks": torch.tensor(n), "mean": torch.tensor(m + shift[s]),
                "stderr": torch.tensor(err), "stderr_err": torch.tensor(err_err), "naive_stderr": float(err[0]),
                "optimal_level": opt, "converged": opt is not None, "stderr_opt": e_opt, "inefficiency": ineff}

    def ratio(self, i=0, j=1) -> dict:
        """R = mean_i / mean_j per level with its delta-method error
        sqrt((var_i - 2 R cov_ij + R^2 var_j) / n_k) / |mean_j|: the DMC mixed estimator
        sum w E / sum w when fed the series (w E, w).  Keys ``block_size``, ``n_blocks``, ``ratio``, ``stderr``."""
        i, j = self._series(i), self._series(j)
        w, shift = self._words()
        n = w[:, 0]
        mi, mj, cij = self._moments(w, i, j)
        vi, vj = self._moments(w, i, i)[2], self._moments(w, j, j)[2]
        mi, mj = mi + shift[i], mj + shift[j]
        with np.errstate(divide="ignore", invalid="ignore"):
            R = mi / mj
            q = vi - 2.0 * R * cij + R * R * vj
            err = np.sqrt(np.where(q < 0.0, 0.0, q) / n) / np.abs(mj)
        return {"block_size": torch.tensor(2.0 ** np.arange(len(n))), "n_blocks": torch.tensor(n),
                "ratio": torch.tensor(R), "stderr": torch.tensor(err)}


def make_blocking(nseries: int = 1, max_levels: int = 24, shift=None,
                  names: Optional[Sequence[str]] = None) -> BlockingAccumulator:
    """An online Flyvbjerg-Petersen blocking accumulator for ``nseries`` (at most 8) series over a
    fixed set of Markov chains; see the module docstring.

    ``max_levels``  levels kept (at most 32); blocks of the top level hold 2^(max_levels - 1) samples
    ``shift``       subtracted from every sample before it is squared (a scalar, or one per series):
                    a rough guess of the mean keeps sum v^2 well conditioned; results include it again
    ``names``       optional labels, accepted wherever a series index is

    ``update(values)`` takes one sample per call, ``reduce()`` pools the ranks, ``result(series)``,
    ``ratio(i, j)`` and ``covariance(level)`` read the state out, ``state_dict()`` /
    ``load_state_dict()`` checkpoint it, ``reset()`` clears it, ``reblock(trace)`` feeds a stored trace."""
    return BlockingAccumulator(nseries, max_levels, shift, names)


def reblock(trace, max_levels: int = 24, shift=None, names: Optional[Sequence[str]] = None) -> BlockingAccumulator:
    """The accumulator of a stored trace [T, B] or [T, K, B] (``make_blocking(...).reblock(trace)``)."""
    tr = trace if isinstance(trace, torch.Tensor) else torch.as_tensor(np.asarray(trace))
    return make_blocking(tr.shape[1] if tr.dim() == 3 else 1, max_levels, shift, names).reblock(tr)
