"""The density replica and its seeded walkers: the reference that tests/test_density_host.py (the
torch host path) and tests/test_gpu_density.py (the device kernels) share.  A plain module, as
support.py; the other shared references are in replicas_estimators.py and replicas_loss.py.

The replica uses nothing from the package: f = (x - lo) * n / (hi - lo) in float64 (distances:
f = r * n / r_max), inside iff 0 <= f < n, bin floor(f), everything else in the channel's outside
word; a walker of weight w adds rint(w 2^32) per sample.  It also counts the EDGE samples,
|f - rint(f)| <= tol, whose bin a float32 (or float64) evaluation of the same rule may place
differently: tol = 1e-4 for float32 inputs, 1e-10 for float64.
"""
import numpy as np
import torch

ONE = 1 << 32
TOL = {torch.float32: 1e-4, torch.float64: 1e-10}
FIELDS = ("total", "skipped", "grid", "grid_out", "radial", "radial_out", "pair", "pair_out")

# name -> (atoms [A, 3], electrons per atom); alternating spins, slot 0 up, unless the name carries
# its spins after "@", one u / d per slot (oracle/system.py)
SYSTEMS = {
    "H2": ([[0.0, 0.0, -0.7], [0.0, 0.0, 0.7]], [1, 1]),
    "Be": ([[0.0, 0.0, 0.0]], [4]),
    "Z5": ([[0.0, 0.0, 0.0]], [5]),                      # odd N, nspins (3, 2)
    "N2": ([[0.0, 0.0, -1.0372], [0.0, 0.0, 1.0372]], [7, 7]),
    "Z5@duddd": ([[0.0, 0.0, 0.0]], [5]),                # spin-polarised, minority first: nspins (1, 4)
}
GRID = ((-2.5, -3.0, -3.5), (2.5, 3.0, 3.5), (6, 9, 16))
RADIAL = (4.0, 16)
PAIR = (5.0, 12)
# the first seeds without an edge sample at tol 1e-4 (the walkers do not depend on the spins)
SEEDS = {"H2": 2, "Be": 3, "Z5": 3, "N2": 14, "Z5@duddd": 3}
BMAX = 70


def geometry(name):
    atoms, per = SYSTEMS[name]
    atoms = np.asarray(atoms, dtype=np.float64)
    n = int(sum(per))
    pattern = name.partition("@")[2]
    assert len(pattern) in (0, n)
    spins = np.array([1.0 if (ch == "u" if pattern else i % 2 == 0) else -1.0 for i, ch in enumerate(pattern or "u" * n)])
    return atoms, per, spins


def walkers(name, B=BMAX, seed=None):
    """[B, 3N] float64 that are exactly representable in float32: electrons at their atoms plus a
    unit normal, so that some fall outside every range used here."""
    atoms, per, _ = geometry(name)
    rng = np.random.default_rng(SEEDS[name] if seed is None else seed)
    block = np.concatenate([np.tile(atoms[i], per[i]) for i in range(len(per))])
    pos = block[None] + rng.standard_normal((B, block.size))
    return pos.astype(np.float32).astype(np.float64)


def replica(pos, atoms, spins, grid=None, radial=None, pair=None, weights=None, tol=1e-10):
    """({name: int64 array}, number of edge samples) for walkers pos [B, 3N] in float64."""
    pos = np.asarray(pos, dtype=np.float64)
    B, N, A = pos.shape[0], pos.shape[1] // 3, len(atoms)
    x = pos.reshape(B, N, 3)
    chan = np.where(np.asarray(spins) > 0, 0, 1)
    if weights is None:
        q = np.full(B, ONE, dtype=np.int64)
        ok = np.ones(B, dtype=bool)
    else:
        w = np.asarray(weights, dtype=np.float64)
        ok = np.isfinite(w) & (w >= 0)
        q = np.where(ok, np.rint(np.where(ok, w, 0.0) * 4294967296.0), 0.0).astype(np.int64)
    out = {"total": np.array([q.sum()], dtype=np.int64), "skipped": np.array([(~ok).sum()], dtype=np.int64)}
    edges = 0

    def rule(f, n):
        nonlocal edges
        with np.errstate(invalid="ignore"):
            edges += int((np.abs(f - np.rint(f)) <= tol).sum())
            inside = (f >= 0) & (f < n)
        return inside, np.floor(np.where(inside, f, 0.0)).astype(np.int64)

    with np.errstate(invalid="ignore", over="ignore"):
        if grid is not None and all(n > 0 for n in grid[2]):
            lo, hi, n = grid
            g = np.zeros((2,) + tuple(n), dtype=np.int64)
            go = np.zeros(2, dtype=np.int64)
            ins, bins = np.ones((B, N), dtype=bool), []
            for d in range(3):
                i_d, b_d = rule((x[..., d] - lo[d]) * (n[d] / (hi[d] - lo[d])), n[d])
                ins &= i_d
                bins.append(b_d)
            for b in range(B):
                for e in range(N):
                    if ins[b, e]:
                        g[chan[e], bins[0][b, e], bins[1][b, e], bins[2][b, e]] += q[b]
                    else:
                        go[chan[e]] += q[b]
            out["grid"], out["grid_out"] = g, go
        if radial is not None and radial[1] > 0:
            rmax, n = radial
            r = np.sqrt(((x[:, :, None, :] - np.asarray(atoms)[None, None]) ** 2).sum(-1))
            ins, bn = rule(r * (n / rmax), n)
            h, ho = np.zeros((2, A, n), dtype=np.int64), np.zeros((2, A), dtype=np.int64)
            for b in range(B):
                for e in range(N):
                    for a in range(A):
                        if ins[b, e, a]:
                            h[chan[e], a, bn[b, e, a]] += q[b]
                        else:
                            ho[chan[e], a] += q[b]
            out["radial"], out["radial_out"] = h, ho
        if pair is not None and pair[1] > 0:
            rmax, n = pair
            h, ho = np.zeros((3, n), dtype=np.int64), np.zeros(3, dtype=np.int64)
            for i in range(N):
                for j in range(i + 1, N):
                    ch = chan[i] if chan[i] == chan[j] else 2
                    r = np.sqrt(((x[:, i] - x[:, j]) ** 2).sum(-1))
                    ins, bn = rule(r * (n / rmax), n)
                    for b in range(B):
                        if ins[b]:
                            h[ch, bn[b]] += q[b]
                        else:
                            ho[ch] += q[b]
            out["pair"], out["pair_out"] = h, ho
    return out, edges


def assert_counts_equal(counts, ref):
    """Every word of the accumulator's named views equals the replica's; absent families are empty."""
    for k in FIELDS:
        got = counts[k].detach().cpu().numpy()
        if k in ref:
            assert got.shape == ref[k].shape, (k, got.shape, ref[k].shape)
            np.testing.assert_array_equal(got, ref[k], err_msg=k)
        else:
            assert got.size == 0, k
