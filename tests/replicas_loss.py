"""Inputs and checkers that the HIP reduction kernels' tests (tests/test_gpu_reductions.py) share
with their CPU counterparts: the multi-rank loss levels (tests/test_loss_levels_host.py holds
aiqmc.Loss.loss._host_level to the same assertions) and the stochastic comb's inputs
(tests/test_dmc.py checks them on the CPU).  A plain module, as support.py.

References are numpy float64 (np.longdouble where a sum is the subject) on the inputs rounded to the
kernel's dtype; none is derived from a kernel's output."""
import functools

import numpy as np
import torch

NP_DT = {torch.float32: np.float32, torch.float64: np.float64}
DTYPES = [torch.float32, torch.float64]
DT_IDS = ["f32", "f64"]

# ----------------------------------------------------------------------------- stochastic comb

COMB_N = [1, 2, 63, 1023, 1024, 1025, 2047, 3001, 4096, 4097, 5000, 9001]
TIE_N = [1024, 2048, 4096, 8192]


def _comb_weights(n, dtype):
    """uniform [0.5, 1.5) with about 10 % zeros (n <= 2: all 1.25), rounded to the context dtype."""
    if n <= 2:
        w = np.full(n, 1.25)
    else:
        rng = np.random.default_rng(100 + n)
        w = rng.uniform(0.5, 1.5, n)
        w[rng.uniform(size=n) < 0.1] = 0.0
    return w.astype(NP_DT[dtype]).astype(np.float64)


def _comb_targets(w, u):
    """branch.py:21-27 as oracle.dmc.branch forms them: (cumsum, targets)."""
    n = w.shape[0]
    cs = np.cumsum(w)
    wtot = cs[-1]
    return cs, (u * wtot + np.linspace(0, wtot, n, endpoint=False)) % wtot


def _comb_gap(w, u):
    """The least distance from a comb target to a cumulative-sum value, over wtot (reference
    only).  n <= 2 with u = 0 is left out: the weights 1.25, their sums and the targets 0 and 1.25
    are binary fractions, every operation of either side is exact, and the target ON cumsum[0] is
    an exact tie, well-posed like those of test_comb_exact_ties."""
    if w.size <= 2 and u == 0.0:
        return 1.0
    cs, tt = _comb_targets(w, u)
    k = np.searchsorted(cs, tt)
    above = np.abs(cs[np.minimum(k, len(cs) - 1)] - tt)
    below = np.where(k > 0, np.abs(tt - cs[np.maximum(k - 1, 0)]), np.inf)
    return float(np.minimum(above, below).min() / cs[-1])


def _tie_weights(n):
    """Integer weights 0..3, the last adjusted so that the sum is exactly 2 n: with u in {0, 0.5,
    0.75} every cumulative sum and every target is an integer, exact in float64 (and float32)."""
    w = np.random.default_rng(n).integers(0, 4, n).astype(np.int64)
    w[-1] += 2 * n - w.sum()
    assert w[-1] > 0 and w.sum() == 2 * n
    return w


def _tie_targets_int(n, u):
    off = {0.0: 0, 0.5: n, 0.75: 3 * n // 2}[u]        # u wtot, wtot = 2 n
    return [(off + 2 * j) % (2 * n) for j in range(n)]


# ----------------------------------------------------------------------------- multi-rank loss levels

LOSS_B = 3001
SPLITS = {"1rank": [3001], "halves": [1500, 1501], "1+3000": [1, 3000], "3ranks": [1025, 7, 1969]}
CLIPS = [(5.0, True), (5.0, False), (0.0, True)]


@functools.lru_cache(maxsize=None)
def _loss_energies(dtype, cplx, n=LOSS_B):
    """The heavy-tailed energies of test_gpu_api.py::test_fused_loss_weights_match_torch_path
    (outliers so that the window bites), a few imaginary parts exactly 0 and -0, rounded to
    dtype: (re, im or None) float64 arrays."""
    g = torch.Generator().manual_seed(11)
    re = torch.randn(LOSS_B, generator=g, dtype=torch.float64) * 2 - 10
    re[::97] *= 40.0
    im = torch.randn(LOSS_B, generator=g, dtype=torch.float64) * 0.3
    im[::53] *= 30.0
    im[[3, 1500, 2999]] = 0.0
    im[[4, 1501]] = -0.0
    rnd = lambda t: t.numpy()[:n].astype(NP_DT[dtype]).astype(np.float64)
    return rnd(re), (rnd(im) if cplx else None)


def _ld_mean(v):
    return float(np.sum(v.astype(np.longdouble)) / np.longdouble(v.size))


def _loss_reference(x, y, clip, center, wscale):
    """The header comment of k_lossr_* (Loss/loss.py:73-135, :206-208, :256-265) on the pooled
    batch: E = mean e, var = mean |e - E|^2, the TV window about E per component, xc = the
    clamped energies, dc = mean xc (centred at the clipped mean) or E; level weights
    w = wscale (Re xc - Re E), wp = wscale Im xc (clipping) or wscale (2 Im e - Im E)."""
    cplx = y is not None
    yy = y if cplx else np.zeros_like(x)
    mr, mi = _ld_mean(x), _ld_mean(yy)
    var = _ld_mean((x - mr) ** 2 + (yy - mi) ** 2)
    if clip > 0:
        tvr, tvi = _ld_mean(np.abs(x - mr)), _ld_mean(np.abs(yy - mi))
        xc = np.clip(x, mr - clip * tvr, mr + clip * tvr)
        yc = np.clip(yy, mi - clip * tvi, mi + clip * tvi)
        wp = wscale * yc
    else:
        xc, yc = x, yy
        wp = wscale * ((yy - mi) + yy)
    dcr, dci = (_ld_mean(xc), _ld_mean(yc)) if (clip > 0 and center) else (mr, mi)
    return dict(mr=mr, mi=mi, var=var, dcr=dcr, dci=dci, xc=xc, yc=yc, w=wscale * (xc - mr), wp=wp,
                nz=float(np.count_nonzero(yy)))


def _run_levels(level, x, y, sizes, clip, center, wscale, dtype, device):
    """R simulated ranks: level 1 per piece, the vectors added in torch (the all-reduce), the
    same for level 2 and the heads of level 3.  Returns the summed vectors and per-rank outputs."""
    cplx = y is not None
    g0 = clip > 0 and center
    offs = np.cumsum([0] + list(sizes))
    t = lambda a, r: torch.tensor(a[offs[r]:offs[r + 1]], dtype=dtype, device=device).contiguous()
    er = [t(x, r) for r in range(len(sizes))]
    ei = [t(y, r) if cplx else None for r in range(len(sizes))]
    L1 = sum(level(1, a, b) for a, b in zip(er, ei))
    L2 = sum(level(2, a, b, L1) for a, b in zip(er, ei)) if clip > 0 else None
    ranks = [level(3, a, b, L1, L2, clip, wscale, g0, cplx) for a, b in zip(er, ei)]
    return L1, L2, ranks, offs


def _check_levels(L1, ranks, ref, cplx, g0, wscale, dtype, n):
    """Level statistics, weights and clipped energies against the reference; returns the stats
    [Re E, Im E, variance, Re dc, Im dc] formed from the summed vectors as the kernel's header
    states them (checked against k_lossr_final's own where that runs)."""
    tol = dict(rtol=1e-11, atol=1e-11) if dtype == torch.float64 else dict(rtol=2e-6, atol=2e-6)
    l1 = L1.cpu().numpy()
    assert l1[4] == n and l1[5] == ref["nz"]
    np.testing.assert_allclose(l1[1] / n, ref["mr"], rtol=1e-12)
    np.testing.assert_allclose(l1[2] / n, ref["mi"], rtol=1e-12)
    cat = lambda k: torch.cat([r[k].reshape(-1) if k else r[0][0] for r in ranks]).cpu().double().numpy()
    np.testing.assert_allclose(cat(0), ref["w"], **tol)
    if g0:
        w1 = torch.cat([r[0][1] for r in ranks]).cpu().double().numpy()
        np.testing.assert_array_equal(w1, np.full(n, NP_DT[dtype](wscale), dtype=np.float64))
    else:
        assert all(r[0].shape[0] == 1 for r in ranks)
    np.testing.assert_allclose(cat(2), ref["xc"], **tol)
    if cplx:
        np.testing.assert_allclose(cat(1), ref["wp"], **tol)
        np.testing.assert_allclose(cat(3), ref["yc"], **tol)
    else:
        assert all(r[1] is None and r[3] is None for r in ranks)
    head = sum(r[4] for r in ranks).cpu().numpy()
    np.testing.assert_allclose(head[0] / n, _ld_mean(ref["xc"]), rtol=1e-12)
    if cplx:
        np.testing.assert_allclose(head[1] / n, _ld_mean(ref["yc"]), rtol=1e-12)
    return head


def _assert_stats(st, ref, cplx):
    print("  stats", st[:6].tolist(), "reference", [ref[k] for k in ("mr", "mi", "var", "dcr", "dci", "nz")])
    np.testing.assert_allclose(st[0], ref["mr"], rtol=1e-12)
    np.testing.assert_allclose(st[2], ref["var"], rtol=1e-12)
    np.testing.assert_allclose(st[3], ref["dcr"], rtol=1e-12)
    if cplx:
        np.testing.assert_allclose(st[1], ref["mi"], rtol=1e-12)
        np.testing.assert_allclose(st[4], ref["dci"], rtol=1e-12)
    else:
        assert st[1] == 0.0 and st[4] == 0.0


def _edge_cases(dtype):
    """(name, re, im, rank sizes): one energy; one block of 1024 and one more; all equal."""
    x, y = _loss_energies(dtype, True)
    return [("n=1", x[:1], None, [1]), ("n=1 complex", x[:1], y[:1], [1]),
            ("n=1024", x[:1024], y[:1024], [1024]), ("n=1025", x[:1025], y[:1025], [1025]),
            ("n=1025 two ranks", x[:1025], y[:1025], [1024, 1]),
            ("equal", np.full(2000, -10.5), np.full(2000, 0.25), [2000]),
            ("equal three ranks", np.full(3001, -10.5), None, [1025, 7, 1969])]


def _check_edges(level, final, dtype, device):
    """final(L1, head, g0, center, n_ranks) -> [Re E, Im E, variance, Re dc, Im dc] from the summed vectors."""
    wscale = 0.125
    for name, x, y, sizes in _edge_cases(dtype):
        for clip, center in CLIPS:
            n, cplx, g0 = x.size, y is not None, clip > 0 and center
            ref = _loss_reference(x, y, clip, center, wscale)
            L1, L2, ranks, _ = _run_levels(level, x, y, sizes, clip, center, wscale, dtype, device)
            print(name, clip, center)
            _check_levels(L1, ranks, ref, cplx, g0, wscale, dtype, n)
            head = sum(r[4] for r in ranks)
            st = final(L1, head, g0, center and clip > 0, len(sizes))
            _assert_stats(st, ref, cplx)
            if name.startswith("n=1 ") or name == "n=1" or name.startswith("equal"):
                # one energy, or -10.5 / 0.25 whose sums are exact: variance 0, a zero-width window,
                # the clipped energies the energies themselves and every energy-gradient weight 0,
                # to the bit
                assert float(L1[0]) == 0.0 and st[2] == 0.0
                assert st[0] == x[0] and st[3] == x[0]
                assert all(bool((r[0][0] == 0).all()) for r in ranks)
                assert float(head[0]) == np.sum(x)
                assert all(bool((r[2].cpu().double() == x[0]).all()) for r in ranks)
                if clip > 0:
                    assert L2.cpu().tolist() == [0.0, 0.0]
                if cplx:   # wscale Im xc (clipping) and wscale (2 Im e - Im E) (without) are both wscale Im e
                    assert all(bool((r[1].cpu().double() == wscale * y[0]).all()) for r in ranks)
