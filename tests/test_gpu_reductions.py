"""The small fixed-order reduction kernels of csrc/dmc.hip and csrc/loss.hip (their block
reductions: csrc/reduce.h) against plain float64 references.

1. k_dmc_branch (stochastic comb, DMC/branch.py:10-33) against oracle.dmc.branch in its three
   regimes -- one weight per thread (n <= 1024), the blocked scan held in LDS (n <= 4096) and the
   cumulative sum through the global buffer (n > 4096) -- for float32 and float64 weights, zero
   weights and exact ties: indices exactly equal.
2. k_dmc_cut_part / k_dmc_cut_fin / k_dmc_weights (DMC/S_matrix.py:4-24, dmc.py:88-92) against
   oracle.dmc.comput_S / update_weights: batches below one block, at and past one grid-stride
   pass, per-walker e_trial / e_est (the first DMC block), the cut_minima= (multi-device) argument.
3. k_lossr_l1/_l2/_l3/_pack/_final (aiqmc_loss_level / _pack / _final) driven directly, with R
   ranks simulated on one device (the rank vectors added in torch, as the all-reduce does) and
   unequal splits, against a numpy restatement of the formulas in the kernels' header comment.
   aiqmc.Loss.loss._host_level (the gloo ranks' torch restatement) runs through the same
   assertions on the CPU (tests/test_loss_levels_host.py), so both paths are held to one
   reference; the comb inputs' CPU checks are in tests/test_dmc.py.

References are numpy float64 (np.longdouble where a sum is the subject) on the inputs rounded
to the kernel's dtype; none is derived from a kernel's output.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import dmc as odmc
from replicas_loss import (CLIPS, COMB_N, DT_IDS, DTYPES, LOSS_B, NP_DT, SPLITS, TIE_N, _assert_stats, _check_edges,
                           _check_levels, _comb_gap, _comb_weights, _ld_mean, _loss_energies,
                           _loss_reference, _run_levels, _tie_targets_int, _tie_weights)

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def _be_ctx(dtype):
    from oracle import system
    from aiqmc import _lib
    s = system.make_system("Be")
    ctx = _lib.Context.for_system(s, dtype)
    return s, ctx


# ----------------------------------------------------------------------------- 1. stochastic comb

@pytest.mark.parametrize("u", [0.0, 0.37, 0.999999])
@pytest.mark.parametrize("n", COMB_N)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_comb_matches_oracle(dtype, n, u):
    """Indices exactly equal to oracle.dmc.branch's; the new weight to 1e-13 (fp64: both sides are
    fp64 sums of at most 9001 terms) or one float32 rounding (fp32: the fp64 quotient rounded
    once); the same bits when run twice."""
    _, ctx = _be_ctx(dtype)
    w = _comb_weights(n, dtype)
    assert _comb_gap(w, u) >= 1e-10
    wn_r, idx_r = odmc.branch(w, u)
    wt = torch.tensor(w, dtype=dtype, device="cuda")
    wn, idx = ctx.dmc_branch(wt, u)
    wn2, idx2 = ctx.dmc_branch(wt, u)
    torch.cuda.synchronize()
    got = idx.cpu().numpy()
    print(n, u, "mismatches", int((got != idx_r).sum()), "weight", wn.item(), "oracle", wn_r)
    np.testing.assert_array_equal(got, idx_r)
    assert abs(float(wn.item()) - wn_r) <= (1e-13 if dtype == torch.float64 else EPS32) * abs(wn_r)
    assert torch.equal(idx, idx2) and torch.equal(wn, wn2)


@pytest.mark.parametrize("u", [0.0, 0.5, 0.75])
@pytest.mark.parametrize("n", TIE_N)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_comb_exact_ties(dtype, n, u):
    """Integer weights summing to 2 n: every operation of the kernel is exact, hundreds of targets
    land ON a cumulative-sum value, and the kernel must take the left one (cp[mid] < target)."""
    _, ctx = _be_ctx(dtype)
    w = _tie_weights(n)
    cs = np.cumsum(w).astype(np.float64)
    tt = np.array(_tie_targets_int(n, u), dtype=np.float64)
    want = np.searchsorted(cs, tt, side="left")
    assert int(np.isin(tt, cs).sum()) >= n // 8
    wn, idx = ctx.dmc_branch(torch.tensor(w, dtype=dtype, device="cuda"), u)
    torch.cuda.synchronize()
    got = idx.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert np.all(w[got] != 0)                            # a zero-weight walker is never selected
    assert wn.item() == 2.0


# ----------------------------------------------------------------------------- 2. DMC weights / cut minima

DMC_B = [1, 2, 255, 256, 257, 300, 16384, 16385]   # 16384 = 256 DMC_NB: one full grid-stride pass
TAU, TDAMP, BRANCHCUT, E_TRIAL = 0.01, 0.97, 0.3, -14.5


def _dmc_inputs(B, dtype, kind, seed=4):
    """Inputs rounded to the context dtype (float64 arrays).  kind: 'cut' -- the energies of
    test_dmc.py (some within the branch cut of e_est); 'far' -- every energy farther than the
    branch cut from e_est (scalar and per-walker), so the cut is the branch cut itself; 'zero' --
    one walker with eloc == e_est exactly (sign 0, cut 0)."""
    rnd = lambda a: np.asarray(a).astype(NP_DT[dtype]).astype(np.float64)
    rng = np.random.default_rng(seed + B)
    N = 4
    d = dict(go=rnd(rng.standard_normal((B, 3 * N))), gn=rnd(rng.standard_normal((B, 3 * N))),
             w0=rnd(rng.uniform(0.5, 1.5, B)))
    eo, en = rng.normal(-14.6, 0.4, B), rng.normal(-14.6, 0.4, B)
    d["e_est"] = -14.625 if kind == "zero" else -14.62      # -14.625 is a float32 number
    d["e_est_b"] = rnd(d["e_est"] + rng.normal(0.0, 0.2, B))
    d["e_trial_b"] = rnd(E_TRIAL + rng.normal(0.0, 0.2, B))
    if kind == "far":
        so, sn = rng.choice([-1.0, 1.0], B), rng.choice([-1.0, 1.0], B)
        do, dn = BRANCHCUT + 0.05 + rng.uniform(0, 1, B), BRANCHCUT + 0.05 + rng.uniform(0, 1, B)
        d["scalar"] = (rnd(d["e_est"] + so * do), rnd(d["e_est"] + sn * dn))
        d["walker"] = (rnd(d["e_est_b"] + so * do), rnd(d["e_est_b"] + sn * dn))
    else:
        eo, en = rnd(eo), rnd(en)
        eob, enb = eo.copy(), en.copy()
        if kind == "zero":
            ko, kn = B // 3, (2 * B) // 3
            eo[ko] = en[kn] = d["e_est"]
            eob[ko], enb[kn] = d["e_est_b"][ko], d["e_est_b"][kn]
        d["scalar"], d["walker"] = (eo, en), (eob, enb)
    return d


def _ref_minima(eo, en, e_est):
    return np.array([min(np.abs(e_est - eo).min(), BRANCHCUT), min(np.abs(e_est - en).min(), BRANCHCUT)])


def _ref_weights(d, eo, en, e_trial, e_est):
    S_old = odmc.comput_S(e_trial, e_est, BRANCHCUT, d["go"] ** 2, TAU, eo, 4)
    S_new = odmc.comput_S(e_trial, e_est, BRANCHCUT, d["gn"] ** 2, TAU, en, 4)
    return odmc.update_weights(d["w0"], TAU, TDAMP, S_new, S_old)


def _assert_weights(w, ref, dtype):
    """fp64: rtol 1e-12 (the project's figure); fp32: the kernel computes in double from the
    float32 inputs and rounds once -- one float32 rounding of the oracle on the same inputs."""
    got = w.cpu().double().numpy()
    print("  max rel err", float(np.max(np.abs(got - ref) / np.abs(ref))))
    np.testing.assert_allclose(got, ref, rtol=1e-12 if dtype == torch.float64 else EPS32, atol=0)


@pytest.mark.parametrize("kind", ["cut", "far", "zero"])
@pytest.mark.parametrize("B", DMC_B)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_dmc_weights_and_cut_minima(dtype, B, kind):
    _, ctx = _be_ctx(dtype)
    d = _dmc_inputs(B, dtype, kind)
    dev = lambda a: torch.tensor(a, dtype=dtype, device="cuda")
    tdamp = torch.tensor([0.0, 0.0, TDAMP], dtype=torch.float64, device="cuda")
    go, gn = dev(d["go"]), dev(d["gn"])
    for form in ("scalar", "walker"):
        eo, en = d[form]
        per_walker = form == "walker"
        e_est = d["e_est_b"] if per_walker else d["e_est"]
        e_trial = d["e_trial_b"] if per_walker else E_TRIAL
        a_est = dev(e_est) if per_walker else e_est
        a_trial = dev(e_trial) if per_walker else e_trial
        # a minimum has no rounding: exact on the dtype-rounded inputs
        cm = ctx.dmc_cut_minima(dev(eo), dev(en), a_est, BRANCHCUT)
        ref_cm = _ref_minima(eo, en, e_est)
        print(B, kind, form, "minima", cm.tolist(), "reference", ref_cm.tolist())
        np.testing.assert_array_equal(cm.cpu().numpy(), ref_cm)
        if kind == "far":
            assert ref_cm.tolist() == [BRANCHCUT, BRANCHCUT]
        if kind == "zero":
            assert ref_cm.tolist() == [0.0, 0.0]
        w_int, w_cm = dev(d["w0"]), dev(d["w0"])
        ctx.dmc_weights(w_int, dev(eo), dev(en), go, gn, tdamp, TAU, a_trial, a_est, BRANCHCUT)
        ctx.dmc_weights(w_cm, dev(eo), dev(en), go, gn, tdamp, TAU, a_trial, a_est, BRANCHCUT, cut_minima=cm)
        torch.cuda.synchronize()
        assert torch.equal(w_int, w_cm)                  # internal minima == cut_minima=, bitwise
        _assert_weights(w_int, _ref_weights(d, eo, en, e_trial, e_est), dtype)
        if kind == "zero":
            # sign(0) = 0 with a cut that is not 0 (another device's minima): that walker's e_cut is 0
            cuts = np.array([0.2, 0.1])
            w_s = dev(d["w0"])
            ctx.dmc_weights(w_s, dev(eo), dev(en), go, gn, tdamp, TAU, a_trial, a_est, BRANCHCUT,
                            cut_minima=torch.tensor(cuts, device="cuda"))
            S = lambda c, g, el: e_trial - e_est + c * np.sign(e_est - el) / (1 + ((g ** 2).sum(-1) * TAU / 4) ** 2)
            ref = np.exp(TAU * TDAMP * (0.5 * S(cuts[1], d["gn"], en) + 0.5 * S(cuts[0], d["go"], eo))) * d["w0"]
            assert np.sign(e_est - eo)[B // 3] == 0
            _assert_weights(w_s, ref, dtype)


@pytest.mark.parametrize("form", ["scalar", "walker"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_dmc_cut_minima_two_devices(dtype, form):
    """S_matrix.py:21-22 takes ONE minimum over the stacked [ndev, B] arrays: a batch of 600 split
    into 250 + 350, each part's dmc_cut_minima, their elementwise min fed to both dmc_weights
    calls -- bitwise the weights of one call on the whole batch."""
    _, ctx = _be_ctx(dtype)
    B, parts = 600, [slice(0, 250), slice(250, 600)]
    d = _dmc_inputs(B, dtype, "cut")
    dev = lambda a: torch.tensor(a, dtype=dtype, device="cuda")
    tdamp = torch.tensor([0.0, 0.0, TDAMP], dtype=torch.float64, device="cuda")
    eo, en = d[form]
    pw = form == "walker"
    pick = lambda a, sl: dev(a[sl]) if pw else a
    e_est, e_trial = (d["e_est_b"], d["e_trial_b"]) if pw else (d["e_est"], E_TRIAL)
    whole = dev(d["w0"])
    ctx.dmc_weights(whole, dev(eo), dev(en), dev(d["go"]), dev(d["gn"]), tdamp, TAU, pick(e_trial, slice(None)),
                    pick(e_est, slice(None)), BRANCHCUT)
    cms = [ctx.dmc_cut_minima(dev(eo[sl]), dev(en[sl]), pick(e_est, sl), BRANCHCUT) for sl in parts]
    cm = torch.minimum(cms[0], cms[1])
    assert not torch.equal(cms[0], cms[1])                # the parts' minima differ: the min matters
    np.testing.assert_array_equal(cm.cpu().numpy(), _ref_minima(eo, en, e_est))
    out = []
    for sl in parts:
        w = dev(d["w0"][sl])
        ctx.dmc_weights(w, dev(eo[sl]), dev(en[sl]), dev(d["go"][sl]), dev(d["gn"][sl]), tdamp, TAU,
                        pick(e_trial, sl), pick(e_est, sl), BRANCHCUT, cut_minima=cm)
        out.append(w)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(out), whole)
    _assert_weights(whole, _ref_weights(d, eo, en, e_trial, e_est), dtype)


# ----------------------------------------------------------------------------- 3. multi-rank loss levels

P_MAX = 600


@functools.lru_cache(maxsize=None)
def _jacobians():
    rng = np.random.default_rng(23)
    return rng.standard_normal((LOSS_B, P_MAX)), rng.standard_normal((LOSS_B, P_MAX))


@pytest.mark.parametrize("P", [1, 255, 256, 257, 600])
@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("clip,center", CLIPS)
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_loss_levels_simulated_ranks(dtype, cplx, clip, center, split, P):
    """The level kernels on R slices of one batch, the rank vectors added in torch, with synthetic
    gradient sums G = w @ O (+ wp @ Op), G0 = w1 @ O formed in numpy from the weights the kernel
    returned (so loss_pack / loss_final see known numbers): statistics, weights, clipped energies
    and grad = (G - (Re dc - Re E) G0) / world against the numpy reference on the pooled batch."""
    from aiqmc import _lib
    sizes = SPLITS[split]
    R = len(sizes)
    x, y = _loss_energies(dtype, cplx)
    wscale = 2.0 / LOSS_B
    g0 = clip > 0 and center
    ref = _loss_reference(x, y, clip, center, wscale)
    L1, L2, ranks, offs = _run_levels(_lib.loss_level, x, y, sizes, clip, center, wscale, dtype, "cuda")
    _check_levels(L1, ranks, ref, cplx, g0, wscale, dtype, LOSS_B)
    O, Op = (a[:, :P] for a in _jacobians())
    npdt = NP_DT[dtype]
    dev = lambda a: torch.tensor(a, dtype=dtype, device="cuda")
    L3 = None
    Gsum, G0sum = np.zeros(P), np.zeros(P)
    for r, (w, wp, cr, ci, head) in enumerate(ranks):
        Or, Opr = O[offs[r]:offs[r + 1]], Op[offs[r]:offs[r + 1]]
        # the rank's gradient sums in the ctx dtype, as param_grad_weighted returns them
        G = (w[0].cpu().double().numpy() @ Or).astype(npdt)
        Gp = (wp.cpu().double().numpy() @ Opr).astype(npdt) if cplx else None
        G0 = (w[1].cpu().double().numpy() @ Or).astype(npdt) if g0 else None
        Gsum += G.astype(np.float64) + (Gp.astype(np.float64) if cplx else 0.0)
        if g0:
            G0sum += G0.astype(np.float64)
        part = _lib.loss_pack(dev(G), dev(Gp) if cplx else None, dev(G0) if g0 else None, head)
        assert part.numel() == 2 + P * (2 if g0 else 1)
        L3 = part if L3 is None else L3 + part
    grad, stats = _lib.loss_final(L1, L3, P, g0, center and clip > 0, R, dtype)
    torch.cuda.synchronize()
    st = stats.cpu().numpy()
    _assert_stats(st, ref, cplx)
    assert st[5] == ref["nz"]
    want = (Gsum - (ref["dcr"] - ref["mr"]) * G0sum) / R
    got = grad.cpu().double().numpy()
    scale = np.abs(want).max()
    err = np.abs(got - want).max() / scale
    print("  grad max err / max|grad|", err, "max|grad|", scale)
    assert err <= (1e-12 if dtype == torch.float64 else EPS32)
    if dtype == torch.float64:
        # end to end: the reference's own weights wscale Re(xc_b - dc) (loss.py:256-265) and the phase
        # weights, summed over the pooled batch.  Each level weight carries <= ~4 roundings of
        # wscale (|xc| + |E|) <= wscale 1300, i.e. <= 6e-13 wscale; 3001 terms with |O| <= 5 give
        # <= 9e-9 wscale against max|grad| ~ wscale sqrt(B) sigma ~ 100 wscale: 1e-10 relative
        direct = ((wscale * (ref["xc"] - ref["dcr"])) @ O + (ref["wp"] @ Op if cplx else 0.0)) / R
        e2e = np.abs(got - direct).max() / np.abs(direct).max()
        print("  grad vs pooled-batch formula", e2e)
        assert e2e <= 1e-10
    # the levels pool over walkers: the single-launch kernel on the concatenated batch agrees
    e = torch.complex(dev(x), dev(y)) if cplx else dev(x)
    w1, wp1, clipped1, st1 = _lib.loss_weights(e, clip, center, wscale, cplx)
    tol = dict(rtol=1e-11, atol=1e-11) if dtype == torch.float64 else dict(rtol=2e-6, atol=2e-6)
    s1 = st1.cpu().numpy()
    for k in (0, 2, 3) + ((1, 4) if cplx else ()):
        np.testing.assert_allclose(st[k], s1[k], rtol=1e-12)
    w_lvl = torch.cat([r[0][0] for r in ranks]).cpu().double().numpy()
    np.testing.assert_allclose(w_lvl - wscale * (st[3] - st[0]), w1.cpu().double().numpy(), **tol)
    if cplx:
        np.testing.assert_allclose(torch.cat([r[1] for r in ranks]).cpu().double().numpy(),
                                   wp1.cpu().double().numpy(), **tol)
    if R == 1:
        # one rank's between-term is exactly 0 (the fp contract(off) blocks): variance = M2 / n to the bit
        assert torch.equal(stats[2], L1[0] / L1[4])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_energy_stats_final_reproduces_one_rank(dtype):
    """energy_stats(finalize=False) + energy_stats_final on ONE rank's 4-vector against
    finalize=True: the between-term n m^2 - n m^2 is exactly 0, so the variance is M2 / n to the
    bit (the mean, fl(fl(n m) / n), to one rounding of m)."""
    from aiqmc import _lib
    x, _ = _loss_energies(dtype, False)
    e = torch.tensor(x, dtype=dtype, device="cuda")
    one = _lib.energy_stats(e, finalize=True)
    two = _lib.energy_stats_final(_lib.energy_stats(e, finalize=False))
    torch.cuda.synchronize()
    assert torch.equal(one[:4], two[:4])
    assert torch.equal(two[5], one[5]) and torch.equal(one[5], one[0] / one[3])
    assert abs(two[4].item() - one[4].item()) <= 2.0 ** -52 * abs(one[4].item())
    np.testing.assert_allclose(one[4].item(), _ld_mean(x), rtol=1e-12)
    np.testing.assert_allclose(one[5].item(), _ld_mean((x - _ld_mean(x)) ** 2), rtol=1e-12)


def _final_hip(dtype):
    from aiqmc import _lib

    def final(L1, head, g0, center, world):
        one = torch.ones(1, dtype=dtype, device="cuda")
        L3 = _lib.loss_pack(one, None, one if g0 else None, head)
        grad, stats = _lib.loss_final(L1, L3, 1, g0, center, world, dtype)
        return stats.cpu().numpy()
    return final


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_loss_level_edge_batches(dtype):
    """One energy (variance 0, a zero-width window, every weight 0), one workgroup's 1024 and one
    more, all energies equal."""
    from aiqmc import _lib
    _check_edges(_lib.loss_level, _final_hip(dtype), dtype, "cuda")


# ----------------------------------------------------------------------------- 4. block_sum's stated order

STATS_N = [1, 63, 64, 65, 1023, 1024, 1025, 4097]


def _fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic; int / int rounds correctly)."""
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _block_sum_replica(v):
    """csrc/reduce.h block_sum for a block of 1024 as its comment states it: v[t] is thread t's
    value; within each wave of 64 an xor butterfly over the lane offsets 32, 16, 8, 4, 2, 1, then
    the 16 wave sums (lane 0's) added in ascending order starting from 0."""
    w = np.asarray(v, dtype=np.float64).reshape(16, 64).copy()
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ o]
    t = 0.0
    for k in range(16):
        t = t + float(w[k, 0])
    return t


def _per_thread(x):
    """[1024] thread t's sequential double sum of x[t], x[t + 1024], ... from 0 (a missing element
    is a + 0.0 = a)."""
    pad = np.zeros(-(-x.size // 1024) * 1024)
    pad[:x.size] = x
    a = np.zeros(1024)
    for row in pad.reshape(-1, 1024):
        a = a + row
    return a


def _energy_stats_replica(x):
    """k_energy_stats (csrc/loss.hip, one block of 1024, finalize on) on the float64 array x:
    m = block_sum(per-thread sums) / n; the second pass the same on (e - m)^2, each thread's
    q += d * d being one fused multiply-add (the device compiler's default contraction; the
    compiled loop is v_add_f64, v_fmac_f64); out = [q, n m, (n m) m, n, m, q / n]."""
    nn = float(x.size)
    s = _block_sum_replica(_per_thread(x))
    m = s / nn
    q = [0.0] * 1024
    for i, e in enumerate(x.tolist()):
        d = e - m
        q[i % 1024] = _fma(d, d, q[i % 1024])
    qq = _block_sum_replica(q)
    return s, q, np.array([qq, nn * m, nn * m * m, nn, m, qq / nn])


# seeds at which the kernel's order and the exactly rounded sum give different bits (searched on
# the CPU, see test_energy_stats_bitwise_stated_order); 900 + n where not listed
STATS_SEED = {("f32", 63): 20963, ("f32", 64): 70964, ("f32", 65): 30965, ("f32", 1023): 821923, ("f32", 1024): 341924, ("f32", 1025): 1521925, ("f64", 63): 10963,
              ("f64", 64): 30964, ("f64", 1023): 11923, ("f64", 1025): 11925}


def _stats_input(n, dtype):
    """Both signs, magnitudes log-uniform over 1e-3 .. 1e5, rounded to dtype: a changed summation
    order changes the last bits."""
    rng = np.random.default_rng(STATS_SEED.get((DT_IDS[DTYPES.index(dtype)], n), 900 + n))
    x = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3.0, 5.0, n)
    return x.astype(NP_DT[dtype]).astype(np.float64)


@pytest.mark.parametrize("n", STATS_N)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_energy_stats_bitwise_stated_order(dtype, n):
    """aiqmc_energy_stats (finalize on) bit for bit against a host replica written from
    csrc/reduce.h's comment on block_sum: a partial wave, one wave, a wave boundary, a partial
    block, a full one and more than one element per thread.  The replica is first shown to differ
    from the exactly rounded sum (math.fsum) of the same numbers, so that the comparison can see a
    changed order: in the first pass (the sum of the energies) for every n > 1, except the
    float32 inputs with n <= 65, whose double sums are exact in any order (24-bit numbers between
    2^-10 and 2^17, at most 65 of them: under 53 bits) -- there in the second pass, the sum of
    the rounded (e - m)^2.  n = 1 has one term and no order."""
    import math
    from aiqmc import _lib
    x = _stats_input(n, dtype)
    s, q, want = _energy_stats_replica(x)
    exact, qexact = math.fsum(x.tolist()), math.fsum(q)
    print(n, "replica sum", repr(s), "fsum", repr(exact), "second pass", repr(want[0]), "fsum", repr(qexact))
    if n > 1 and (dtype == torch.float64 or n > 65):
        assert s != exact and abs(s - exact) <= 2.0 ** -45 * float(np.abs(x).sum())
    elif n > 1:
        assert s == exact and want[0] != qexact and abs(want[0] - qexact) <= 2.0 ** -45 * qexact
    got = _lib.energy_stats(torch.tensor(x, dtype=dtype, device="cuda"), finalize=True)
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    print("  replica", want.tolist())
    print("  kernel ", g.tolist())
    assert g.tobytes() == want.tobytes()
