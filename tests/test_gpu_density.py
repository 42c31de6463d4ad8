"""aiqmc_density_accumulate / aiqmc_density_layout on the GPU against the float64 numpy replica of
tests/test_density_host.py (`replica`: the bin rule written out directly, nothing from the package).

Every comparison first asserts that its seeded input has no edge sample (|f - rint(f)| <= 1e-4 for a
float32 context, f <= 64 in these tests; 1e-10 for float64) and then demands exact integer equality
of every accumulator word.  Systems: H2 (N = 2: the up-up and down-down pair channels stay empty),
Be (4, 1), Z5 (N = 5, nspins (3, 2): odd, unequal channels), N2 (14, 2), Z5@duddd (spin-polarised,
nspins (1, 4), the one up electron in slot 1).  Batches 1 and 70 (70 is
neither a wave nor a workgroup multiple, and more than one workgroup of 32 walkers); 6-16 bins per
axis.  The replica of a (system, families, weights) case is computed once and shared.
"""
import ctypes

import numpy as np
import pytest
import torch

import replicas as H
import support
from replicas import GRID, ONE, PAIR, RADIAL, TOL, replica, walkers

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
ALL = dict(grid=GRID, radial=RADIAL, pair=PAIR)
_CTX, _REF = {}, {}


def _ctx(name, dtype):
    if (name, dtype) not in _CTX:
        from oracle import system
        atoms, per, spins = H.geometry(name)
        s = system.make_system(name)
        assert np.array_equal(s.atoms, atoms) and np.array_equal(s.spins, spins)
        _CTX[(name, dtype)] = support.make_ctx(s, dtype, atoms=atoms)
    return _CTX[(name, dtype)]


def _ref(name, B, fams, dtype, weights=None):
    """The replica of the first B seeded walkers of `name` (cached; edge-free asserted)."""
    key = (name, B, fams, dtype, weights is not None)
    if key not in _REF:
        atoms, _, spins = H.geometry(name)
        kw = {k: ALL[k] for k in fams}
        ref, edges = replica(walkers(name)[:B], atoms, spins, weights=weights, tol=TOL[dtype], **kw)
        assert edges == 0
        _REF[key] = ref
    return _REF[key]


def _weights(B=H.BMAX):
    return np.random.default_rng(17).uniform(0.0, 2.0, B).astype(np.float32).astype(np.float64)


def _run(ctx, pos, kw, weights=None, acc=None):
    """(words on the host, layout) after one accumulate call (into acc when given)."""
    from aiqmc import _lib
    cfg = _lib.density_cfg(**kw)
    lay = ctx.density_layout(cfg)
    if acc is None:
        acc = torch.zeros(lay["n_words"], dtype=torch.int64, device=ctx.device)
    x = torch.tensor(np.asarray(pos), dtype=ctx.dtype, device=ctx.device).reshape(-1, 3 * ctx.N)
    w = None if weights is None else torch.tensor(weights, dtype=ctx.dtype, device=ctx.device)
    ctx.density_accumulate(x, acc, cfg, w)
    torch.cuda.synchronize()
    return acc, lay


def _named(acc, lay):
    w = acc.cpu().numpy()
    return {k: w[o:o + lay["sizes"][k]] for k, o in lay["offsets"].items()}


def _assert_equal(acc, lay, ref):
    got = _named(acc, lay)
    for k in H.FIELDS:
        if k in ref:
            np.testing.assert_array_equal(got[k], ref[k].reshape(-1), err_msg=k)
        else:
            assert got[k].size == 0, k


@pytest.mark.parametrize("fams", [("grid", "radial", "pair"), ("grid",), ("radial",), ("pair",)],
                         ids=["all", "grid", "radial", "pair"])
@pytest.mark.parametrize("B", [1, 70])
@pytest.mark.parametrize("name", list(H.SYSTEMS))
@DTYPES
def test_words_equal_the_replica(dtype, name, B, fams):
    ref = _ref(name, B, fams, dtype)
    acc, lay = _run(_ctx(name, dtype), walkers(name)[:B], {k: ALL[k] for k in fams})
    assert lay["privatised"]
    _assert_equal(acc, lay, ref)


@pytest.mark.parametrize("name", list(H.SYSTEMS))
@DTYPES
def test_weighted_words_and_conservation(dtype, name):
    """Weights in [0, 2): every word is the replica's sum of rint(w 2^32) in int64; per channel,
    inside + outside = total x the electrons (pairs) of the channel."""
    w = _weights()
    ref = _ref(name, H.BMAX, ("grid", "radial", "pair"), dtype, weights=w)
    ctx = _ctx(name, dtype)
    acc, lay = _run(ctx, walkers(name), ALL, weights=w)
    _assert_equal(acc, lay, ref)
    c = _named(acc, lay)
    tot = int(c["total"][0])
    assert tot == int(np.rint(w * 2.0 ** 32).astype(np.int64).sum()) and c["skipped"][0] == 0
    nup, ndn = ctx.nspins
    A = ctx.A
    np.testing.assert_array_equal(c["grid"].reshape(2, -1).sum(1) + c["grid_out"], [tot * nup, tot * ndn])
    np.testing.assert_array_equal(c["radial"].reshape(2, A, -1).sum(2) + c["radial_out"].reshape(2, A),
                                  np.array([[tot * nup], [tot * ndn]]).repeat(A, 1))
    np.testing.assert_array_equal(c["pair"].reshape(3, -1).sum(1) + c["pair_out"],
                                  [tot * (nup * (nup - 1) // 2), tot * (ndn * (ndn - 1) // 2), tot * nup * ndn])
    if name == "H2":
        assert c["pair"].reshape(3, -1)[:2].sum() == 0 and c["pair_out"][:2].sum() == 0


@DTYPES
def test_polarised_minority_first_channel_totals(dtype):
    """Z5@duddd, nspins (1, 4) with the one up electron in slot 1: every word equals the replica, the
    spin-resolved grid totals are n_up B and n_down B (not swapped), the pair channels hold
    n_up (n_up - 1) / 2 = 0, n_down (n_down - 1) / 2 = 6 and n_up n_down = 4 pairs per walker, and the
    up channel is exactly what slot 1 alone gives."""
    name, B = "Z5@duddd", H.BMAX
    ctx = _ctx(name, dtype)
    assert ctx.nspins == (1, 4)
    acc, lay = _run(ctx, walkers(name), ALL)
    _assert_equal(acc, lay, _ref(name, B, ("grid", "radial", "pair"), dtype))
    c = _named(acc, lay)
    assert c["total"][0] == B * H.ONE
    np.testing.assert_array_equal(c["grid"].reshape(2, -1).sum(1) + c["grid_out"], [1 * B * H.ONE, 4 * B * H.ONE])
    np.testing.assert_array_equal(c["radial"].reshape(2, -1).sum(1) + c["radial_out"], [1 * B * H.ONE, 4 * B * H.ONE])
    np.testing.assert_array_equal(c["pair"].reshape(3, -1).sum(1) + c["pair_out"], [0, 6 * B * H.ONE, 4 * B * H.ONE])
    atoms, _, _ = H.geometry(name)
    slot1, edges = replica(walkers(name).reshape(B, 5, 3)[:, 1].reshape(B, 3), atoms, np.array([1.0]), tol=TOL[dtype],
                           grid=GRID, radial=RADIAL)
    assert edges == 0
    np.testing.assert_array_equal(c["grid"].reshape(2, -1)[0], slot1["grid"][0].reshape(-1))
    np.testing.assert_array_equal(c["radial"].reshape(2, -1)[0], slot1["radial"][0].reshape(-1))


@pytest.mark.parametrize("name", ["Z5", "N2"])
@DTYPES
def test_halves_and_permutation_give_the_same_bits(dtype, name):
    ctx = _ctx(name, dtype)
    pos, w = walkers(name), _weights()
    whole, lay = _run(ctx, pos, ALL, weights=w)
    _assert_equal(whole, lay, _ref(name, H.BMAX, ("grid", "radial", "pair"), dtype, weights=w))
    halves, _ = _run(ctx, pos[:33], ALL, weights=w[:33])
    halves, _ = _run(ctx, pos[33:], ALL, weights=w[33:], acc=halves)
    assert torch.equal(halves, whole)
    p = np.random.default_rng(3).permutation(H.BMAX)
    perm, _ = _run(ctx, pos[p], ALL, weights=w[p])
    assert torch.equal(perm, whole)


@DTYPES
def test_maximum_contention_closed_form(dtype):
    """4,096 identical N2 walkers whose up electrons sit in one grid cell and the down electrons in
    another: every sample of a channel lands in ONE bin, whose word must be the closed form
    4096 x (samples of the channel) x 2^32.  A flush or an atomic that loses updates fails here."""
    name, B = "N2", 4096
    atoms, _, spins = H.geometry(name)
    one = np.empty((14, 3))
    for e in range(14):
        base = np.array([0.3, 0.4, 0.5]) if spins[e] > 0 else np.array([-1.2, 0.6, -1.0])
        one[e] = base + 1e-3 * np.array([e, -e, 2 * e])
    one = one.reshape(1, -1).astype(np.float32).astype(np.float64)
    ref1, edges = replica(one, atoms, spins, tol=TOL[dtype], **ALL)
    assert edges == 0
    for k, n_ch in (("grid", 2), ("radial", 4), ("pair", 3)):
        assert (ref1[k].reshape(n_ch, -1) != 0).sum(1).tolist() == [1] * n_ch, k    # one bin per channel
        assert ref1[k + "_out"].sum() == 0
    acc, lay = _run(_ctx(name, dtype), np.repeat(one, B, axis=0), ALL)
    c = _named(acc, lay)
    assert c["total"][0] == B * ONE and c["skipped"][0] == 0
    for k, per_walker in (("grid", [7, 7]), ("radial", [7, 7, 7, 7]), ("pair", [21, 21, 49])):
        got = c[k].reshape(len(per_walker), -1)
        np.testing.assert_array_equal(got.max(1), [B * n * ONE for n in per_walker], err_msg=k)
        np.testing.assert_array_equal(got.sum(1), got.max(1), err_msg=k)
        np.testing.assert_array_equal(got != 0, ref1[k].reshape(len(per_walker), -1) != 0, err_msg=k)
        assert c[k + "_out"].sum() == 0


@DTYPES
def test_both_sides_of_the_privatisation_limit(dtype):
    """radial (4, 16) against radial (4 K, 16 K) with K = 65: the same bin width exactly (inv_h = 4),
    so walkers within 4 bohr of both atoms fill the same bins; the first has 127 small words (LDS
    path), the second 4,211 > AIQMC_DENSITY_LDS_WORDS (global atomics).  Same input, same words."""
    from aiqmc import _lib
    name, K = "N2", 65
    ctx = _ctx(name, dtype)
    atoms, per, spins = H.geometry(name)
    pos = walkers(name, seed=6)     # the first seed whose contracted walkers have no edge sample
    block = np.concatenate([np.tile(atoms[i], per[i]) for i in range(2)])
    pos = (block + 0.4 * (pos - block)).astype(np.float32).astype(np.float64)
    small = dict(ALL)
    big = dict(ALL, radial=(RADIAL[0] * K, RADIAL[1] * K))
    ref_s, e_s = replica(pos, atoms, spins, tol=TOL[dtype], **small)
    ref_b, e_b = replica(pos, atoms, spins, tol=TOL[dtype], **big)
    assert e_s == 0 and e_b == 0 and ref_s["radial_out"].sum() == 0
    a_s, l_s = _run(ctx, pos, small)
    a_b, l_b = _run(ctx, pos, big)
    assert l_s["privatised"] and not l_b["privatised"]
    assert l_s["n_words"] - l_s["offsets"]["radial"] <= _lib.DENSITY_LDS_WORDS < l_b["n_words"] - l_b["offsets"]["radial"]
    _assert_equal(a_s, l_s, ref_s)
    _assert_equal(a_b, l_b, ref_b)
    c_s, c_b = _named(a_s, l_s), _named(a_b, l_b)
    for k in ("total", "skipped", "grid", "grid_out", "radial_out", "pair", "pair_out"):
        np.testing.assert_array_equal(c_s[k], c_b[k], err_msg=k)
    rb = c_b["radial"].reshape(2, 2, RADIAL[1] * K)
    np.testing.assert_array_equal(rb[:, :, :RADIAL[1]], c_s["radial"].reshape(2, 2, RADIAL[1]))
    assert rb[:, :, RADIAL[1]:].sum() == 0


def test_exactly_at_the_limit_is_privatised():
    """Be (A = 1): radial 2 n + 2 and pair 3 m + 3 words; n = 2044, m = 1 is exactly 4,096 words (the
    largest LDS footprint), m = 2 is over.  float64: f reaches 2,044 here, beyond the float32 cap."""
    from aiqmc import _lib
    ctx = _ctx("Be", torch.float64)
    atoms, _, spins = H.geometry("Be")
    pos = walkers("Be")
    for m, priv in ((1, True), (2, False)):
        kw = dict(radial=(6.0, 2044), pair=(7.0, m))
        lay = ctx.density_layout(_lib.density_cfg(**kw))
        assert lay["n_words"] - 2 == 4096 + 3 * (m - 1) and lay["privatised"] is priv
        ref, edges = replica(pos, atoms, spins, tol=1e-10, **kw)
        assert edges == 0
        acc, lay = _run(ctx, pos, kw)
        _assert_equal(acc, lay, ref)


@DTYPES
def test_rejected_weights_and_non_finite_coordinates(dtype):
    name = "Z5"
    ctx = _ctx(name, dtype)
    atoms, _, spins = H.geometry(name)
    pos = walkers(name)[:12].copy()
    w = _weights(12)
    w[3], w[7], w[9] = np.nan, -0.5, np.inf
    pos[1, 4], pos[2, 0], pos[3, 2] = np.nan, np.inf, np.nan
    ref, edges = replica(pos, atoms, spins, weights=w, tol=TOL[dtype], **ALL)
    assert edges == 0 and ref["skipped"][0] == 3
    acc, lay = _run(ctx, pos, ALL, weights=w)
    _assert_equal(acc, lay, ref)
    # electron 1 of walker 1 and electron 0 of walker 2 are outside in every family they enter
    q = np.rint(w * 2.0 ** 32)
    c = _named(acc, lay)
    assert c["grid_out"][1] >= q[1] and c["grid_out"][0] >= q[2]
    assert c["pair_out"].sum() >= 4 * (q[1] + q[2])
    # B = 0 leaves the accumulator untouched
    again, _ = _run(ctx, pos[:0], ALL, acc=acc.clone())
    assert torch.equal(again, acc)


def test_c_validation_messages():
    from aiqmc import _lib
    ctx = _ctx("H2", torch.float32)
    lay = lambda **kw: ctx.density_layout(_lib.density_cfg(**kw))
    for kw, msg in ((dict(grid=((0, 0, 0), (1, 0, 1), (4, 4, 4))), r"grid_hi\[1\] <= grid_lo\[1\]"),
                    (dict(grid=((0, 0, 0), (1, 1, 1), (4, 4, -4))), r"negative grid_n\[2\]"),
                    (dict(radial=(1.0, -1)), "negative rad_n"), (dict(pair=(1.0, -1)), "negative pair_n"),
                    (dict(radial=(0.0, 4)), "rad_max"), (dict(pair=(float("inf"), 4)), "pair_max"),
                    (dict(grid=((0, 0, 0), (1, 1, 1), (1 << 10, 1 << 10, 1 << 10))), "AIQMC_DENSITY_MAX_WORDS")):
        with pytest.raises(RuntimeError, match=msg):
            lay(**kw)
    cfg = _lib.density_cfg(pair=(2.0, 4))
    acc = torch.zeros(17, dtype=torch.int64, device="cuda")
    x = torch.zeros(1, 6, device="cuda")
    rc = ctx._lib.aiqmc_density_accumulate(ctx._h, ctypes.byref(cfg), x.data_ptr(), -1, None, acc.data_ptr(), None)
    assert rc == -1 and "negative batch" in _lib.last_error()
    rc = ctx._lib.aiqmc_density_accumulate(ctx._h, ctypes.byref(cfg), x.data_ptr(), 1, None, None, None)
    assert rc == -1 and "accumulator" in _lib.last_error()
    with pytest.raises(ValueError, match="17 words"):
        ctx.density_accumulate(x, acc[:16], cfg)
    torch.cuda.synchronize()
    assert int(acc.abs().sum()) == 0


@DTYPES
def test_make_density_on_a_network_equals_the_host_path(dtype):
    from aiqmc import observables, systems
    from aiqmc.wavefunction_Ynlm import nn
    s = systems.make_system("N2")
    net = s.make_network()
    pos, w = walkers("N2"), _weights()
    assert _ref("N2", H.BMAX, ("grid", "radial", "pair"), dtype, weights=w) is not None   # edge-free
    dev = observables.make_density(net.apply, s.nspins, **ALL)
    host = observables.make_density(lambda *a: None, s.nspins, **ALL)
    for sl in (slice(0, 40), slice(40, 70)):     # the accumulator lives across updates
        dev.update(None, nn.AINetData(positions=torch.tensor(pos[sl], dtype=dtype, device="cuda"), spins=s.spins,
                                      atoms=s.atoms, charges=s.charges), weights=torch.tensor(w[sl]))
        host.update(None, nn.AINetData(positions=torch.tensor(pos[sl], dtype=dtype), spins=s.spins, atoms=s.atoms,
                                       charges=s.charges), weights=torch.tensor(w[sl]))
    assert dev.words.is_cuda and not host.words.is_cuda
    assert torch.equal(dev.words.cpu(), host.words)
    H.assert_counts_equal(dev.counts, _ref("N2", H.BMAX, ("grid", "radial", "pair"), dtype, weights=w))
    dev.reduce()                                  # one process: the identity
    assert torch.equal(dev.words.cpu(), host.words)
    r = dev.result()
    np.testing.assert_allclose(r["pair"].sum(1).numpy() + r["pair_outside"].numpy(), [21, 21, 49], rtol=1e-13)
