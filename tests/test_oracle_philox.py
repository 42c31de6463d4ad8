"""oracle/philox.py, the float64 replica of the device Philox draws (CPU only).

Known answers: the Random123 vectors of Philox4x32-10.  Statistics: fixed seeds, so every figure
below is deterministic; every z-score must satisfy |z| <= 4.5 (two-sided tail 7e-6 per figure).
Word coverage: the high words of seed and step and the kind reach every draw.

The null-context check of the read-back export (aiqmc_debug_read_draws) is here too: it needs
the built library but no GPU.
"""
import numpy as np
import pytest

from oracle import philox

ZMAX = 4.5


# ----------------------------------------------------------------------------- known answers

@pytest.mark.parametrize("counter,key,want", [
    ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
     [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
])
def test_random123_known_answers(counter, key, want):
    got = philox.philox4x32_10(counter, key)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert [int(w) for w in got] == want


def test_vectorised_over_stream_ids_equals_one_at_a_time():
    sid = np.array([0, 1, 63, 64, 2 ** 31, 2 ** 32 - 1], dtype=np.uint64)
    all_ = philox.words(2 ** 40 + 9, 2 ** 33 + 5, sid, 2)
    for j, s in enumerate(sid):
        one = philox.philox4x32_10([int(s), 5, 2, 2], [9, 2 ** 8])
        assert np.array_equal(all_[:, j], one)


def test_uniform_grid_and_box_muller_order():
    sid = np.arange(1000, dtype=np.uint64)
    w = philox.words(3, 4, sid, 1)
    u = philox.u4(3, 4, sid, 1)
    assert np.array_equal(u, ((w >> 8).astype(np.float64) + 1.0) * 2.0 ** -24)
    assert u.min() >= 2.0 ** -24 and u.max() <= 1.0
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)      # exact in float32
    g = philox.normal3(3, 4, sid, 1)
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    np.testing.assert_allclose(g[0] ** 2 + g[1] ** 2, r0 ** 2, rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(np.arctan2(g[1], g[0]) % (2 * np.pi), (2 * np.pi * u[1]) % (2 * np.pi), atol=1e-12)
    np.testing.assert_allclose(g[2], r1 * np.cos(2 * np.pi * u[3]), rtol=0, atol=1e-15)


# ----------------------------------------------------------------------------- statistics

@pytest.fixture(scope="module")
def draws7():
    return philox.mc_draws(7, 0, 4, 4096, 14)


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float(a @ b / np.sqrt((a @ a) * (b @ b)))


def test_mc_draws_shapes_streams_and_kinds(draws7):
    g1, g2, u = draws7
    B, N = 4096, 14
    assert g1.shape == (4, B, 3 * N) and g2.shape == (4, B, N, 3) and u.shape == (4, B, N)
    # one stream id spelled out: sweep 2, walker 100, electron 5 -> sid = 100 * 14 + 5, step = 2
    sid = np.array([100 * N + 5], dtype=np.uint64)
    assert np.array_equal(g1[2, 100, 15:18], philox.normal3(7, 2, sid, 0)[:, 0])
    assert np.array_equal(g2[2, 100, 5], philox.normal3(7, 2, sid, 1)[:, 0])
    assert u[2, 100, 5] == philox.u4(7, 2, sid, 2)[0, 0] - 2.0 ** -24
    # the offset is the step of sweep 0
    h1, h2, hu = philox.mc_draws(7, 2, 1, 8, N)
    assert np.array_equal(h1[0], g1[2, :8]) and np.array_equal(h2[0], g2[2, :8]) and np.array_equal(hu[0], u[2, :8])


@pytest.mark.parametrize("which", [0, 1])
def test_normals_moments(draws7, which):
    """mc_draws(7, 0, 4, 4096, 14): 688,128 normals per array.  Mean, variance and fourth moment
    within 4.5 standard errors of 0, 1 and 3 (observed |z| up to 1.1, 0.09, 0.18); the largest
    |g| (4.67) is where 688k normals put it: P(|g| > 6) is 2e-9 per draw."""
    g = draws7[which].ravel()
    n = g.size
    assert n == 4 * 4096 * 14 * 3
    z_mean = g.mean() * np.sqrt(n)
    z_var = (np.mean(g * g) - 1.0) / np.sqrt(2.0 / n)          # Var(g^2) = 2
    z_m4 = (np.mean(g ** 4) - 3.0) / np.sqrt(96.0 / n)         # Var(g^4) = 105 - 9
    print(f"normals[{which}]: z mean {z_mean:.3f} var {z_var:.3f} m4 {z_m4:.3f} max|g| {np.abs(g).max():.3f}")
    assert abs(z_mean) <= ZMAX and abs(z_var) <= ZMAX and abs(z_m4) <= ZMAX
    assert 3.5 < np.abs(g).max() < 6.0


def test_normals_uncorrelated(draws7):
    """Sample correlations, each with standard error n^-1/2: gauss1 against gauss2 at the same
    index, sweep st against sweep st + 1, seed 7 against seed 8, and the three components of one
    Box-Muller call against each other."""
    g1, g2, _ = draws7
    a = g1.reshape(4, 4096, 14, 3)
    n = a.size
    z = {"g1.g2": _corr(a, g2) * np.sqrt(n)}
    for st in range(3):
        z[f"g1 sweep {st}.{st + 1}"] = _corr(a[st], a[st + 1]) * np.sqrt(n / 4)
        z[f"g2 sweep {st}.{st + 1}"] = _corr(g2[st], g2[st + 1]) * np.sqrt(n / 4)
    h1, h2, _ = philox.mc_draws(8, 0, 4, 4096, 14)
    z["g1 seed 7.8"] = _corr(g1, h1) * np.sqrt(n)
    z["g2 seed 7.8"] = _corr(g2, h2) * np.sqrt(n)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        z[f"g1 xyz {i}.{j}"] = _corr(a[..., i], a[..., j]) * np.sqrt(n / 3)
    print({k: round(v, 3) for k, v in z.items()})
    assert all(abs(v) <= ZMAX for v in z.values()), z


def test_uniforms(draws7):
    """u in [0, 1 - 2^-24]; the 64-bin chi-square (63 degrees of freedom: mean 63, standard
    deviation 11.2) below 120 (observed 48.8); mean and variance within 4.5 standard errors."""
    u = draws7[2].ravel()
    n = u.size
    assert u.min() >= 0.0 and u.max() <= 1.0 - 2.0 ** -24
    assert np.array_equal(u, np.round(u * 2 ** 24) / 2 ** 24)      # on the grid
    cnt = np.bincount((u * 64).astype(np.int64), minlength=64)
    chi2 = float(((cnt - n / 64) ** 2 / (n / 64)).sum())
    z_mean = (u.mean() - 0.5) / np.sqrt(1.0 / 12 / n)
    z_var = (u.var() - 1.0 / 12) / np.sqrt(1.0 / 180 / n)          # Var((u - 1/2)^2) = 1/180
    print(f"u: chi2 {chi2:.1f} z mean {z_mean:.3f} var {z_var:.3f}")
    assert chi2 < 120.0
    assert abs(z_mean) <= ZMAX and abs(z_var) <= ZMAX
    assert abs(_corr(u, draws7[0][..., ::3]) * np.sqrt(n)) <= ZMAX


@pytest.fixture(scope="module")
def rot5():
    return philox.haar_rotations(5, 0, 65536)


def test_rotations_are_orthogonal_with_fair_sign(rot5):
    R = rot5
    B = R.shape[0]
    assert R.shape == (65536, 3, 3)
    assert np.max(np.abs(np.einsum("bij,bkj->bik", R, R) - np.eye(3))) <= 1e-12
    det = np.linalg.det(R)
    assert np.max(np.abs(np.abs(det) - 1.0)) <= 1e-12
    z = ((det > 0).mean() - 0.5) / np.sqrt(0.25 / B)
    print(f"det +1 fraction z {z:.3f}")
    assert abs(z) <= ZMAX
    # the sign is kind 18's first uniform, compared with one half
    us = philox.u4(5, 0, np.arange(B, dtype=np.uint64), 18)[0]
    assert np.array_equal(det < 0, us < 0.5)


def test_rotations_are_haar(rot5):
    """Haar O(3): every entry has mean 0 (standard error sqrt(1/(3B))) and mean square 1/3
    (E R_ij^4 = 1/5, so standard error sqrt((1/5 - 1/9)/B)); observed max |z| 2.3 and 1.8.  The
    proper part S = det(R) R is Haar SO(3): its trace 1 + 2 cos(theta) has mean 0 and variance 1
    (E tr^2 = 1, E tr^4 = 3: standard errors sqrt(1/B) and sqrt(2/B))."""
    R = rot5
    B = R.shape[0]
    z1 = R.mean(axis=0) / np.sqrt(1.0 / 3 / B)
    z2 = ((R * R).mean(axis=0) - 1.0 / 3) / np.sqrt((1.0 / 5 - 1.0 / 9) / B)
    tr = np.linalg.det(R) * np.trace(R, axis1=1, axis2=2)
    zt = tr.mean() * np.sqrt(B)
    zv = (np.mean(tr * tr) - 1.0) / np.sqrt(2.0 / B)
    print(f"rot: max|z| mean {np.abs(z1).max():.3f} meansq {np.abs(z2).max():.3f} trace {zt:.3f} {zv:.3f}")
    assert np.abs(z1).max() <= ZMAX and np.abs(z2).max() <= ZMAX
    assert abs(zt) <= ZMAX and abs(zv) <= ZMAX
    # distinct entries of one matrix are uncorrelated
    for (i, j), (k, l) in (((0, 0), (1, 1)), ((0, 1), (1, 0)), ((0, 2), (2, 2))):
        assert abs(_corr(R[:, i, j], R[:, k, l]) * np.sqrt(B)) <= ZMAX


def test_tmove_draws():
    B, N = 4096, 4
    us, ua = philox.tmove_draws(7, 1, B, N)
    assert us.shape == (B,) and ua.shape == (B, N)
    assert us.min() >= 0.0 and us.max() <= 1.0 - 2.0 ** -24 and ua.min() >= 0.0 and ua.max() <= 1.0 - 2.0 ** -24
    assert us[3] == philox.u4(7, 1, np.array([3], dtype=np.uint64), 19)[0, 0] - 2.0 ** -24
    assert ua[3, 2] == philox.u4(7, 1, np.array([3 * N + 2], dtype=np.uint64), 20)[0, 0] - 2.0 ** -24
    assert abs((ua.mean() - 0.5) / np.sqrt(1.0 / 12 / ua.size)) <= ZMAX
    assert abs((us.mean() - 0.5) / np.sqrt(1.0 / 12 / us.size)) <= ZMAX
    # electron 0's acceptance uniform is not the walker's selection uniform (kinds 19 and 20)
    assert abs(_corr(us, ua[:, 0]) * np.sqrt(B)) <= ZMAX


# ----------------------------------------------------------------------------- word coverage

def test_high_words_of_step_and_seed_reach_every_draw():
    B, N = 64, 14
    base = philox.mc_draws(7, 3, 1, B, N)
    for seed, off in ((7, 3 + 2 ** 32), (7 + 2 ** 32, 3)):
        other = philox.mc_draws(seed, off, 1, B, N)
        for a, b in zip(base, other):
            assert not np.any(a == b), (seed, off)
    r0 = philox.haar_rotations(5, 2, B)
    assert not np.any(r0 == philox.haar_rotations(5, 2 + 2 ** 32, B))
    assert not np.any(r0 == philox.haar_rotations(5 + 2 ** 32, 2, B))
    t0 = philox.tmove_draws(7, 1, B, N)
    for seed, off in ((7, 1 + 2 ** 32), (7 + 2 ** 32, 1)):
        t1 = philox.tmove_draws(seed, off, B, N)
        # 24-bit uniforms: two of 896 coincide by chance with probability 5e-5 each
        assert np.mean(t0[0] == t1[0]) < 0.01 and np.mean(t0[1] == t1[1]) < 0.01


def test_kinds_differ_at_one_stream_id():
    sid = np.arange(896, dtype=np.uint64)
    w = [philox.words(7, 0, sid, k) for k in (0, 1, 2)]
    for i in range(3):
        for j in range(i + 1, 3):
            assert not np.any(np.all(w[i] == w[j], axis=0))
    g1, g2, u = philox.mc_draws(7, 0, 1, 64, 14)
    assert not np.any(g1.reshape(64, 14, 3) == g2[0])


def test_out_of_range_seed_or_step_is_refused():
    with pytest.raises(ValueError):
        philox.words(-1, 0, 0, 0)
    with pytest.raises(ValueError):
        philox.words(0, 2 ** 64, 0, 0)


# ----------------------------------------------------------------------------- the read-back export

def test_read_draws_refuses_a_null_context_without_a_gpu():
    from aiqmc import _lib
    lib = _lib.load()
    assert lib.aiqmc_debug_read_draws(None, 0, None, 4, None) < 0
    assert "context" in _lib.last_error()
