"""References that a host test and a GPU test of the same estimator share: the blocking accumulator's
words (tests/test_blocking_host.py, tests/test_gpu_blocking.py), the RDM test basis
(tests/test_rdm_host.py, tests/test_gpu_rdm.py) and the S^2 / RDM ratio tolerances
(tests/test_gpu_observables.py, tests/test_gpu_rdm.py).  A plain module, as support.py."""
import numpy as np
import torch

# ----------------------------------------------------------------------------- blocking words
U = 2.0 ** -53


def _sums(blocks, B, K):
    """Per-level sums of a list of block arrays [nb, K, B]: n [L], S [L, K], Q [L, K (K + 1) / 2]
    and the sums of the absolute terms aS, aQ (numpy's summation order)."""
    iu = np.triu_indices(K)
    L = len(blocks)
    out = {"n": np.zeros(L), "S": np.zeros((L, K)), "Q": np.zeros((L, iu[0].size)), "aS": np.zeros((L, K)),
           "aQ": np.zeros((L, iu[0].size))}
    for k, v in enumerate(blocks):
        if v.shape[0] == 0:
            continue
        out["n"][k] = v.shape[0] * B
        out["S"][k] = v.sum(axis=(0, 2))
        out["aS"][k] = np.abs(v).sum(axis=(0, 2))
        p = v[:, iu[0]] * v[:, iu[1]]
        out["Q"][k] = p.sum(axis=(0, 2))
        out["aQ"][k] = np.abs(p).sum(axis=(0, 2))
    return out


def pair_reblock(trace, shift, L):
    """The same blocks as (first + second) / 2 of the level below: the recurrence's own terms."""
    T, K, B = trace.shape
    v = trace.astype(np.float64) - np.asarray(shift, dtype=np.float64)[None, :, None]
    blocks = []
    for k in range(L):
        blocks.append(v)
        nb = v.shape[0] // 2
        v = (v[0:2 * nb:2] + v[1:2 * nb:2]) / 2.0
    return _sums(blocks, B, K), blocks


def words_of(acc):
    """(t, n [L], S [L, K], Q [L, Kq]) of an accumulator, numpy float64 on the host."""
    a = acc.acc.detach().cpu().numpy()
    w = a[1 + acc.K:].reshape(acc.L, acc.M)
    return a[0], w[:, 0].copy(), w[:, 1:1 + acc.K].copy(), w[:, 1 + acc.K:].copy()


def assert_words(acc, ref, T, factor, what=""):
    """Counts and t exact; every S and Q word within factor * sum |term| of the reference, where
    factor is a float or a callable of the word's term count."""
    t, n, S, Q = words_of(acc)
    assert t == T, (what, t)
    np.testing.assert_array_equal(n, ref["n"], err_msg=what)
    f = np.array([factor(x) if callable(factor) else factor for x in ref["n"]])[:, None]
    for got, want, scale, name in ((S, ref["S"], ref["aS"], "S"), (Q, ref["Q"], ref["aQ"], "Q")):
        err, bound = np.abs(got - want), f * scale
        assert np.all(err <= bound), (what, name, float((err - bound).max()), float(err.max()))


def order_bound(n):
    """2 n u: two summation orders of the same n fp64 terms, as a factor of sum |term|."""
    return 2.0 * n * U


# ----------------------------------------------------------------------------- RDM test basis
C0, C1 = np.array([0.1, -0.2, 0.3]), np.array([-0.4, 0.5, 0.2])


def _shells(obs):
    """s, p and d shells on two centres (nao = 20), contracted and not."""
    S = obs.Shell
    return [S(C0, 0, [1.3, 0.4], obs.normalized_shell(0, [1.3, 0.4], [0.6, 0.5])), S(C0, 1, [0.9], [0.7]),
            S(C0, 2, [0.7], obs.normalized_shell(2, [0.7], [1.0])),
            S(C1, 0, [0.5], [1.1]), S(C1, 1, [1.1, 0.35], [0.3, -0.8]), S(C1, 2, [0.45, 0.8], [0.5, 0.25])]


# ----------------------------------------------------------------------------- S^2 / RDM ratios
# (rtol, atol) of dlogabs and atol of cos / sin of dphase: the single-value bounds, doubled
TOL = {torch.float64: (2e-10, 2e-10, 2e-9), torch.float32: (2e-5, 4e-4, 4e-4)}
