"""The multi-rank loss levels' host restatement (aiqmc.Loss.loss._host_level / _mean_var, what gloo
ranks run) through the assertions of the HIP level kernels (tests/test_gpu_reductions.py): R ranks
simulated by slicing one batch and adding the rank vectors, unequal splits included, against the
numpy float64 restatement of the formulas in csrc/loss.hip's k_lossr_* header comment.  CPU only."""
import numpy as np
import pytest
import torch

from replicas_loss import (CLIPS, DT_IDS, DTYPES, LOSS_B, SPLITS, _assert_stats, _check_edges, _check_levels,
                           _loss_energies, _loss_reference, _run_levels)


def _final_host(L1, head, g0, center, world):
    from aiqmc.Loss import loss as L
    mr, mi, var = (float(v) for v in L._mean_var(L1))
    n = float(L1[4])
    dc = (float(head[0]) / n, float(head[1]) / n) if center else (mr, mi)
    return np.array([mr, mi, var, dc[0], dc[1], float(L1[5])])


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("clip,center", CLIPS)
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_host_levels_simulated_ranks(dtype, cplx, clip, center, split):
    """Loss.loss._host_level / _mean_var (what gloo ranks run) through the assertions of the HIP
    level kernels, unequal splits included."""
    from aiqmc.Loss import loss as L
    sizes = SPLITS[split]
    x, y = _loss_energies(dtype, cplx)
    wscale = 2.0 / LOSS_B
    g0 = clip > 0 and center
    ref = _loss_reference(x, y, clip, center, wscale)
    L1, L2, ranks, _ = _run_levels(L._host_level, x, y, sizes, clip, center, wscale, dtype, "cpu")
    head = _check_levels(L1, ranks, ref, cplx, g0, wscale, dtype, LOSS_B)
    st = _final_host(L1, head, g0, g0, len(sizes))
    _assert_stats(st, ref, cplx)
    assert st[5] == ref["nz"]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_host_level_edge_batches(dtype):
    from aiqmc.Loss import loss as L
    _check_edges(L._host_level, _final_host, dtype, "cpu")


def test_levels_pool_over_walkers_not_rank_means():
    """The deviation noted in fused_levels' docstring, in numbers.  The reference's loss is
    pmean(mean(e)) (Loss/loss.py:206): the mean of the rank means.  The levels weight every
    walker equally: E = sum n_r m_r / sum n_r.  Equal rank batches: the same number.  Unequal
    rank batches: the levels still give the pooled mean, the mean of rank means is another number."""
    from aiqmc.Loss import loss as L
    e = np.array([-10.0, -11.0, -12.0, -13.0, -14.0, -15.0])
    pooled = e.mean()                                      # -12.5
    for sizes, rank_means in (([3, 3], [-11.0, -14.0]), ([1, 5], [-10.0, -13.0])):
        parts = np.split(e, np.cumsum(sizes)[:-1])
        assert [p.mean() for p in parts] == rank_means
        L1 = sum(L._host_level(1, torch.tensor(p), None) for p in parts)
        mr, _, var = L._mean_var(L1)
        assert float(mr) == pooled == -12.5
        np.testing.assert_allclose(float(var), np.mean((e - pooled) ** 2), rtol=1e-14)
    assert np.mean([-11.0, -14.0]) == pooled               # equal split: mean of rank means = pooled
    assert np.mean([-10.0, -13.0]) == -11.5 != pooled      # unequal split: the reference's differs
