"""B3 of a proposal takes the records of the moved electron's 2(N-1) pairs from F2 of the same wave
(walker_rev.h, the handover block), and the walker cache's pair record holds the tanh derivative
factors RSQ2 (1 - t^2) (WCache::pt; written by k_walker_rev's F2 and by quad_small.h's packed walker
launch).

One host-draw sweep with the walker cache (proposal reuse: the handover and the cached records)
against the same sweep with every proposal evaluated from scratch (B3 recomputes both double layers
for every pair), on the smallest and the edge shapes of k_walker_rev's proposal path (N >= 9):
  (9, 1)   odd N, unequal spin channels, the smallest N on this path
  (14, 2)  the benchmark's shape, three B3 iterations per lane
  (16, 1)  all 16 column lanes live, M = 30 handed-over pairs, four B3 iterations
A sweep's B N proposals move every electron once, so every pi is covered.  Tolerances are those of
test_gpu_fullsize.py::test_proposal_reuse_matches_recompute (fp64: positions to 1e-11, equal accept
counts) and ::test_proposal_reuse_matches_recompute_f32_4096 (fp32: fewer than 2e-3 of the walkers
further than 1e-4 apart -- none of these two or three).  The draws' seeds were chosen on the fp64
oracle so that no acceptance ratio of the sweep lies within MARGIN of its uniform (asserted here):
fp32 rounding moves a ratio by ~1e-4 of itself at most, so a flipped acceptance is a defect, not
rounding.

The packed walker launch (N <= 8, quad_small.h) writes the same record: one Be sweep of five walkers
against the fp64 oracle, as test_gpu_shapes.py does for its shapes.
"""
import numpy as np
import pytest
import torch

import support

pytestmark = pytest.mark.gpu

# shape -> (walkers, seed of the draws); seeds found by scanning 0, 1, ... on the oracle for MARGIN
CASES = {(9, 1): (3, 0), (14, 2): (3, 0), (16, 1): (2, 1)}
MARGIN = 1e-2


_REF = {}


def _case(shape):
    """(system, params, walkers, draws, oracle positions, oracle accept mask), cached per shape."""
    if shape not in _REF:
        n, a = shape
        B, seed = CASES[shape]
        s, params, pos = support.seeded_case(support.z_name(n, a), 300 + 3 * n + a, B, randomize_aux=True)
        draws = support.host_draws(seed, B, n)
        x_ref, acc = support.oracle_sweep(s, params, pos, draws, 0.05)
        u = draws[2][0].numpy()
        gap = np.abs(acc - u)
        print(f"{shape}: min |acceptance - u| = {gap.min():.3e}, accepted {(acc > u).sum()} of {acc.size}")
        assert gap.min() > MARGIN, (shape, seed, gap.min())
        _REF[shape] = (s, params, pos, draws, x_ref, acc > u)
    return _REF[shape]


def _gpu_sweep(s, params, pos, draws, dtype, reuse):
    """One mc_step sweep on a fresh context; (positions, accepted moves per walker)."""
    N, B = s.nelectrons, pos.shape[0]
    g1, g2, u = draws
    idx = torch.arange(N)
    ctx = support.make_ctx(s, dtype, params)
    ctx.set_proposal_reuse(reuse)
    x = torch.tensor(pos, dtype=dtype, device="cuda").contiguous()
    acc = ctx.mc_step(x, 1, 0.05, count_accepts=True, gauss1=g1,
                      gauss2=g2.reshape(1, B, N, N, 3)[:, :, idx, idx, :].contiguous(), u=u)
    torch.cuda.synchronize()
    return x, acc


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("shape", list(CASES), ids=lambda sh: f"N{sh[0]}A{sh[1]}")
def test_handover_sweep_matches_recompute(shape, dtype):
    s, params, pos, draws, x_ref, cond = _case(shape)
    B = pos.shape[0]
    a, acc_a = _gpu_sweep(s, params, pos, draws, dtype, True)
    b, acc_b = _gpu_sweep(s, params, pos, draws, dtype, False)
    d = (a - b).abs().reshape(B, -1).amax(1)
    print(f"{shape} {dtype}: max |reuse - recompute| = {float(d.max()):.3e}, "
          f"max |reuse - oracle| = {np.abs(a.double().cpu().numpy() - x_ref).max():.3e}")
    # no decision is near its uniform: both paths (and fp32) accept exactly the oracle's moves
    n_ref = torch.tensor(cond.sum(1), device=acc_a.device, dtype=acc_a.dtype)
    assert torch.equal(acc_a.reshape(-1), n_ref), (acc_a, n_ref)
    assert torch.equal(acc_a, acc_b)
    assert not torch.equal(a, torch.tensor(pos, dtype=dtype, device="cuda"))
    if dtype == torch.float64:
        assert torch.allclose(a, b, rtol=0, atol=1e-11), float((a - b).abs().max())
        np.testing.assert_allclose(a.cpu().numpy(), x_ref, rtol=1e-9, atol=1e-9)
    else:
        differ = (d > 1e-4).float().mean()
        assert float(differ) < 2e-3, float(differ)


def test_packed_walker_record_sweep_matches_oracle():
    """Be, five walkers (N <= 4: four walkers per wave, the second wave partial)."""
    s, params, pos = support.seeded_case("Be", 41, 5, randomize_aux=True)
    draws = support.host_draws(11, 5, s.nelectrons)
    x_ref, _ = support.oracle_sweep(s, params, pos, draws, 0.05)
    x, acc = _gpu_sweep(s, params, pos, draws, torch.float64, True)
    assert int(acc.sum()) > 0
    np.testing.assert_allclose(x.cpu().numpy(), x_ref, rtol=1e-9, atol=1e-9)
