"""The argument vocabulary of aiqmc._lib.Context (_rng, _weights, _acc, _dev, _obs_chunk) on the
CPU: a Context that never saw the library (object.__new__, device cpu, float64, N = 2, A = 1)."""
import itertools

import pytest
import torch

from aiqmc import _lib


@pytest.fixture
def ctx():
    c = object.__new__(_lib.Context)
    c.device, c.dtype, c.N, c.A = torch.device("cpu"), torch.float64, 2, 1
    c._h = None   # __del__ finds no handle
    return c


B = 3
DRAWS = {"gauss1": 3 * B * 2, "gauss2": B * 2 * 3, "u": B * 2}


def _draws(names, wrong=None):
    return {k: (torch.zeros(n + (k == wrong)) if k in names else None, n) for k, n in DRAWS.items()}


def test_rng_all_or_nothing(ctx):
    mode, staged = ctx._rng("mc_step", **_draws(()))
    assert mode == _lib.AIQMC_RNG_PHILOX and staged == (None, None, None)
    mode, staged = ctx._rng("mc_step", **_draws(DRAWS))
    assert mode == _lib.AIQMC_RNG_HOST
    assert [t.numel() for t in staged] == list(DRAWS.values())
    assert all(t.dtype == torch.float64 and t.is_contiguous() for t in staged)
    for pair in itertools.combinations(DRAWS, 2):
        with pytest.raises(ValueError, match="gauss1, gauss2 and u are injected together or not at all"):
            ctx._rng("mc_step", **_draws(pair))
    for one in DRAWS:
        with pytest.raises(ValueError, match="injected together or not at all"):
            ctx._rng("mc_step", **_draws((one,)))


def test_rng_wording_of_the_other_sets(ctx):
    with pytest.raises(ValueError, match="rot, u_sel and u_acc are injected together or not at all"):
        ctx._rng("dmc_tmoves", rot=(torch.zeros(9 * B), 9 * B), u_sel=(None, B), u_acc=(None, 2 * B))
    mode, (r,) = ctx._rng("local_energy_ecp", rot=(None, 9 * B))
    assert mode == _lib.AIQMC_RNG_PHILOX and r is None


@pytest.mark.parametrize("wrong", list(DRAWS))
def test_rng_wrong_size_names_the_draw(ctx, wrong):
    with pytest.raises(ValueError, match=rf"mc_step: {wrong}: expected {DRAWS[wrong]} values, got {DRAWS[wrong] + 1}"):
        ctx._rng("mc_step", **_draws(DRAWS, wrong=wrong))


def test_weights(ctx):
    assert ctx._weights(None, B) is None
    w = ctx._weights([1, 2, 3], B)
    assert w.dtype == torch.float64 and w.shape == (B,) and w.tolist() == [1.0, 2.0, 3.0]
    assert ctx._weights(torch.ones(B, 1, dtype=torch.float32), B).shape == (B,)
    for bad in ([1.0, 2.0], torch.ones(B + 1)):
        with pytest.raises(ValueError, match="^weights must have one entry per walker$"):
            ctx._weights(bad, B)


def test_acc(ctx):
    good = torch.zeros(17, dtype=torch.int64)
    assert ctx._acc(good, 17, torch.int64, "density_accumulate") is good
    cases = {"dtype": torch.zeros(17, dtype=torch.float64), "numel": torch.zeros(16, dtype=torch.int64),
             "non-contiguous": torch.zeros(34, dtype=torch.int64)[::2], "not a tensor": [0] * 17}
    for bad in cases.values():
        with pytest.raises(ValueError, match="^density_accumulate: acc must be a contiguous int64 tensor of 17 words"):
            ctx._acc(bad, 17, torch.int64, "density_accumulate")
    with pytest.raises(ValueError, match="^rdm_accumulate: acc must be a contiguous float64 tensor of 5 words on cpu"):
        ctx._acc(good, 5, torch.float64, "rdm_accumulate")


def test_dev(ctx):
    t = ctx._dev([[1, 2], [3, 4]], 4)
    assert t.dtype == torch.float64 and t.is_contiguous() and t.shape == (2, 2)
    assert ctx._dev(torch.arange(6.0)[::2], 3).is_contiguous()
    assert ctx._dev(torch.ones(5), None).numel() == 5          # n None: any size
    z = torch.tensor([1 + 2j, 3 - 1j])
    assert ctx._dev(z, 2, "eloc_old", real=True).tolist() == [1.0, 3.0]
    assert ctx._dev(torch.ones(2, dtype=torch.float32), 2, real=True).dtype == torch.float64
    with pytest.raises(ValueError, match="^expected 3 values, got 2$"):
        ctx._dev(torch.ones(2), 3)
    with pytest.raises(ValueError, match="^eloc_old: expected 3 values, got 2$"):
        ctx._dev(z, 3, "eloc_old", real=True)


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, name, *args, stream=True, raw=False):
        self.calls.append((name, args, stream))


def test_obs_chunk(ctx):
    ctx._call = rec = _Recorder()
    with ctx._obs_chunk(None):
        pass
    assert rec.calls == []
    for bad in (0, -4):
        with pytest.raises(ValueError, match="chunk must be positive"):
            with ctx._obs_chunk(bad):
                pytest.fail("the body ran")
    assert rec.calls == []
    with ctx._obs_chunk(96):
        assert rec.calls == [("aiqmc_debug_set_obs_chunk", (96,), False)]
    assert rec.calls[1:] == [("aiqmc_debug_set_obs_chunk", (0,), False)]
    del rec.calls[:]
    with pytest.raises(KeyError):
        with ctx._obs_chunk(7):
            raise KeyError("body")
    assert rec.calls == [("aiqmc_debug_set_obs_chunk", (7,), False), ("aiqmc_debug_set_obs_chunk", (0,), False)]
