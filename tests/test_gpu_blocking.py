"""aiqmc_blocking_update on the GPU against the torch path of aiqmc.statistics and the numpy
``pair_reblock`` of tests/test_blocking_host.py (blocks formed as (first + second) / 2, bit for
bit the recurrence's terms).

Tolerance.  t and the counts are exact.  The three implementations add the SAME fp64 terms in
different orders, so each S and Q word must agree within 2 n u sum |term| (u = 2^-53, n the word's
term count = its level's block count); the ceiling that would still be explicable is
4 n u sum |term|.  The waiting blocks ``pend`` come from the same elementwise operations in the
same order and must be equal bit for bit.

Shapes: B = 1 (partial wave), 63, 64 (exact wave), 257 (a second chunk with one chain), 1000
(several chunks, a partial last one); K = 1, 3, 8; T = 21 = 0b10101 samples (cascades reach level
4, blocks left waiting at levels 1 and 3); L = 8, and L = 3 where the top level keeps filling.
The trace and the references of a (B, K, dtype) case are computed once and shared.
"""
import numpy as np
import pytest
import torch

from replicas_estimators import assert_words, order_bound, pair_reblock, words_of

pytestmark = pytest.mark.gpu

T = 21
DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
_TRACE, _REF = {}, {}


def _shift(K):
    return tuple(0.25 + 0.5 * i for i in range(K))


def _trace(B, K, dtype):
    """[T, K, B] float64 holding values of `dtype`, series i centred at 3 (i + 1)."""
    key = (B, K, dtype)
    if key not in _TRACE:
        x = np.random.default_rng(100 + B + K).standard_normal((T, K, B)) + 3.0 * np.arange(1, K + 1)[None, :, None]
        _TRACE[key] = x.astype(np.float32).astype(np.float64) if dtype == torch.float32 else x
    return _TRACE[key]


def _refs(B, K, dtype, L):
    """(numpy pair_reblock sums, the host accumulator) of the case."""
    key = (B, K, dtype, L)
    if key not in _REF:
        _REF[key] = (pair_reblock(_trace(B, K, dtype), _shift(K), L)[0], _feed(_trace(B, K, dtype), L, dtype, "cpu"))
    return _REF[key]


def _feed(trace, L, dtype, device, n=None):
    from aiqmc import statistics
    K = trace.shape[1]
    acc = statistics.make_blocking(nseries=K, max_levels=L, shift=_shift(K))
    x = torch.tensor(trace, dtype=dtype, device=device)
    for t in range(T if n is None else n):
        acc.update(x[t])
    if device != "cpu":
        torch.cuda.synchronize()
    return acc


@pytest.mark.parametrize("L", [8, 3])
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("B", [1, 63, 64, 257, 1000])
@DTYPES
def test_kernel_equals_the_torch_path_and_numpy(dtype, B, K, L):
    ref, host = _refs(B, K, dtype, L)
    dev = _feed(_trace(B, K, dtype), L, dtype, "cuda")
    assert dev.acc.is_cuda and dev.pend.is_cuda and not host.acc.is_cuda
    assert ref["n"].tolist() == [B * (T >> k) for k in range(L)]
    assert_words(dev, ref, T, order_bound, "kernel vs numpy")
    t, n, S, Q = words_of(host)
    as_ref = dict(ref, n=n, S=S, Q=Q)
    assert_words(dev, as_ref, T, order_bound, "kernel vs torch")
    assert torch.equal(dev.pend.cpu(), host.pend)
    np.testing.assert_array_equal(dev.acc[1:1 + K].cpu().numpy(), _shift(K))
    # the read-out runs on either state
    r_d, r_h = dev.result(K - 1), host.result(K - 1)
    np.testing.assert_allclose(r_d["mean"].numpy(), r_h["mean"].numpy(), rtol=1e-13)
    assert r_d["n_blocks"].tolist() == [B * (T >> k) for k in range(min(L, 5))]


def test_same_inputs_twice_give_identical_words():
    B, K, L = 1000, 3, 8
    tr = _trace(B, K, torch.float64)
    a, b = _feed(tr, L, torch.float64, "cuda"), _feed(tr, L, torch.float64, "cuda")
    assert torch.equal(a.acc, b.acc) and torch.equal(a.pend, b.pend)
    assert float(a.acc[0]) == T


def test_nan_reaches_exactly_its_words():
    """A NaN in series 1 of chain 100 at sample 17 = 0b10001: it enters level 0 and level 1
    (samples 16-17), waits at level 2 and completes it at sample 19, then waits at level 3.  The
    words of series 1 at levels 0-2 are non-finite; levels 3 and 4 (built from samples 0-15) and
    every word of series 0 alone keep the bits of the clean run."""
    B, K, L = 257, 2, 8
    clean = _trace(B, K, torch.float64)
    tr = clean.copy()
    tr[17, 1, 100] = np.nan
    dev, base = _feed(tr, L, torch.float64, "cuda"), _feed(clean, L, torch.float64, "cuda")
    ref = pair_reblock(tr, _shift(K), L)[0]
    t, n, S, Q = words_of(dev)
    _, n0, S0, Q0 = words_of(base)
    assert t == T
    np.testing.assert_array_equal(n, n0)
    np.testing.assert_array_equal(np.isfinite(S), np.isfinite(ref["S"]))
    np.testing.assert_array_equal(np.isfinite(Q), np.isfinite(ref["Q"]))
    hit = np.zeros(L, dtype=bool)
    hit[:3] = True
    np.testing.assert_array_equal(~np.isfinite(S[:, 1]), hit)
    np.testing.assert_array_equal(~np.isfinite(Q[:, 1]), hit)      # Q[0][1]
    np.testing.assert_array_equal(~np.isfinite(Q[:, 2]), hit)      # Q[1][1]
    np.testing.assert_array_equal(S[:, 0], S0[:, 0])
    np.testing.assert_array_equal(Q[:, 0], Q0[:, 0])
    np.testing.assert_array_equal(S[3:], S0[3:])
    np.testing.assert_array_equal(Q[3:], Q0[3:])
    pend = dev.pend.cpu().numpy()
    assert np.isnan(pend[3, 1, 100]) and np.isfinite(np.delete(pend[3].reshape(-1), 1 * B + 100)).all()


def test_update_on_a_non_default_stream():
    from aiqmc import statistics
    B, K, L = 257, 3, 8
    tr = _trace(B, K, torch.float32)
    want = _feed(tr, L, torch.float32, "cuda")
    x = torch.tensor(tr, dtype=torch.float32, device="cuda")
    acc = statistics.make_blocking(nseries=K, max_levels=L, shift=_shift(K))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for t in range(T):
            acc.update(x[t])
    side.synchronize()
    assert torch.equal(acc.acc, want.acc) and torch.equal(acc.pend, want.pend)


def test_state_dict_resumes_on_the_device_bit_for_bit():
    from aiqmc import statistics
    B, K, L = 257, 3, 8
    tr = _trace(B, K, torch.float64)
    whole = _feed(tr, L, torch.float64, "cuda")
    first = _feed(tr, L, torch.float64, "cuda", n=13)
    sd = first.state_dict()
    assert not sd["acc"].is_cuda and not sd["pend"].is_cuda
    resumed = statistics.make_blocking(nseries=K, max_levels=L)
    resumed.load_state_dict(sd)
    x = torch.tensor(tr, dtype=torch.float64, device="cuda")
    for t in range(13, T):
        resumed.update(x[t])
    assert resumed.acc.is_cuda and torch.equal(resumed.acc, whole.acc) and torch.equal(resumed.pend, whole.pend)


def test_n2_local_energies_fed_per_iteration():
    """8 N2 walkers, 8 iterations of mc_step followed by local_energy, each fed as it is produced:
    the level-0 sum is the sum of the stored trace (64 terms, two orders) and the counts follow."""
    from aiqmc import statistics, systems
    s = systems.make_system("N2")
    net = s.make_network()
    ctx = net.apply._aiqmc_network.bind(net.init(5), s.atoms, torch.float32)
    block = np.concatenate([np.tile(s.atoms[i], int(s.charges[i])) for i in range(s.natoms)])
    pos = torch.tensor(block[None] + np.random.default_rng(11).standard_normal((8, 3 * s.nelectrons)),
                       dtype=torch.float32, device="cuda")
    acc = statistics.make_blocking(names=("E_L",))
    trace = []
    for it in range(8):
        ctx.mc_step(pos, 2, 0.05, seed=1 + it)
        el, _, _ = ctx.local_energy(pos)
        acc.update(el)
        trace.append(el.clone())
    torch.cuda.synchronize()
    x = torch.stack(trace).cpu().numpy().astype(np.float64)
    assert np.isfinite(x).all()
    t, n, S, Q = words_of(acc)
    assert t == 8 and n[:4].tolist() == [64, 32, 16, 8] and n[4:].sum() == 0
    assert abs(S[0, 0] - x.sum()) <= order_bound(64) * np.abs(x).sum()
    assert abs(Q[0, 0] - (x * x).sum()) <= order_bound(64) * (x * x).sum()
    r = acc.result("E_L")
    np.testing.assert_allclose(r["mean"][0].item(), x.mean(), rtol=1e-13)
    np.testing.assert_allclose(r["mean"][3].item(), x.mean(), rtol=1e-13)
    np.testing.assert_allclose(r["naive_stderr"], np.sqrt(x.var(ddof=1) / 64), rtol=1e-10)
