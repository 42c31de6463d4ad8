"""Which kernel a walker launch reaches, asked of a context (Context.launch_row ->
aiqmc_debug_launch_row: csrc/launch_route.h's route() with the context's shape, dtype and current
debug switches; it launches nothing).  The expected rows are the table of launch_route.h / shape.hip
written out: 1 k_quad_value, 2 k_quad_grad, 3 k_quad_grad<walker>, 4 k_walker<LAP>,
5 k_walker_rev<PROP>, 6 k_walker_rev<SPL>, 7 k_walker_rev, 8 k_walker<GRAD>."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KINDS = ("walker_value", "walker_orbitals", "walker_grad", "sweep_walker", "proposal", "quadrature",
         "lap_forward", "grad_forward")
# rows in KINDS order, one configuration (the sweep walker of a larger batch: _sweep_rows)
PACKED = (3, 7, 3, 3, 2, 1, 4, 8)          # N <= 8, default switches
ONE_WAVE_F32 = (7, 7, 7, 6, 5, 5, 4, 8)    # N > 8 fp32: a batch of one leaves SIMDs idle -> two waves per walker
ONE_WAVE_F64 = (7, 7, 7, 7, 5, 5, 4, 8)    # N > 8 fp64: the two-wave kernel is an fp32 instantiation


def _ctx(n, dtype):
    from aiqmc import _lib
    from oracle import system
    s = system.make_system(f"Z{n}")
    t = s.tables()
    return _lib.Context(s.nelectrons, s.natoms, s.nspins, s.atoms, s.charges, t["spin_up_indices"],
                        t["spin_down_indices"], t["parallel_indices"], t["antiparallel_indices"], dtype=dtype, device=0)


def _rows(ctx, nconf=1):
    return tuple(ctx.launch_row(k, nconf) for k in KINDS)


def _replace(rows, **by_kind):
    return tuple(by_kind.get(k, r) for k, r in zip(KINDS, rows))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [4, 5, 8, 9])
def test_launch_rows_by_kind_and_switch(n, dtype):
    ctx = _ctx(n, dtype)
    f32 = dtype == torch.float32
    big = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 1   # past the split's batch condition
    default = PACKED if n <= 8 else (ONE_WAVE_F32 if f32 else ONE_WAVE_F64)
    default_big = default if n <= 8 else ONE_WAVE_F64   # a large batch: one wave per walker, row 7
    assert _rows(ctx) == default
    assert _rows(ctx, big) == default_big

    ctx.set_packed_walkers(False)   # N <= 8 walker kinds leave row 3; sweep walkers of a small fp32 batch split
    unpacked = default if n > 8 else _replace(default, walker_value=7, walker_grad=7, sweep_walker=6 if f32 else 7)
    unpacked_big = default_big if n > 8 else _replace(default, walker_value=7, walker_grad=7, sweep_walker=7)
    assert _rows(ctx) == unpacked
    assert _rows(ctx, big) == unpacked_big
    ctx.set_packed_walkers(True)
    assert _rows(ctx) == default
    assert _rows(ctx, big) == default_big

    ctx.set_proposal_reuse(False)   # no ecache: proposals and quadrature values from scratch, row 7
    assert _rows(ctx) == _replace(default, proposal=7, quadrature=7)
    assert _rows(ctx, big) == _replace(default_big, proposal=7, quadrature=7)
    ctx.set_proposal_reuse(True)
    assert _rows(ctx) == default
    assert _rows(ctx, big) == default_big


def test_launch_row_rejects_an_unknown_kind():
    ctx = _ctx(4, torch.float32)
    with pytest.raises(RuntimeError):
        ctx.launch_row(8, 1)
    with pytest.raises(RuntimeError):
        ctx.launch_row(-1, 1)
