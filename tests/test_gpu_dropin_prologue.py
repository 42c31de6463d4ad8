"""Only a Context knows which pseudopotential tables it holds (Context.set_ecp / ensure_ecp / ecp):
the drop-ins on top of it see a set_ecp from anywhere.  C atom with its ccECP, shape (4, 1),
3 walkers, float64, injected rotations from a seeded generator."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TABLES = ("rn_local", "local_coes", "local_exps", "rn_non_local", "non_local_coes", "non_local_exps")
B = 3


def _setup():
    """A fresh network (so fresh contexts), its parameters, the walkers, one HostRotations, the
    ccECP tables X and Y = X with one local coefficient changed."""
    from aiqmc import systems
    from aiqmc.Energy.pphamiltonian import HostRotations
    from aiqmc.wavefunction_Ynlm import nn
    s = systems.make_system("C_ecp")
    network = s.make_network()
    ain = nn.network_of(network.apply, "test")
    params = ain.init(5)
    rng = np.random.default_rng(17)
    x = torch.tensor(rng.standard_normal((B, 3 * s.nelectrons)), device="cuda")
    q, r = np.linalg.qr(rng.standard_normal((B, 3, 3)))
    rot = torch.tensor(q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :])
    e = systems.ccecp_tables("C_ecp")
    X = {k: np.array(getattr(e, k), dtype=np.float64) for k in TABLES}
    Y = {k: v.copy() for k, v in X.items()}
    Y["local_coes"][0, 1] += 0.5
    data = nn.AINetData(positions=x, spins=s.spins, atoms=s.atoms, charges=s.charges)
    return s, network, ain, params, data, HostRotations(rot), X, Y, int(e.list_l)


def _pp_local_energy(s, network, tables, list_l):
    from aiqmc.Energy import pphamiltonian
    from aiqmc.wavefunction_Ynlm import nn
    return pphamiltonian.local_energy(f=network.apply, lognetwork=nn.make_log_network(network.apply),
                                      charges=s.charges, nspins=s.nspins, natoms=s.natoms, nelectrons=s.nelectrons,
                                      ndim=3, list_l=list_l, **tables)


def test_direct_set_ecp_between_two_drop_in_calls_is_seen():
    s, network, ain, params, data, key, X, Y, list_l = _setup()
    le = _pp_local_energy(s, network, X, list_l)
    first, _ = le(params, key, data)
    ctx = ain.bind(params, s.atoms, torch.float64)
    ctx.set_ecp(*Y.values(), list_l)
    other = ctx.local_energy_ecp(data.positions, rot=key.rot)
    assert not torch.equal(other, first)          # Y does change the energies
    third, _ = le(params, key, data)
    assert torch.equal(third, first)


def test_components_without_tables_refuse_a_context_that_holds_some():
    from aiqmc import systems
    from aiqmc.Energy import components
    s, network, ain, params, data, key, X, Y, list_l = _setup()
    comps = components.make_energy_components(network.apply, s.charges, s.nspins)
    assert comps(params, None, data).shape == (8, B)
    ain.bind(params, s.atoms, torch.float64).set_ecp_tables(systems.ccecp_tables("C_ecp"))
    with pytest.raises(ValueError):
        comps(params, None, data)


def test_tmoves_keep_the_local_part():
    from aiqmc.DMC import Tmoves
    s, network, ain, params, data, key, X, Y, list_l = _setup()
    ctx = ain.bind(params, s.atoms, torch.float64)
    assert ctx.ecp is None
    assert ctx.ensure_ecp(*X.values(), list_l)
    before = ctx.ecp
    e_before = ctx.local_energy_ecp(data.positions, rot=key.rot)
    Tmoves.attach_nonlocal(ctx, s.natoms, list_l, X["rn_non_local"], X["non_local_coes"], X["non_local_exps"])
    after = ctx.ecp
    assert after.list_l == before.list_l == list_l
    assert all(getattr(after, k) is getattr(before, k) for k in TABLES)      # nothing was uploaded
    assert np.array_equal(after.local_coes, X["local_coes"].reshape(s.natoms, -1))
    assert torch.equal(ctx.local_energy_ecp(data.positions, rot=key.rot), e_before)


def test_ensure_ecp_is_idempotent_and_order_safe():
    from aiqmc import _lib
    from aiqmc.wavefunction_Ynlm import nn
    s, network, ain, params, data, key, X, Y, list_l = _setup()
    ctx = ain.bind(params, s.atoms, torch.float64)
    assert ctx.ensure_ecp(*X.values(), list_l) and not ctx.ensure_ecp(*X.values(), list_l)
    assert ctx.ensure_ecp(*Y.values(), list_l)
    assert ctx.ensure_ecp(*X.values(), list_l)
    fresh = _lib.Context.for_system(s, torch.float64)
    fresh.set_params(nn.flatten_params(params))
    fresh.set_ecp(*X.values(), list_l)
    assert torch.equal(ctx.local_energy_ecp(data.positions, rot=key.rot),
                       fresh.local_energy_ecp(data.positions, rot=key.rot))
