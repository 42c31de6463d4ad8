"""The pure pieces of the prologue the drop-in closures share, without a GPU: nn.as_positions /
kernel_dtype / network_of and VMCmcstep.philox_key."""
import numpy as np
import pytest
import torch


def test_positions_and_kernel_dtype():
    from aiqmc.wavefunction_Ynlm import nn
    t64 = torch.zeros(2, 6, dtype=torch.float64)
    assert nn.as_positions(t64) is t64 and nn.kernel_dtype(t64) == torch.float64
    a32 = nn.as_positions(np.zeros((2, 6), dtype=np.float32))
    assert isinstance(a32, torch.Tensor) and a32.dtype == torch.float32 and nn.kernel_dtype(a32) == torch.float32
    ints = nn.as_positions([[0, 1, 2, 3, 4, 5]])
    assert not ints.dtype.is_floating_point and nn.kernel_dtype(ints) == torch.float32


def test_network_of_names_the_caller_and_follows_the_tag():
    from aiqmc import systems
    from aiqmc.Energy import hamiltonian
    from aiqmc.wavefunction_Ynlm import nn
    with pytest.raises(TypeError, match="some_factory"):
        nn.network_of(lambda *a: None, "some_factory")
    assert nn.network_of(lambda *a: None, None) is None
    s = systems.make_system("C_ecp")
    network = s.make_network()
    ain = nn.network_of(network.apply, "test")
    assert isinstance(ain, nn.AINet)
    assert nn.network_of(nn.make_log_network(network.apply), "test") is ain
    assert nn.network_of(hamiltonian.local_energy(network.apply, s.charges, s.nspins), "test") is ain
    assert hamiltonian.network_of is nn.network_of


def test_philox_key():
    from aiqmc.VMC.VMCmcstep import PhiloxKey, philox_key
    assert philox_key(7) == PhiloxKey(7, 0)
    k = PhiloxKey(3, 9)
    assert philox_key(k) is k
    with pytest.raises(TypeError):
        philox_key(None)


def test_every_submodule_imports_and_branch_uses_the_lookup():
    import importlib
    import pkgutil
    import aiqmc
    names = [m.name for m in pkgutil.walk_packages(aiqmc.__path__, "aiqmc.")
             if not m.name.rsplit(".", 1)[1].startswith("libaiqmc_hip")]   # the HIP library is no Python module
    assert "aiqmc.DMC.branch" in names
    for name in names:
        importlib.import_module(name)
    from aiqmc.DMC import branch
    w = torch.ones(4)
    with pytest.raises(TypeError, match="branch needs the aiqmc network"):
        branch.branch(None, w, 0.5)
    with pytest.raises(TypeError, match="branch"):
        branch.branch(None, w, 0.5, network=lambda *a: None)
