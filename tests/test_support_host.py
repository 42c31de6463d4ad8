"""tests/support.py itself, on the CPU: the names, the seeded inputs byte for byte against the three
calls they stand for, the oracle cache, and the rank runner's two outcomes."""
import os
import time

import numpy as np
import pytest

import support


@pytest.mark.parametrize("shape,name", [((2, 1), "Z2"), ((5, 2), "Z3-2"), ((13, 3), "Z5-4-4"), ((10, 4), "Z3-3-2-2")])
def test_z_name(shape, name):
    assert support.z_name(*shape) == name


def _bytes(params, pos):
    from oracle import system
    return system.flatten_params(params).tobytes(), pos.tobytes()


def test_seeded_case_is_the_three_calls():
    from oracle import system
    s = system.make_system("Z2")
    rng = np.random.default_rng(107)
    params = system.init_params(rng, s, randomize_aux=True)
    pos = system.init_electrons(rng, s.atoms, s.charges, 4, 1.0)
    s1, p1, x1 = support.seeded_case("Z2", 107)
    s2, p2, x2 = support.seeded_case("Z2", 107)
    assert (s1.nelectrons, s1.natoms) == (2, 1) and x1.shape == (4, 6) and x1.dtype == np.float64
    assert _bytes(p1, x1) == _bytes(params, pos)
    assert _bytes(p2, x2) == _bytes(params, pos)


def test_oracle_case_is_cached():
    a = support.oracle_case("Z2", 107)
    assert support.oracle_case("Z2", 107) is a
    assert _bytes(a[1], a[2]) == _bytes(*support.seeded_case("Z2", 107)[1:])
    assert [v.shape for v in a[3:]] == [(4,), (4,), (4, 6)]


_OK = "import os; assert os.environ['MASTER_ADDR'] == '127.0.0.1' and int(os.environ['WORLD_SIZE']) == 2"
# rank 1 exits 3; rank 0 writes its pid and would outlive the test
_FAIL = r'''
import os, sys, time
if os.environ["RANK"] == "1":
    while not (os.path.exists(sys.argv[1]) and open(sys.argv[1]).read()):
        time.sleep(0.01)
    sys.exit(3)
open(sys.argv[1], "w").write(str(os.getpid()))
time.sleep(120)
'''


def test_run_ranks_returns_every_exit_code():
    assert support.run_ranks(_OK, 2, [], timeout=60) == [0, 0]


def test_run_ranks_reports_a_failure_and_leaves_no_child(tmp_path):
    pidfile = tmp_path / "pid"
    t0 = time.monotonic()
    codes = support.run_ranks(_FAIL, 2, [str(pidfile)], timeout=60)
    assert codes[1] == 3 and codes[0] not in (0, None), codes
    assert time.monotonic() - t0 < 30
    with pytest.raises(ProcessLookupError):     # reaped by run_ranks: the pid is gone
        os.kill(int(pidfile.read_text()), 0)
