"""k_ldl_front's chain workgroup clears S / Lc of its LDL' beside the last k-steps of its diagonal tile's update, one barrier
earlier than before (front_rows_diag): one launch against the phased launches with every workgroup a process of its own
(tests/hipemu: emu_launch_concurrent) and the work-items in both orders (a missing barrier shows as a different result)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import helpers


@pytest.fixture()
def concurrent_emu():
    helpers.use_emu()
    from hipemu import build_emu
    lib = ctypes.CDLL(build_emu.build())
    lib._Z18emu_set_concurrenti(1)
    yield lib
    lib._Z18emu_set_concurrenti(0)


def _run(m, seed, lib, concurrent):
    from sedumi_amd import problem
    from sedumi_amd.plan import Plan
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((m, m))
    X = sp.csc_matrix(B @ B.T + m * np.eye(m)); X.sort_indices()
    lib._Z18emu_set_concurrenti(int(concurrent))
    plan = Plan(0)
    plan.set_one_launch_fronts(True)
    plan.set_chol(problem.dense_symbolic(m), X)
    plan.upload("ada", X.data); plan.upload("rhs", rng.standard_normal(m))
    plan.kprof(True)
    plan.blkchol(None, False); plan.ldlsolve()
    names = set(plan.kprof_summary().keys())
    plan.kprof(False)
    assert "k_ldl_front" in names and "k_ldl_panel" not in names
    return plan.download("lpr"), plan.download("d"), plan.download("y")


@pytest.mark.parametrize("m,reverse", [(200, 0), (200, 1), (123, 1)])
def test_chain_workgroup_lds_setup_as_concurrent_workgroups(concurrent_emu, m, reverse):
    """m = 200: a last block of 8 columns (one sweep); 123: of 59 (an odd number of sweeps).  One launch against the phased
    launches, bit for bit; reverse: the work-items of every workgroup in descending order."""
    concurrent_emu._Z15emu_set_reversei(reverse)
    try:
        one = _run(m, 3, concurrent_emu, True)
        phased = _run(m, 3, concurrent_emu, False)
    finally:
        concurrent_emu._Z15emu_set_reversei(0)
    for a, b in zip(one, phased):
        assert np.array_equal(a, b)
