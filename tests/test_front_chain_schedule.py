"""k_ldl_front's chain workgroup prepares the LDS arrays of its diagonal block's LDL' (S cleared with the unit diagonal of a
partial block, Lc zeroed) beside the last k-steps of its diagonal tile's update instead of behind them (front_rows_diag).  The
paths that touches, on the GPU: probes at the edges of a block, blocks of fewer than 64 columns, many factorisations in a row."""
import numpy as np
import pytest
import scipy.sparse as sp

import helpers

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("m,maxu", [(640, 30.0), (736, 30.0), (752, 30.0), (752, 2.0)])
def test_probe_at_the_edges_of_a_block(refmex, m, maxu):
    """helpers.check_one_launch_pivot_rule puts the rank-deficient part from column m / 2 on: column 320 is the first sweep of
    block 5, 368 the first column of its last group, 376 the first column of its last sweep."""
    helpers.check_one_launch_pivot_rule(refmex, m, maxu)


def test_rank_deficient_fronts_second_seed(refmex):
    """40 more seeded rank-deficient fronts (probes anywhere in a block), another seed than test_gpu_parity's."""
    helpers.check_rank_deficient_fronts(refmex, 40, seed=2027)


@pytest.mark.parametrize("m", [123, 666, 700])
def test_blocks_of_fewer_than_64_columns_bit_for_bit(refmex, m):
    """a last block of 59 (m = 123), 26 (666) and 60 (700) columns: an odd number of sweeps, a last group cut short."""
    helpers.check_one_launch_front(refmex, m)


def test_fifty_factorisations_of_control07s_shape(refmex):
    """50 factorisations of m = 666 in a row, every one the bits of the first."""
    from sedumi_amd import problem
    from sedumi_amd.plan import Plan
    m = 666
    rng = np.random.default_rng(5)
    B = rng.standard_normal((m, m))
    X = sp.csc_matrix(B @ B.T + m * np.eye(m)); X.sort_indices()
    plan = Plan(0)
    plan.set_chol(problem.dense_symbolic(m), X)
    plan.upload("ada", X.data); plan.upload("rhs", rng.standard_normal(m))
    plan.blkchol(None, False); plan.ldlsolve()
    l0, d0, y0 = plan.download("lpr"), plan.download("d"), plan.download("y")
    for _ in range(50):
        plan.blkchol(None, False); plan.ldlsolve()
        assert np.array_equal(plan.download("lpr"), l0) and np.array_equal(plan.download("d"), d0) and np.array_equal(plan.download("y"), y0)
