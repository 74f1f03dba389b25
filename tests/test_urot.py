"""urotorder, givensrot, sqrtinv (sdm_rot.hip) -- the kernel logic on the CPU emulator against the compiled reference (oracle/_ref)
on ADMITTED cases (tests/urot_exact.py): perm and gjc equal to the reference's; g, triu(u), givensrot's and the chain's outputs by the accuracy
rule of DESIGN 7c with the reference's algorithm in numpy.longdouble, on the reference's decisions, as `exact`; the structure of the outputs, the
invariants, repeatable bits, a block alone, the residences of the working copy; the checks of the C ABI; the driver switch.  The device runs of
the same checks: test_urot_gpu.py."""
import numpy as np
import pytest

import helpers
import urot_exact as ue


@pytest.fixture(scope="module", autouse=True)
def _emu():
    helpers.use_emu()


@pytest.mark.parametrize("case", range(len(ue.CASES)))
def test_urot_chain_matches_reference_on_admitted_cases(refmex, case):
    ue.check_case(refmex, ue.CASES[case], seed=ue.seed_of(case))


def test_urot_case_with_more_rotations_than_a_chunk(refmex):
    """the order-300 case has a step whose rotations take more than one chunk of 256 (the carry between chunks)"""
    i = ue.CASES.index(dict(s=[300]))
    c = ue.make_case(refmex, ue.CASES[i], ue.seed_of(i))
    assert np.diff(c["gjc"]).max() > 256


def test_graded_cases_recompute_d_more_than_once(refmex):
    """the graded inputs are what reaches the d-recompute branch after step 0 (every other input recomputes once, at step 0)"""
    for i, kw in enumerate(ue.CASES):
        c = ue.make_case(refmex, kw, ue.seed_of(i))
        if kw.get("graded"):
            assert all(len(rc) > 1 and rc[0] == 0 for rc in c["recomp"]), c["recomp"]


def test_urot_block_alone_gives_the_bits_it_has_in_a_list(refmex):
    ue.check_block_alone(refmex)


def test_urot_residences_give_the_same_bits(refmex):
    ue.check_residences(refmex)


def test_urot_entry_points_check_before_anything_touches_a_device():
    """On the product library, with or without a device present: wrong lengths, a gjc that decreases or overflows its rows, a g shorter than gjc says,
    a wrong vlab length and a negative budget are refused, and a cone without PSD blocks returns empty arrays -- all before any allocation."""
    import ctypes as C
    from sedumi_amd import capi, mex, problem
    from sedumi_amd.capi import SdmError
    capi.use_library(None)
    try:
        K = problem.make_K(1, [], [4])
        with pytest.raises(SdmError, match="u size mismatch"):
            mex.urotorder(np.ones(15), K, 1.1)
        with pytest.raises(SdmError, match="perm size mismatch"):
            mex.urotorder(np.ones(16), K, 1.1, np.ones(3))
        with pytest.raises(SdmError, match="not a number"):
            mex.urotorder(np.ones(16), K, np.nan)
        with pytest.raises(SdmError, match="x size mismatch"):
            mex.givensrot(np.zeros(4), np.zeros(0), np.ones(15), K)
        with pytest.raises(SdmError, match="g size mismatch"):
            mex.givensrot(np.array([0.0, 1, 2, 3]), np.ones(5), np.ones(16), K)
        with pytest.raises(SdmError, match="rotation count per step"):
            mex.givensrot(np.array([0.0, 2, 1, 3]), np.ones(6), np.ones(16), K)           # decreasing
        with pytest.raises(SdmError, match="rotation count per step"):
            mex.givensrot(np.array([0.0, 0, 0, 2]), np.ones(6), np.ones(16), K)           # step 2 has one row below it, not two
        with pytest.raises(SdmError, match="gjc out of range"):
            mex.givensrot(np.array([0.0, -1, 0, 0]), np.ones(6), np.ones(16), K)
        with pytest.raises(SdmError, match="v size mismatch"):
            mex.sqrtinv(np.ones(16), np.ones(3), K)
        Kc, keep = capi.make_cone(1, [], [4], 1)
        one = np.ones(16)
        assert capi.lib().sdm_urotorder(C.byref(Kc), capi.pf(one), C.c_double(1.1), None, capi.pf(one), capi.pf(one), capi.pf(one), capi.pf(one), None) != 0
        assert b"null argument" in capi.lib().sdm_last_error()
        with pytest.raises(SdmError):
            mex.set_rot_lds_budget(-1)
        K0 = problem.make_K(3, [3], [])
        u, p, gjc, g = mex.urotorder(np.zeros(0), K0, 1.1)
        assert u.size == 0 and p.size == 0 and gjc.size == 0 and g.shape == (0, 1)
        assert mex.givensrot(np.zeros(0), np.zeros(0), np.zeros(0), K0).size == 0
        assert mex.sqrtinv(np.zeros(0), np.ones(3 + 2), K0).size == 0
    finally:
        helpers.use_emu()


def test_driver_switch_device_rot_solves_the_same():
    ue.check_driver_switch()
