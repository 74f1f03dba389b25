"""qrK as a blocked Householder QR (sdm_qrk.hip) -- the kernel logic on the CPU emulator against the compiled reference
(oracle/_ref) by the accuracy rule of DESIGN 7c, with the reference's own algorithm in numpy.longdouble as `exact` (tests/qrk_exact.py); the
backward checks, the structure of the outputs, the explicit kind, repeatable bits, the panel's residences, the chain into psdframeit; the
size checks of the C ABI; the driver switch.  The device runs of the same checks: test_qrk_gpu.py."""
import numpy as np
import pytest

import helpers
import qrk_exact as qe


@pytest.fixture(scope="module", autouse=True)
def _emu():
    helpers.use_emu()


@pytest.mark.parametrize("case", range(len(qe.CASES)))
def test_qrk_matches_reference_by_the_accuracy_rule(refmex, case):
    qe.check_case(refmex, qe.CASES[case], seed=case)


def test_qrk_block_alone_gives_the_bits_it_has_in_a_list(refmex):
    qe.check_block_alone(refmex)


def test_qrk_panel_residences_give_the_same_bits(refmex):
    qe.check_residences(refmex)


def test_qrk_size_checks_launch_nothing():
    """On the product library, with or without a device present: a wrong frame_kind, a wrong length of x and a negative budget are refused
    and a cone without PSD blocks returns empty arrays -- all before anything touches a device."""
    import ctypes as C
    from sedumi_amd import capi, mex, problem
    from sedumi_amd.capi import SdmError
    capi.use_library(None)
    try:
        K = problem.make_K(1, [], [4])
        with pytest.raises(SdmError, match="frame_kind"):
            mex.qrK(np.ones(16), K, frame_kind=2)
        Kc, keep = capi.make_cone(1, [], [4], 1)
        one = np.ones(16)
        assert capi.lib().sdm_qrk(C.byref(Kc), capi.pf(one), C.c_int(7), capi.pf(one), None) != 0
        assert b"frame_kind" in capi.lib().sdm_last_error()
        with pytest.raises(SdmError, match="size mismatch x"):
            mex.qrK(np.ones(15), K)
        with pytest.raises(SdmError):
            mex.set_qr_panel_lds_budget(-1)
        K0 = problem.make_K(3, [3], [])
        assert mex.qrK(np.zeros(0), K0).size == 0
        q, r = mex.qrK(np.zeros(0), K0, nlhs=2, frame_kind=mex.FRAME_EXPLICIT)
        assert q.size == 0 and r.size == 0
    finally:
        helpers.use_emu()


def test_driver_switch_device_qr_solves_the_same():
    qe.check_driver_switch()
