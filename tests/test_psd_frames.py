"""psdframeit / psdinvjmul in qrK's Householder frames (sdm_cone.hip) -- the kernel logic on the CPU emulator against the
compiled reference (oracle/_ref) by the accuracy rule of tests/driver/accuracy.py, with the formulas in numpy.longdouble as `exact`
(tests/psd_frames_exact.py); the size checks of the C ABI; the driver switch.  The device runs of the same checks: test_psd_frames_gpu.py."""
import numpy as np
import pytest

import helpers
import psd_frames_exact as pfe


@pytest.fixture(scope="module", autouse=True)
def _emu():
    helpers.use_emu()


@pytest.mark.parametrize("case", range(len(pfe.CASES)))
def test_frames_match_reference_by_the_accuracy_rule(refmex, case):
    pfe.check_case(refmex, pfe.CASES[case], seed=case)


def test_frame_expansion_strip_paths_give_the_same_bits(refmex):
    pfe.check_strip_paths(refmex)


def test_frame_size_checks_launch_nothing():
    """On the product library, with or without a device present: a wrong frame_kind is refused and a cone without PSD blocks returns empty
    arrays -- both before anything touches a device (where there is none, a launch or an allocation would fail).  Wrong lengths are refused
    by the mirror."""
    from sedumi_amd import capi, mex, problem
    from sedumi_amd.capi import SdmError
    capi.use_library(None)
    try:
        K = problem.make_K(1, [], [4])
        with pytest.raises(SdmError, match="frame_kind"):
            mex.psdframeit(np.ones(4), np.ones(16), K, frame_kind=2)
        with pytest.raises(SdmError, match="frame_kind"):
            mex.psdinvjmul(np.ones(4), np.ones(16), np.ones(16), K, frame_kind=-1)
        import ctypes as C
        Kc, keep = capi.make_cone(1, [], [4], 1)
        one = np.ones(16)
        assert capi.lib().sdm_psdframeit(C.byref(Kc), capi.pf(one), capi.pf(one), C.c_int(7), capi.pf(one)) != 0
        assert b"frame_kind" in capi.lib().sdm_last_error()
        with pytest.raises(SdmError, match="frms size mismatch"):
            mex.psdframeit(np.ones(4), np.ones(15), K)
        with pytest.raises(SdmError, match="lab size mismatch"):
            mex.psdframeit(np.ones(3), np.ones(16), K)
        with pytest.raises(SdmError, match="size y mismatch"):
            mex.psdinvjmul(np.ones(4), np.ones(16), np.ones(15), K)
        with pytest.raises(SdmError):
            mex.set_frame_lds_budget(-1)
        K0 = problem.make_K(3, [3], [])
        assert mex.psdframeit(np.zeros(0), np.zeros(0), K0).size == 0
        assert mex.psdinvjmul(np.zeros(0), np.zeros(0), np.zeros(0), K0).size == 0
        assert mex.psdframe_explicit(np.zeros(0), K0).size == 0
    finally:
        helpers.use_emu()


def test_driver_switch_device_cone_solves_the_same():
    """A small user-level SDP with a real and a Hermitian PSD block: psdframeit / psdinvjmul through the library (device_cone=True, explicit
    frames) against the numpy ones: same iteration count, objectives within test_native_driver.py's 1e-6."""
    from sedumi_amd.driver import solve
    from sedumi_amd.driver import loop as lp
    from sedumi_amd.driver.conemex import NativeMex
    assert NativeMex().device_cone is False and NativeMex(device_cone=True).device_cone is True
    r0 = solve(*pfe.small_hermitian_sdp(), hot=lp.HipHot())
    r1 = solve(*pfe.small_hermitian_sdp(), hot=lp.HipHot(), device_cone=True)
    assert r0["iter"] == r1["iter"] and r1["iter"] > 3
    assert abs(r1["cx"] - r0["cx"]) <= 1e-6 * abs(r0["cx"]) and abs(r1["by"] - r0["by"]) <= 1e-6 * abs(r0["by"])
    assert abs(r1["cx"] - r1["by"]) <= 1e-6 * (1 + abs(r1["cx"]))
