"""psdfactor and psdinvscale (sdm_psdfact.hip), psdscale for a bare factor and trydif.m:62-63 as one call (sdm_trydif_psd) -- the
kernel logic on the CPU emulator: the residuals of the defining equations in numpy.longdouble within the componentwise backward error bounds, the
mirror and Im diag bit for bit, the triangles that must not be read poisoned with NaN, offsets and lengths, the decisions on blocks that are not
positive definite, the fused call bit-equal to the two single calls, the driver switch (tests/psdfact_exact.py).  The device runs of the same
checks: test_psdfact_gpu.py."""
import pytest

import helpers
import psdfact_exact as pe


@pytest.fixture(scope="module", autouse=True)
def _emu():
    helpers.use_emu()


@pytest.mark.parametrize("spectrum", pe.SPECTRA)
@pytest.mark.parametrize("case", range(len(pe.CASES)))
def test_psdfactor_psdinvscale_psdscale_stay_inside_the_backward_error_bounds(case, spectrum):
    pe.check_case(pe.CASES[case], spectrum)


def test_psdfact_block_alone_gives_the_bits_it_has_in_a_list():
    pe.check_block_alone()


def test_psdfact_entry_points_check_before_anything_touches_a_device():
    """on the product library, with or without a device present, and on the emulated one"""
    from sedumi_amd import capi
    pe.check_lengths_are_refused()
    capi.use_library(None)
    try:
        pe.check_lengths_are_refused()
    finally:
        helpers.use_emu()


@pytest.mark.parametrize("p", pe.BAD_P)
def test_psdfactor_says_not_positive_definite_and_returns_zeros(p):
    pe.check_not_positive_definite(dict(s=[129]), p)


def test_psdfactor_says_not_positive_definite_on_a_hermitian_block():
    pe.check_not_positive_definite(dict(hs=[65]), 64)


def test_psdfactor_keeps_the_blocks_before_a_bad_one_and_zeroes_the_rest():
    pe.check_bad_block_in_a_list()


def test_driver_switch_device_fact_solves_the_same():
    pe.check_driver_switch()
