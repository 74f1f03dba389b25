"""psdeig and minpsdeig (sdm_psdeig.hip), the block Jacobi eigensolver over all PSD blocks -- the kernel logic on the CPU emulator:
the three residuals of the decomposition in numpy.longdouble against those of LAPACK on the same input, the +-lambda spectra a sign-based Hestenes
gets wrong, lab ascending, the values-only call and the minimum bit for bit, a diagonal block's permutation, offsets and lengths, a block with a
NaN in a list, the driver switch (tests/psdeig_exact.py).  The device runs of the same checks: test_psdeig_gpu.py."""
import pytest

import helpers
import psdeig_exact as pe


@pytest.fixture(scope="module", autouse=True)
def _emu():
    helpers.use_emu()


@pytest.mark.parametrize("spectrum", pe.SPECTRA)
@pytest.mark.parametrize("case", range(len(pe.CASES)))
def test_psdeig_residuals_stay_within_a_multiple_of_lapacks(case, spectrum):
    pe.check_case(pe.CASES[case], spectrum)


def test_psdeig_of_zero_one_one_zero():
    pe.check_zero_one()


def test_psdeig_of_a_diagonal_block_is_the_sorting_permutation():
    pe.check_diagonal()


def test_psdeig_does_not_read_the_imaginary_diagonal():
    pe.check_imag_diagonal_ignored()


def test_psdeig_block_alone_gives_the_bits_it_has_in_a_list():
    pe.check_block_alone()


def test_psdeig_entry_points_check_before_anything_touches_a_device():
    """on the product library, with or without a device present, and on the emulated one"""
    from sedumi_amd import capi
    pe.check_lengths_are_refused()
    capi.use_library(None)
    try:
        pe.check_lengths_are_refused()
    finally:
        helpers.use_emu()


def test_psdeig_marks_a_block_with_a_nan_and_leaves_the_others_alone():
    pe.check_nan_block_in_a_list()


def test_driver_switch_device_eig_solves_the_same():
    pe.check_driver_switch()
