"""psdjmul (k_psdjmul, sdm_cone.hip) and the PSD parts of maxstep.m:63 and of widelen.m:101-104 / trydif.m:62-64 as one call each
(sdm_maxstep_psd, sdm_wstruct_psd) -- the kernel logic on the CPU emulator: the value against psdjmul.m:40-73 in numpy.longdouble within the bound of
a sum of that many products, the symmetry and Im diag bit for bit, the exact case against the identity, offsets, lengths and isolation of the blocks,
the fused calls bit-equal to the single calls they replace, the driver switches (tests/psdjmul_exact.py).  The device runs of the same checks:
test_psdjmul_gpu.py."""
import pytest

import helpers
import psdjmul_exact as je


@pytest.fixture(scope="module", autouse=True)
def _emu():
    helpers.use_emu()


@pytest.mark.parametrize("case", range(len(je.CASES)))
def test_psdjmul_is_the_longdouble_product_within_the_sum_bound(case):
    je.check_case(je.CASES[case])


def test_psdjmul_block_alone_gives_the_bits_it_has_in_a_list():
    je.check_block_alone()


def test_psdjmul_nan_in_one_block_leaves_the_others_alone():
    je.check_nan_block_in_a_list()


def test_psdjmul_entry_points_check_before_anything_touches_a_device():
    """on the product library, with or without a device present, and on the emulated one"""
    from sedumi_amd import capi
    je.check_lengths_are_refused()
    capi.use_library(None)
    try:
        je.check_lengths_are_refused()
    finally:
        helpers.use_emu()


@pytest.mark.parametrize("case", range(len(je.FUSED_CASES)))
def test_maxstep_psd_is_bit_equal_to_the_two_single_calls(case):
    je.check_maxstep(je.FUSED_CASES[case])


def test_maxstep_psd_names_the_block_with_a_nan():
    je.check_maxstep_nan_block()


@pytest.mark.parametrize("case", range(len(je.FUSED_CASES)))
def test_wstruct_psd_is_bit_equal_to_the_two_single_calls(case):
    je.check_wstruct(je.FUSED_CASES[case])


def test_wstruct_psd_with_a_block_that_is_not_positive_definite():
    je.check_wstruct_bad_block()


def test_driver_switches_device_jmul_and_device_step_solve_the_same():
    je.check_driver_switches()
