"""SURVEY 8f N11 on the device: the checks of test_psdjmul.py / test_psdjmul_shims.py on the hipcc-built library, plus the shape that only the
device runs (three real blocks of order 200 and a Hermitian one of order 130)."""
import os

import pytest

from helpers import ROOT, use_hip
import psdjmul_exact as je

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _hip():
    use_hip()


@pytest.mark.parametrize("case", range(len(je.CASES)))
def test_psdjmul_is_the_longdouble_product_within_the_sum_bound_on_the_gpu(case):
    je.check_case(je.CASES[case])


def test_psdjmul_of_several_larger_blocks_on_the_gpu():
    je.check_case(je.GPU_ONLY_CASE)


def test_psdjmul_block_alone_gives_the_bits_it_has_in_a_list_on_the_gpu():
    je.check_block_alone()


def test_psdjmul_nan_in_one_block_leaves_the_others_alone_on_the_gpu():
    je.check_nan_block_in_a_list()


def test_psdjmul_entry_points_refuse_wrong_lengths_on_the_gpu():
    je.check_lengths_are_refused()


@pytest.mark.parametrize("case", range(len(je.FUSED_CASES)))
def test_maxstep_psd_is_bit_equal_to_the_two_single_calls_on_the_gpu(case):
    je.check_maxstep(je.FUSED_CASES[case])


def test_maxstep_psd_of_several_larger_blocks_on_the_gpu():
    je.check_maxstep(je.GPU_ONLY_CASE)


def test_maxstep_psd_names_the_block_with_a_nan_on_the_gpu():
    je.check_maxstep_nan_block()


@pytest.mark.parametrize("case", range(len(je.FUSED_CASES)))
def test_wstruct_psd_is_bit_equal_to_the_two_single_calls_on_the_gpu(case):
    je.check_wstruct(je.FUSED_CASES[case])


def test_wstruct_psd_of_several_larger_blocks_on_the_gpu():
    je.check_wstruct(je.GPU_ONLY_CASE)


def test_wstruct_psd_with_a_block_that_is_not_positive_definite_on_the_gpu():
    je.check_wstruct_bad_block()


def test_psdjmul_shim_matches_the_library_on_the_gpu(refmex):
    from sedumi_amd import capi
    from test_mexshims import build_shims
    from test_psdjmul_shims import check_shim
    check_shim(build_shims(capi.DEFAULT_LIB, os.path.join(ROOT, "tests", "hipemu", "_mexshims_hip")))


def test_driver_switches_device_jmul_and_device_step_solve_the_same_on_the_gpu():
    je.check_driver_switches()
