"""SURVEY 8f N10 on the device: the checks of test_psdeig.py / test_psdeig_shims.py on the hipcc-built library, plus the shape that only the device
runs (three real blocks of order 200 and a Hermitian one of order 130)."""
import os

import pytest

from helpers import ROOT, use_hip
import psdeig_exact as pe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _hip():
    use_hip()


@pytest.mark.parametrize("spectrum", pe.SPECTRA)
@pytest.mark.parametrize("case", range(len(pe.CASES)))
def test_psdeig_residuals_stay_within_a_multiple_of_lapacks_on_the_gpu(case, spectrum):
    pe.check_case(pe.CASES[case], spectrum)


@pytest.mark.parametrize("spectrum", pe.SPECTRA)
def test_psdeig_of_several_larger_blocks_on_the_gpu(spectrum):
    pe.check_case(pe.GPU_ONLY_CASE, spectrum)


def test_psdeig_of_zero_one_one_zero_on_the_gpu():
    pe.check_zero_one()


def test_psdeig_of_a_diagonal_block_is_the_sorting_permutation_on_the_gpu():
    pe.check_diagonal()


def test_psdeig_does_not_read_the_imaginary_diagonal_on_the_gpu():
    pe.check_imag_diagonal_ignored()


def test_psdeig_block_alone_gives_the_bits_it_has_in_a_list_on_the_gpu():
    pe.check_block_alone()


def test_psdeig_entry_points_refuse_wrong_lengths_on_the_gpu():
    pe.check_lengths_are_refused()


def test_psdeig_marks_a_block_with_a_nan_and_leaves_the_others_alone_on_the_gpu():
    pe.check_nan_block_in_a_list()


def test_psdeig_shims_match_the_library_on_the_gpu(refmex):
    from sedumi_amd import capi
    from test_mexshims import build_shims
    from test_psdeig_shims import check_shims
    check_shims(build_shims(capi.DEFAULT_LIB, os.path.join(ROOT, "tests", "hipemu", "_mexshims_hip")))


def test_driver_switch_device_eig_solves_the_same_on_the_gpu():
    pe.check_driver_switch()
