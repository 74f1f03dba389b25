"""SURVEY 8f N9 on the device: the checks of test_psdfact.py / test_psdfact_shims.py on the hipcc-built library, plus the shape that only the
device runs (three real blocks of order 200 and a Hermitian one of order 130)."""
import os

import pytest

from helpers import ROOT, use_hip
import psdfact_exact as pe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _hip():
    use_hip()


@pytest.mark.parametrize("spectrum", pe.SPECTRA)
@pytest.mark.parametrize("case", range(len(pe.CASES)))
def test_psdfactor_psdinvscale_psdscale_stay_inside_the_backward_error_bounds_on_the_gpu(case, spectrum):
    pe.check_case(pe.CASES[case], spectrum)


@pytest.mark.parametrize("spectrum", pe.SPECTRA)
def test_psdfact_of_several_larger_blocks_on_the_gpu(spectrum):
    pe.check_case(pe.GPU_ONLY_CASE, spectrum)


def test_psdfact_block_alone_gives_the_bits_it_has_in_a_list_on_the_gpu():
    pe.check_block_alone()


def test_psdfact_entry_points_refuse_wrong_lengths_on_the_gpu():
    pe.check_lengths_are_refused()


@pytest.mark.parametrize("p", pe.BAD_P)
def test_psdfactor_says_not_positive_definite_and_returns_zeros_on_the_gpu(p):
    pe.check_not_positive_definite(dict(s=[129]), p)


def test_psdfactor_says_not_positive_definite_on_a_hermitian_block_on_the_gpu():
    pe.check_not_positive_definite(dict(hs=[65]), 64)


def test_psdfactor_keeps_the_blocks_before_a_bad_one_and_zeroes_the_rest_on_the_gpu():
    pe.check_bad_block_in_a_list()


def test_psdfact_shims_match_the_library_on_the_gpu(refmex):
    from sedumi_amd import capi
    from test_mexshims import build_shims
    from test_psdfact_shims import check_shims
    check_shims(build_shims(capi.DEFAULT_LIB, os.path.join(ROOT, "tests", "hipemu", "_mexshims_hip")))


def test_driver_switch_device_fact_solves_the_same_on_the_gpu():
    pe.check_driver_switch()
