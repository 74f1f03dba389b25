"""SURVEY 8f N8 on the device: the checks of test_triumtriu.py / test_triumtriu_shims.py on the hipcc-built library, plus the shape that only the
device runs (three real blocks of order 200 and a Hermitian one of order 130)."""
import os

import pytest

from helpers import ROOT, use_hip
import triu_exact as te

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _hip():
    use_hip()


@pytest.mark.parametrize("complex_diag", (False, True))
@pytest.mark.parametrize("case", range(len(te.CASES)))
def test_triumtriu_is_the_longdouble_product_within_the_dot_product_bound_on_the_gpu(case, complex_diag):
    te.check_case(te.CASES[case], complex_diag)


@pytest.mark.parametrize("complex_diag", (False, True))
def test_triumtriu_of_several_larger_blocks_on_the_gpu(complex_diag):
    te.check_case(te.GPU_ONLY_CASE, complex_diag)


def test_triumtriu_block_alone_gives_the_bits_it_has_in_a_list_on_the_gpu():
    te.check_block_alone()


def test_triumtriu_entry_points_refuse_wrong_lengths_on_the_gpu():
    te.check_lengths_are_refused()


@pytest.mark.parametrize("case", range(len(te.CHAIN_CASES)))
def test_updtransfo_psd_is_bit_equal_to_the_six_single_calls_on_the_gpu(case):
    te.check_chain(te.CHAIN_CASES[case], full=True)


def test_updtransfo_psd_of_several_larger_blocks_on_the_gpu():
    te.check_chain(te.GPU_ONLY_CASE, full=True)


def test_updtransfo_psd_is_bit_equal_under_every_lds_budget_on_the_gpu():
    te.check_chain_under_every_budget()


def test_triumtriu_shim_matches_the_library_on_the_gpu(refmex):
    from sedumi_amd import capi
    from test_mexshims import build_shims
    from test_triumtriu_shims import check_shim
    check_shim(build_shims(capi.DEFAULT_LIB, os.path.join(ROOT, "tests", "hipemu", "_mexshims_hip")))


def test_driver_switch_device_updt_solves_the_same_on_the_gpu():
    te.check_driver_switch()
