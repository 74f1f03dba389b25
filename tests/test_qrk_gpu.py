"""SURVEY 8f N6 on the device: the checks of test_qrk.py / test_qrk_shims.py on the hipcc-built library, every case in full, plus the shape
that only the device runs (three real blocks of order 200 and a Hermitian one of order 130)."""
import os

import pytest

from helpers import ROOT, use_hip
import qrk_exact as qe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _hip():
    use_hip()


@pytest.mark.parametrize("case", range(len(qe.CASES)))
def test_qrk_matches_reference_by_the_accuracy_rule_on_the_gpu(refmex, case):
    qe.check_case(refmex, qe.CASES[case], seed=case, full=True)


def test_qrk_of_several_larger_blocks_on_the_gpu(refmex):
    qe.check_case(refmex, qe.GPU_ONLY_CASE, seed=qe.GPU_ONLY_SEED, full=True)


def test_qrk_block_alone_gives_the_bits_it_has_in_a_list_on_the_gpu(refmex):
    qe.check_block_alone(refmex)


def test_qrk_panel_residences_give_the_same_bits_on_the_gpu(refmex):
    qe.check_residences(refmex)


def test_qrk_shim_matches_the_reference_gateway_on_the_gpu(refmex):
    from sedumi_amd import capi
    from test_mexshims import build_shims
    from test_qrk_shims import check_shims
    check_shims(refmex, build_shims(capi.DEFAULT_LIB, os.path.join(ROOT, "tests", "hipemu", "_mexshims_hip")))


def test_driver_switch_device_qr_solves_the_same_on_the_gpu():
    qe.check_driver_switch()
