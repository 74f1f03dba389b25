"""SURVEY 8f N7 on the device: the checks of test_urot.py / test_urot_shims.py on the hipcc-built library, every case in full, plus the shape that
only the device runs (three real blocks of order 200 and a Hermitian one of order 130)."""
import os

import pytest

from helpers import ROOT, use_hip
import urot_exact as ue

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _hip():
    use_hip()


@pytest.mark.parametrize("case", range(len(ue.CASES)))
def test_urot_chain_matches_reference_on_admitted_cases_on_the_gpu(refmex, case):
    ue.check_case(refmex, ue.CASES[case], seed=ue.seed_of(case), full=True)


def test_urot_chain_of_several_larger_blocks_on_the_gpu(refmex):
    ue.check_case(refmex, ue.GPU_ONLY_CASE, seed=ue.GPU_ONLY_SEED, full=True)


def test_urot_block_alone_gives_the_bits_it_has_in_a_list_on_the_gpu(refmex):
    ue.check_block_alone(refmex)


def test_urot_residences_give_the_same_bits_on_the_gpu(refmex):
    ue.check_residences(refmex)


def test_urot_shims_match_the_reference_gateways_on_the_gpu(refmex):
    from sedumi_amd import capi
    from test_mexshims import build_shims
    from test_urot_shims import check_shims
    check_shims(refmex, build_shims(capi.DEFAULT_LIB, os.path.join(ROOT, "tests", "hipemu", "_mexshims_hip")))


def test_driver_switch_device_rot_solves_the_same_on_the_gpu():
    ue.check_driver_switch()
