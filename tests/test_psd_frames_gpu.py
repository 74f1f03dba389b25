"""SURVEY 8f N5 on the device: the checks of test_psd_frames.py / test_psd_frames_shims.py on the hipcc-built library, plus the shapes that
only the device runs (three real blocks of order 200 and a Hermitian one of order 130)."""
import os

import pytest

from helpers import ROOT, use_hip
import psd_frames_exact as pfe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _hip():
    use_hip()


@pytest.mark.parametrize("case", range(len(pfe.CASES)))
def test_frames_match_reference_by_the_accuracy_rule_on_the_gpu(refmex, case):
    pfe.check_case(refmex, pfe.CASES[case], seed=case, full=True)


def test_frames_of_several_larger_blocks_on_the_gpu(refmex):
    pfe.check_case(refmex, pfe.GPU_ONLY_CASE, seed=31, full=True)


def test_frame_expansion_strip_paths_give_the_same_bits_on_the_gpu(refmex):
    pfe.check_strip_paths(refmex)


def test_psd_frame_shims_match_the_reference_gateways_on_the_gpu(refmex):
    from sedumi_amd import capi
    from test_mexshims import build_shims
    from test_psd_frames_shims import check_shims
    check_shims(refmex, build_shims(capi.DEFAULT_LIB, os.path.join(ROOT, "tests", "hipemu", "_mexshims_hip")))
