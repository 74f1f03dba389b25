"""triumtriu (k_triumtriu, sdm_cone.hip) and the PSD chain of updtransfo.m:99-108 as one call (sdm_updtransfo_psd) -- the kernel
logic on the CPU emulator: the value against triumtriu.m:40-71 in numpy.longdouble within the bound of a dot product of that length, the mirror
bit for bit, the lower triangles of the operands ignored (NaN there), offsets and lengths, the fused call bit-equal to the six single calls, the
driver switch (tests/triu_exact.py).  The device runs of the same checks: test_triumtriu_gpu.py."""
import pytest

import helpers
import triu_exact as te


@pytest.fixture(scope="module", autouse=True)
def _emu():
    helpers.use_emu()


@pytest.mark.parametrize("complex_diag", (False, True))
@pytest.mark.parametrize("case", range(len(te.CASES)))
def test_triumtriu_is_the_longdouble_product_within_the_dot_product_bound(case, complex_diag):
    te.check_case(te.CASES[case], complex_diag)


def test_triumtriu_block_alone_gives_the_bits_it_has_in_a_list():
    te.check_block_alone()


def test_triumtriu_entry_points_check_before_anything_touches_a_device():
    """on the product library, with or without a device present, and on the emulated one"""
    from sedumi_amd import capi
    te.check_lengths_are_refused()
    capi.use_library(None)
    try:
        te.check_lengths_are_refused()
    finally:
        helpers.use_emu()


@pytest.mark.parametrize("case", range(len(te.CHAIN_CASES)))
def test_updtransfo_psd_is_bit_equal_to_the_six_single_calls(case):
    te.check_chain(te.CHAIN_CASES[case])


def test_updtransfo_psd_is_bit_equal_under_every_lds_budget():
    te.check_chain_under_every_budget()


def test_driver_switch_device_updt_solves_the_same():
    te.check_driver_switch()
