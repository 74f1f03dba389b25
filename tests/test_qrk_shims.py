"""the qrK mexFunction shim (sedumi_amd/mexshims) against the reference gateway, linked to the emulated build of the C ABI and
driven through the same mxArray marshalling as the reference MEX (tests/test_mexshims.py's way); the same on the hipcc library:
test_qrk_gpu.py."""
import os

import numpy as np
import pytest

from helpers import ROOT
import qrk_exact as qe


@pytest.fixture(scope="module")
def shimmex(refmex):
    import sys
    from test_mexshims import build_shims
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
    import build_emu
    return build_shims(build_emu.build(), os.path.join(ROOT, "tests", "hipemu", "_mexshims"))


def check_shims(refmex, shimmex):
    from oracle.refmex import RefMexError
    c = qe.make_case(refmex, dict(s=[6, 40], hs=[5]), 21)
    K = c["K"]
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)
    q, r = shimmex.call("qrK", 2, col(c["x"]), K)
    q, r = np.asarray(q), np.asarray(r)
    assert q.shape == (c["qref"].size, 1) and r.shape == (c["x"].size, 1)
    qe.check_rule("qrK shim", qe.parts(q.ravel(), r.ravel(), K), c)
    qe.check_backward(q.ravel(), r.ravel(), c)
    q1 = np.asarray(shimmex.call("qrK", 1, col(c["x"]), K))
    assert np.array_equal(q1, q)                                        # q alone
    with pytest.raises(RefMexError, match="size mismatch x"):
        shimmex.call("qrK", 2, col(c["x"][:-1]), K)


def test_qrk_shim_matches_the_reference_gateway(refmex, shimmex):
    from sedumi_amd.build import SHIMS
    assert "qrK" in SHIMS
    check_shims(refmex, shimmex)
