"""the psdjmul mexFunction shim (sedumi_amd/mexshims) linked to the emulated build of the C ABI and driven through the same mxArray
marshalling as the reference MEX (tests/test_mexshims.py's way): bit-equal to mex.psdjmul on the library it is linked to, [] for a cone without
PSD blocks, wrong lengths and sparse arguments refused; the same on the hipcc library: test_psdjmul_gpu.py."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import ROOT
import psdjmul_exact as je


@pytest.fixture(scope="module")
def shimmex(refmex):
    import sys
    from test_mexshims import build_shims
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
    import build_emu
    return build_shims(build_emu.build(), os.path.join(ROOT, "tests", "hipemu", "_mexshims"))


def check_shim(shimmex):
    """capi must be bound to the library the shims are linked to"""
    from oracle.refmex import RefMexError
    from sedumi_amd import mex, problem
    c = je.make_case(dict(s=[6, 40], hs=[5]))
    K = c["K"]
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)
    want = mex.psdjmul(c["x"], c["y"], K)
    z = np.asarray(shimmex.call("psdjmul", 1, col(c["x"]), col(c["y"]), K))
    assert z.shape == want.shape and np.array_equal(z, want)
    je.check_value_and_symmetry(c, z.ravel())
    zl = np.asarray(shimmex.call("psdjmul", 1, col(np.concatenate(([0.5], c["x"]))), col(np.concatenate(([0.5], c["y"]))), K))   # whole-cone length
    assert np.array_equal(zl, want)
    assert np.asarray(shimmex.call("psdjmul", 1, col(np.ones(6)), col(np.ones(6)), problem.make_K(3, [3], []))).size == 0         # K.s empty: []
    with pytest.raises(RefMexError, match="size mismatch"):
        shimmex.call("psdjmul", 1, col(c["x"][1:]), col(c["y"][1:]), K)
    with pytest.raises(RefMexError, match="size mismatch"):
        shimmex.call("psdjmul", 1, col(c["x"]), col(np.concatenate(([0.5], c["y"]))), K)
    with pytest.raises(RefMexError, match="Sparse inputs not supported"):
        shimmex.call("psdjmul", 1, sp.csc_matrix(col(c["x"])), col(c["y"]), K)
    with pytest.raises(RefMexError, match="Sparse inputs not supported"):
        shimmex.call("psdjmul", 1, col(c["x"]), sp.csc_matrix(col(c["y"])), K)


def test_psdjmul_shim_matches_the_library(shimmex):
    import helpers
    from sedumi_amd.build import SHIMS
    assert "psdjmul" in SHIMS
    helpers.use_emu()
    check_shim(shimmex)
