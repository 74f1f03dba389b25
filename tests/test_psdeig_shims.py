"""the psdeig and minpsdeig mexFunction shims (sedumi_amd/mexshims) linked to the emulated build of the C ABI and driven through the
same mxArray marshalling as the reference MEX (tests/test_mexshims.py's way): the outputs bit-equal to sedumi_amd.mex on the library they are
linked to for nlhs 1 and 2, the .m files' [] for a cone without PSD blocks, sparse arguments refused; the same on the hipcc library:
test_psdeig_gpu.py."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import ROOT
import psdeig_exact as pe


@pytest.fixture(scope="module")
def shimmex(refmex):
    import sys
    from test_mexshims import build_shims
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
    import build_emu
    return build_shims(build_emu.build(), os.path.join(ROOT, "tests", "hipemu", "_mexshims"))


def check_shims(shimmex):
    """capi must be bound to the library the shims are linked to"""
    from oracle.refmex import RefMexError
    from sedumi_amd import mex, problem
    c = pe.make_case(dict(s=[6, 40], hs=[5]), "sym")
    K = c["K"]
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)
    wl, wq = mex.psdeig(c["x"], K, nlhs=2)
    lab, q = shimmex.call("psdeig", 2, col(c["x"]), K)
    lab, q = np.asarray(lab), np.asarray(q)
    assert lab.shape == wl.shape and q.shape == wq.shape and np.array_equal(lab, wl) and np.array_equal(q, wq)
    pe.check_values(c, lab.ravel(), q.ravel(), "shim")
    assert np.array_equal(np.asarray(shimmex.call("psdeig", 1, col(c["x"]), K)), wl)
    assert np.array_equal(np.asarray(shimmex.call("psdeig", 1, col(np.concatenate(([0.5], c["x"]))), K)), wl)        # whole-cone length
    m = np.asarray(shimmex.call("minpsdeig", 1, col(c["x"]), K))
    assert m.shape == (1, 1) and np.array_equal(m, mex.minpsdeig(c["x"], K)) and m[0, 0] == wl.min()
    assert np.array_equal(np.asarray(shimmex.call("minpsdeig", 1, col(np.concatenate(([0.5], c["x"]))), K)), m)
    K0 = problem.make_K(3, [3], [])                                      # K.s empty: []
    l0, q0 = shimmex.call("psdeig", 2, col(np.ones(6)), K0)
    assert np.asarray(l0).size == 0 and np.asarray(q0).size == 0
    assert np.asarray(shimmex.call("minpsdeig", 1, col(np.ones(6)), K0)).size == 0
    for name in ("psdeig", "minpsdeig"):
        with pytest.raises(RefMexError, match="size mismatch"):
            shimmex.call(name, 1, col(c["x"][1:]), K)
        with pytest.raises(RefMexError, match="Sparse inputs not supported"):
            shimmex.call(name, 1, sp.csc_matrix(col(c["x"])), K)


def test_psdeig_shims_match_the_library(shimmex):
    import helpers
    from sedumi_amd.build import SHIMS
    assert "psdeig" in SHIMS and "minpsdeig" in SHIMS
    helpers.use_emu()
    check_shims(shimmex)
