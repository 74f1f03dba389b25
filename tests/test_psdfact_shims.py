"""the psdfactor and psdinvscale mexFunction shims (sedumi_amd/mexshims) linked to the emulated build of the C ABI and driven through
the same mxArray marshalling as the reference MEX (tests/test_mexshims.py's way): both outputs of psdfactor and the output of psdinvscale bit-equal
to sedumi_amd.mex on the library they are linked to, the .m files' answers for a cone without PSD blocks, sparse arguments refused; the same on the
hipcc library: test_psdfact_gpu.py."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import ROOT
import psd_frames_exact as pfe
import psdfact_exact as pe


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
    c = pe.make_case(dict(s=[6, 70], hs=[5]), "flat")
    K = c["K"]
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)
    want, wpos = mex.psdfactor(c["x"], K, nlhs=2)
    ux, ispos = shimmex.call("psdfactor", 2, col(c["x"]), K)
    ux = np.asarray(ux)
    assert ux.shape == want.shape and np.array_equal(ux, want) and wpos is True and bool(np.asarray(ispos).ravel()[0]) is True
    assert np.asarray(ispos).size == 1
    pe.check_factor_value(c["xs"], ux.ravel(), K)
    assert np.array_equal(np.asarray(shimmex.call("psdfactor", 1, col(np.concatenate(([0.5], c["x"]))), K)), want)   # whole-cone length, one output
    # a block that is not positive definite: both outputs again
    bad = pfe.pack_blocks([c["xs"][0], c["xs"][1] - 4.0 * np.eye(70), c["xs"][2]], K)
    want, wpos = mex.psdfactor(bad, K, nlhs=2)
    ux, ispos = shimmex.call("psdfactor", 2, col(bad), K)
    assert wpos is False and bool(np.asarray(ispos).ravel()[0]) is False and np.array_equal(np.asarray(ux), want)
    assert np.asarray(ux)[:36].all() and not np.asarray(ux)[36:].any()
    ud = mex.psdfactor(c["x"], K)
    y = mex.psdinvscale(ud, c["g"], K)
    got = np.asarray(shimmex.call("psdinvscale", 1, col(ud), col(c["g"]), K))
    assert got.shape == y.shape and np.array_equal(got, y)
    pe.check_invscale_value(ud.ravel(), c["gs"], got.ravel(), K)
    assert np.array_equal(np.asarray(shimmex.call("psdinvscale", 1, col(ud), col(np.concatenate(([0.5], c["g"]))), K)), y)
    # K.s empty: zeros(0,1) and true; []
    K0 = problem.make_K(3, [3], [])
    u0, i0 = shimmex.call("psdfactor", 2, col(np.ones(6)), K0)
    assert np.asarray(u0).shape == (0, 1) and bool(np.asarray(i0).ravel()[0]) is True
    assert np.asarray(shimmex.call("psdinvscale", 1, col(np.zeros(0)), col(np.ones(6)), K0)).size == 0
    with pytest.raises(RefMexError, match="size mismatch"):
        shimmex.call("psdfactor", 1, col(c["x"][1:]), K)
    with pytest.raises(RefMexError, match="size mismatch"):
        shimmex.call("psdinvscale", 1, col(ud), col(c["g"][1:]), K)
    with pytest.raises(RefMexError, match="size mismatch"):
        shimmex.call("psdinvscale", 1, col(ud.ravel()[1:]), col(c["g"]), K)
    with pytest.raises(RefMexError, match="Sparse inputs not supported"):
        shimmex.call("psdfactor", 1, sp.csc_matrix(col(c["x"])), K)
    with pytest.raises(RefMexError, match="Sparse inputs not supported"):
        shimmex.call("psdinvscale", 1, sp.csc_matrix(col(ud)), col(c["g"]), K)
    with pytest.raises(RefMexError, match="Sparse inputs not supported"):
        shimmex.call("psdinvscale", 1, col(ud), sp.csc_matrix(col(c["g"])), K)


def test_psdfact_shims_match_the_library(shimmex):
    import helpers
    from sedumi_amd.build import SHIMS
    assert "psdfactor" in SHIMS and "psdinvscale" in SHIMS
    helpers.use_emu()
    check_shims(shimmex)
