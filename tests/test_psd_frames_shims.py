"""the psdframeit / psdinvjmul mexFunction shims (sedumi_amd/mexshims) against the reference gateways, linked to the emulated
build of the C ABI and driven through the same mxArray marshalling as the reference MEX (tests/test_mexshims.py's way); the same on the
hipcc library: test_psd_frames_gpu.py."""
import os

import numpy as np
import pytest

from helpers import ROOT
import psd_frames_exact as pfe


@pytest.fixture(scope="module")
def shimmex(refmex):
    import sys
    from test_mexshims import build_shims
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
    import build_emu
    return build_shims(build_emu.build(), os.path.join(ROOT, "tests", "hipemu", "_mexshims"))


def check_shims(refmex, shimmex):
    from oracle.refmex import RefMexError
    from sedumi_amd import problem
    kw = dict(s=[6, 65], hs=[4])
    c = pfe.make_case(refmex, kw, 21)
    K = c["K"]
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)
    x = shimmex.call("psdframeit", 1, col(c["lab"]), col(c["frms"]), K)
    z = shimmex.call("psdinvjmul", 1, col(c["lab"]), col(c["frms"]), col(c["y"]), K)
    pfe.check_rule("psdframeit shim", np.asarray(x).ravel(), c["Xref"], c["X"], K)
    pfe.check_rule("psdinvjmul shim", np.asarray(z).ravel(), c["Zref"], c["Z"], K)
    # lab at lendiag length and y at full length inside a K with an LP part and Lorentz cones (psdframeit.c:134-137, psdinvjmul.c:195-202)
    K2 = problem.make_K(3, [3, 4], kw["s"], hs=kw["hs"])
    rng = np.random.default_rng(2)
    lab2 = np.concatenate((rng.random(3 + 2 * 2), c["lab"]))
    y2 = np.concatenate((rng.standard_normal(3 + 7), c["y"]))
    for lab_, y_ in ((lab2, y2), (c["lab"], y2), (lab2, c["y"])):
        assert np.array_equal(shimmex.call("psdframeit", 1, col(lab_), col(c["frms"]), K2), x)
        assert np.array_equal(shimmex.call("psdinvjmul", 1, col(lab_), col(c["frms"]), col(y_), K2), z)
        assert np.array_equal(refmex.call("psdinvjmul", 1, col(lab_), col(c["frms"]), col(y_), K2).ravel(), c["Zref"])
    with pytest.raises(RefMexError, match="frms size mismatch"):
        shimmex.call("psdframeit", 1, col(c["lab"]), col(c["frms"][:-1]), K)
    with pytest.raises(RefMexError, match="size xfrm mismatch"):
        shimmex.call("psdinvjmul", 1, col(c["lab"]), col(np.concatenate((c["frms"], [0.0]))), col(c["y"]), K)


def test_psd_frame_shims_match_the_reference_gateways(refmex, shimmex):
    from sedumi_amd.build import SHIMS
    assert "psdframeit" in SHIMS and "psdinvjmul" in SHIMS
    check_shims(refmex, shimmex)
