"""the urotorder, givensrot and sqrtinv mexFunction shims (sedumi_amd/mexshims) against the reference gateways, linked to the
emulated build of the C ABI and driven through the same mxArray marshalling as the reference MEX (tests/test_mexshims.py's way); the same on the
hipcc library: test_urot_gpu.py."""
import os

import numpy as np
import pytest

from helpers import ROOT
import urot_exact as ue


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
    c = ue.make_case(refmex, dict(s=[6, 40], hs=[5]), 1)
    K = c["K"]
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)
    out = [np.asarray(v) for v in shimmex.call("urotorder", 4, col(c["u"]), K, c["maxu"])]
    assert out[0].shape == (c["u"].size, 1) and out[1].shape == out[2].shape == (c["perm"].size, 1) and out[3].shape == (c["g"].size, 1)
    ue.check_urotorder(c, tuple(v.ravel() for v in out))
    for nlhs in (1, 2, 3):                                               # nlhs 1 .. 4: the first outputs, the same arrays
        got = shimmex.call("urotorder", nlhs, col(c["u"]), K, c["maxu"])
        got = [got] if nlhs == 1 else list(got)
        assert len(got) == nlhs and all(np.array_equal(np.asarray(a), b) for a, b in zip(got, out))
    for pin in (np.zeros((0, 0)), np.zeros((0, 1))):                     # an empty permIN is an absent one
        got = shimmex.call("urotorder", 2, col(c["u"]), K, c["maxu"], pin)
        assert np.array_equal(np.asarray(got[1]), out[1])
    pin = np.concatenate([1.0 + np.random.default_rng(3).permutation(n) for n in (6, 40, 5)])
    a, b = shimmex.call("urotorder", 2, col(c["u"]), K, c["maxu"], col(pin)), refmex.call("urotorder", 2, col(c["u"]), K, c["maxu"], col(pin))
    assert np.array_equal(np.asarray(a[1]), np.asarray(b[1]))
    g0 = np.asarray(shimmex.call("urotorder", 4, col(c["u"]), K, 1e3)[3])
    assert g0.shape == (0, 1) and np.asarray(refmex.call("urotorder", 4, col(c["u"]), K, 1e3)[3]).shape == (0, 1)   # no rotation: g is 0 x 1
    y = np.asarray(shimmex.call("givensrot", 1, col(c["gjc"]), col(c["g"]), col(c["x"]), K))
    assert y.shape == (c["x"].size, 1)
    ue.check_rule("givensrot shim", ue.pfe.split_blocks(y.ravel(), K), ue.pfe.split_blocks(c["yref"], K), c["Yx"], K)
    s = np.asarray(shimmex.call("sqrtinv", 1, col(c["x"]), col(np.concatenate(([1.0], c["vlab"]))), K))
    assert s.shape == (c["x"].size, 1) and (np.abs(s.ravel() - c["sref"]) <= 2 * np.spacing(np.abs(c["sref"]))).all()
    # size errors, raised like the reference's asserts
    with pytest.raises(RefMexError, match="u size mismatch"):
        shimmex.call("urotorder", 4, col(c["u"][:-1]), K, c["maxu"])
    with pytest.raises(RefMexError, match="perm size mismatch"):
        shimmex.call("urotorder", 4, col(c["u"]), K, c["maxu"], col(pin[:-1]))
    with pytest.raises(RefMexError, match="x size mismatch"):
        shimmex.call("givensrot", 1, col(c["gjc"]), col(c["g"]), col(c["x"][:-1]), K)
    with pytest.raises(RefMexError, match="g size mismatch"):
        shimmex.call("givensrot", 1, col(c["gjc"]), col(c["g"][:-1]), col(c["x"]), K)
    with pytest.raises(RefMexError, match="v size mismatch"):
        shimmex.call("sqrtinv", 1, col(c["x"]), col(c["vlab"][:-1]), K)
    with pytest.raises(RefMexError, match="q size mismatch"):
        shimmex.call("sqrtinv", 1, col(c["x"][:-1]), col(c["vlab"]), K)


def test_urot_shims_match_the_reference_gateways(refmex, shimmex):
    from sedumi_amd.build import SHIMS
    assert {"urotorder", "givensrot", "sqrtinv"} <= set(SHIMS)
    check_shims(refmex, shimmex)
