"""Shared by the psdjmul / maxstep_psd / wstruct_psd tests: the cases, psdjmul.m:40-73 in numpy.longdouble and the checks of a case
on whichever library capi is bound to.  psdjmul has no compiled reference (it is an .m file): the expected value is the longdouble one.

Value bound of psdjmul, per plane and per entry of a block of order n, u = 2^-53, gamma_p = p u / (1 - p u), |M| = |Re M| + |Im M|, P = |X| |Y|:
    real block       |z - z_ld| <= gamma_{2n+1} (P + P^T) / 2
    Hermitian block  per plane  <= gamma_{4n+1} (P + P^T) / 2
Entry (i, j) of 2 Z is the sum of the n products of (X Y)(i, j) and the n products of conj((X Y)(j, i)) -- on a Hermitian block two real products
per complex one and plane: 2 n (4 n) real products whose absolute values add up to at most (P + P^T)(i, j).  gamma_{2n} (gamma_{4n}) bounds such a
sum in any order, with or without FMA (Higham, Accuracy and Stability, section 3.1); + 1 for rounding the longdouble value to double; halving is
exact.  Derived, not measured; no margin on top.

The fused calls have no tolerance: they are bit-equal to the single calls they replace."""
import numpy as np

import psd_frames_exact as pfe
import psdfact_exact as pe
import triu_exact as te

LD, CLD = np.longdouble, np.clongdouble
gamma = te.gamma
make_K = te.make_K
CASES = te.CASES
GPU_ONLY_CASE = te.GPU_ONLY_CASE
FUSED_CASES = [dict(s=[5]), dict(hs=[2]), dict(s=[33, 65]), dict(s=[70, 35]), dict(s=[65], hs=[33])]
BAD_CASE = dict(s=[33, 65, 34])                                          # block 1 not positive definite at p = 64: its second tile row, a block behind it

_cache = {}


def _abs1(M):
    return (np.abs(np.real(M)) + np.abs(np.imag(M))).astype(LD)


def make_case(kw, seed=1):
    """x, y Gaussian, no symmetry, every entry of every block filled, Hermitian diagonals complex; the longdouble answer and the bound of every
    entry.  Computed once per session, never modified."""
    key = (repr(sorted(kw.items())), seed)
    if key in _cache:
        return _cache[key]
    K = make_K(kw)
    rng = np.random.default_rng(seed)
    xs, ys, Z, Bnd = [], [], [], []
    for n, herm in pfe.block_list(K):
        X, Y = (rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if herm else 0) for _ in range(2))
        xs.append(X); ys.append(Y)
        ZZ = X.astype(CLD if herm else LD) @ Y.astype(CLD if herm else LD)                            # psdjmul.m: ZZ = XX*YY
        Z.append(LD(0.5) * (ZZ + ZZ.conj().T))                                                       #            ZZ = 0.5*(ZZ + ZZ')
        P = _abs1(X) @ _abs1(Y)
        Bnd.append(gamma(LD(4 * n + 1 if herm else 2 * n + 1)) * LD(0.5) * (P + P.T))
    c = dict(K=K, kw=kw, xs=xs, ys=ys, x=pfe.pack_blocks(xs, K), y=pfe.pack_blocks(ys, K), Z=Z, Bnd=Bnd)
    for v in (c["x"], c["y"]):
        v.setflags(write=False)
    _cache[key] = c
    return c


def check_value_and_symmetry(c, z):
    """checks 1 and 2"""
    K = c["K"]
    for Zl, E, Bd, (n, herm) in zip(pfe.split_blocks(z, K), c["Z"], c["Bnd"], pfe.block_list(K)):
        for name, part in (("Re", np.real),) + ((("Im", np.imag),) if herm else ()):
            dev = np.abs(part(Zl).astype(LD) - part(E))
            worst = float(np.max(dev / np.where(Bd > 0, Bd, 1))) if n else 0.0
            print("psdjmul    n=%-4d %s %s  largest |z - z_ld| / bound %.3f" % (n, "herm" if herm else "real", name, worst))
            assert (dev <= Bd).all(), (n, herm, name, worst)
        assert np.array_equal(np.real(Zl), np.real(Zl).T)                                            # symmetric / Hermitian, bit for bit
        if herm:
            assert np.array_equal(np.imag(Zl), -np.imag(Zl).T)
            d = np.imag(Zl).diagonal()
            assert not d.any() and not np.signbit(d).any()                                           # Im diag exactly 0.0
    assert np.isfinite(z).all()


def check_case(kw):
    """checks 1 - 3 and the lengths and the repeat of 4 on one case"""
    from sedumi_amd import mex
    c = make_case(kw)
    K = c["K"]
    z = mex.psdjmul(c["x"], c["y"], K)
    assert z.shape == (c["x"].size, 1)
    z = z.ravel()
    check_value_and_symmetry(c, z)
    assert z.any()
    # 3: y = the identity of every block: 0.5 (X + X^H) formed in double, exactly
    eye = pfe.pack_blocks([np.eye(n, dtype=complex if herm else float) for n, herm in pfe.block_list(K)], K)
    want = pfe.pack_blocks([0.5 * (X + X.conj().T) for X in c["xs"]], K)
    assert np.array_equal(mex.psdjmul(c["x"], eye, K).ravel(), want)
    assert np.array_equal(mex.psdjmul(eye, c["x"], K).ravel(), want)                                  # and the identity on the left: the other operand's indexing
    # 4: whole-cone length (K.l = 1 entry in front), two calls
    zl = mex.psdjmul(np.concatenate(([np.nan], c["x"])), np.concatenate(([7.0], c["y"])), K).ravel()
    assert np.array_equal(z, zl)
    assert np.array_equal(z, mex.psdjmul(c["x"], c["y"], K).ravel())
    return z


def check_block_alone():
    """check 4: the block of order 65 alone gives the bits it has inside s=[129, 3, 65]"""
    from sedumi_amd import mex
    c = make_case(dict(s=[129, 3, 65]))
    z3 = mex.psdjmul(c["x"], c["y"], c["K"]).ravel()
    z1 = mex.psdjmul(c["xs"][2].ravel(order="F"), c["ys"][2].ravel(order="F"), make_K(dict(s=[65]))).ravel()
    assert np.array_equal(z3[-65 * 65:], z1) and np.abs(z1).max() > 0


def check_nan_block_in_a_list():
    """check 4: a NaN in block 1 of s=[65, 129, 64] leaves blocks 0 and 2 bit-equal to their values without it"""
    from sedumi_amd import mex
    c = make_case(dict(s=[65, 129, 64]))
    K = c["K"]
    z = mex.psdjmul(c["x"], c["y"], K).ravel()
    X1 = c["xs"][1].copy()
    X1[100, 7] = np.nan
    zn = mex.psdjmul(pfe.pack_blocks([c["xs"][0], X1, c["xs"][2]], K), c["y"], K).ravel()
    a, b = 65 * 65, 65 * 65 + 129 * 129
    assert np.isnan(zn[a:b]).any() and np.isfinite(z).all()
    assert np.array_equal(zn[:a], z[:a]) and np.array_equal(zn[b:], z[b:])


def check_lengths_are_refused():
    """checks 5 and 9: len < lenud and x, y of different sizes raise; K.s empty returns the empty answers.  Needs no device: refused (or returned)
    before anything is allocated."""
    import ctypes as C
    import pytest
    from sedumi_amd import capi, mex, problem
    from sedumi_amd.capi import SdmError
    K = problem.make_K(1, [], [4])
    one = np.ones(16)
    for call in (lambda: mex.psdjmul(np.ones(15), np.ones(15), K), lambda: mex.psdjmul(one, np.ones(17), K),
                 lambda: mex.maxstep_psd(one, np.ones(15), K), lambda: mex.maxstep_psd(np.ones(15), one, K), lambda: mex.maxstep_psd(np.ones(17), one, K),
                 lambda: mex.wstruct_psd(np.ones(15), np.ones(15), K), lambda: mex.wstruct_psd(one, np.ones(17), K)):
        with pytest.raises(SdmError, match="size mismatch"):
            call()
    Kc, keep = capi.make_cone(1, [], [4], 1)
    L, ip, info, m = capi.lib(), C.c_int(7), C.c_int(7), C.c_double(0.0)
    for rc in (L.sdm_psdjmul(C.byref(Kc), capi.pf(one), capi.pf(one), C.c_int64(15), capi.pf(one)),
               L.sdm_maxstep_psd(C.byref(Kc), capi.pf(one), capi.pf(one), C.c_int64(15), C.byref(m), C.byref(info)),
               L.sdm_wstruct_psd(C.byref(Kc), capi.pf(one), capi.pf(one), C.c_int64(15), capi.pf(one), capi.pf(one), capi.pf(one), C.byref(ip),
                                 C.byref(info))):
        assert rc != 0 and b"size mismatch" in L.sdm_last_error()
    K0 = problem.make_K(3, [3], [])
    assert mex.psdjmul(np.ones(6), np.ones(6), K0).size == 0
    m, info = mex.maxstep_psd(np.zeros(0), np.ones(6), K0, nlhs=2)                                  # 9
    assert m.shape == (1, 1) and m[0, 0] == np.inf and info == -1 and mex.maxstep_psd(np.zeros(0), np.ones(6), K0)[0, 0] == np.inf
    ux, s, lab, ispos, info = mex.wstruct_psd(np.ones(6), np.ones(6), K0)
    assert ux.size == 0 and s.size == 0 and lab.size == 0 and ispos is True and info == -1


# ------------------------------------------------------------------------------------------------ the fused calls
def check_maxstep(kw):
    """check 7: maxstep_psd(ud, g) bit-equal to minpsdeig(psdinvscale(ud, g)): mineig and info, also with g at whole-cone length"""
    from sedumi_amd import mex
    c = pe.make_case(kw, "flat")
    K = c["K"]
    ud = mex.psdfactor(c["x"], K)
    wm, wi = mex.minpsdeig(mex.psdinvscale(ud, c["g"], K), K, nlhs=2)
    m, i = mex.maxstep_psd(ud, c["g"], K, nlhs=2)
    print("maxstep_psd", kw, "mineig", m[0, 0], "info", i)
    assert m.shape == (1, 1) and np.array_equal(m, wm, equal_nan=True) and i == wi == -1 and np.isfinite(m).all()
    assert np.array_equal(mex.maxstep_psd(ud, c["g"], K), wm)
    ml, il = mex.maxstep_psd(ud, np.concatenate(([np.nan], c["g"])), K, nlhs=2)
    assert np.array_equal(ml, wm) and il == wi


def check_maxstep_nan_block():
    """check 7: a NaN in block 1 of g: info == 1 and a NaN mineig, as the composition gives"""
    from sedumi_amd import mex
    c = pe.make_case(dict(s=[33, 65]), "flat")
    K = c["K"]
    ud = mex.psdfactor(c["x"], K)
    G1 = c["gs"][1].copy()
    G1[40, 3] = np.nan
    g = pfe.pack_blocks([c["gs"][0], G1], K)
    wm, wi = mex.minpsdeig(mex.psdinvscale(ud, g, K), K, nlhs=2)
    m, i = mex.maxstep_psd(ud, g, K, nlhs=2)
    assert i == 1 and wi == 1 and np.isnan(m[0, 0]) and np.array_equal(m, wm, equal_nan=True)


def _compose_wstruct(x, z, K):
    """sdm_trydif_psd followed by sdm_psdeig(K, s, lenud, lab, NULL, info) (the raw call: the mirror hands info out only beside q)"""
    import ctypes as C
    from sedumi_amd import capi, mex
    ux, s, ispos = mex.trydif_psd(x, z, K)
    Kc, keep, lenud, slen = mex._frame_sizes(K, mex.FRAME_HOUSEHOLDER)[:4]
    lab, info, sv = np.zeros(slen), C.c_int(7), np.ascontiguousarray(s.ravel())
    capi.check(capi.lib().sdm_psdeig(C.byref(Kc), capi.pf(sv), C.c_int64(lenud), capi.pf(lab), None, C.byref(info)))
    sweeps = mex.psdeig_last_sweeps()
    return ux, s, lab.reshape(-1, 1), ispos, int(info.value), sweeps


def _check_wstruct_equal(x, z, K):
    from sedumi_amd import mex
    ux, s, lab, ispos, info, sweeps = _compose_wstruct(x, z, K)
    got = mex.wstruct_psd(x, z, K)
    assert mex.psdeig_last_sweeps() == sweeps                                                        # the sweeps of the fused call are reported too
    for name, a, b in zip(("ux", "s", "lab"), got[:3], (ux, s, lab)):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), name
    assert got[3] is ispos and got[4] == info
    gl = mex.wstruct_psd(np.concatenate(([np.nan], x)), np.concatenate(([np.nan], z)), K)            # whole-cone length
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(gl[:3], got[:3])) and gl[3:] == got[3:]
    return got


def check_wstruct(kw):
    """check 8: wstruct_psd(x, z) bit-equal in ux, s, lab, ispos, info and sweeps to trydif_psd(x, z) followed by psdeig(s)"""
    c = pe.make_case(kw, "flat")
    ux, s, lab, ispos, info = _check_wstruct_equal(c["x"], c["z"], c["K"])
    print("wstruct_psd", kw, "ispos", ispos, "info", info, "min lab", float(lab.min()))
    assert ispos is True and info == -1 and np.isfinite(lab).all() and (lab > 0).all()


def check_wstruct_bad_block():
    """check 8: block 1 of BAD_CASE with pivot 64 <= -2 (psdfact_exact's construction): ispos False, ux and s exactly 0.0 from block 1 on, block 0 as
    without it, and everything what the composition gives"""
    c = pe.make_case(BAD_CASE, "flat")
    K = c["K"]
    good = _check_wstruct_equal(c["x"], c["z"], K)
    x = pfe.pack_blocks([c["xs"][0], pe._minus4(c["xs"][1], 64), c["xs"][2]], K)
    ux, s, lab, ispos, info = _check_wstruct_equal(x, c["z"], K)
    a = 33 * 33
    assert ispos is False and good[3] is True
    assert np.array_equal(ux[:a], good[0][:a]) and np.array_equal(s[:a], good[1][:a]) and np.array_equal(lab[:33], good[2][:33])
    assert not ux[a:].any() and not s[a:].any() and ux[:a].any()


# ------------------------------------------------------------------------------------------------ the driver
ALL_EARLIER = dict(device_cone=True, device_qr=True, device_rot=True, device_updt=True, device_fact=True, device_eig=True)


def check_driver_switches():
    """checks 10 and 11: solve(...) on the problem of urot_exact.check_driver_switch with that check's bounds (they are literals inside that function:
    restated here); both switches off is the default run bit for bit; each switch alone and both with the six earlier ones stay within the bounds;
    with device_step the driver makes the fused calls and none of the calls they replace"""
    import collections
    from sedumi_amd.driver import solve
    from sedumi_amd.driver import loop as lp
    from sedumi_amd.driver.conemex import NativeMex
    h = NativeMex()
    assert h.device_jmul is False and h.device_step is False
    h = NativeMex(device_jmul=True)
    assert h.device_jmul is True and h.device_step is False and h.device_eig is False
    h = NativeMex(device_step=True)
    assert h.device_step is True and h.device_jmul is False and h.device_fact is False
    r0 = solve(*pfe.small_hermitian_sdp(), hot=lp.HipHot())
    rf = solve(*pfe.small_hermitian_sdp(), hot=lp.HipHot(), device_jmul=False, device_step=False)
    assert all(rf[k] == r0[k] for k in ("iter", "STOP", "cx", "by", "x0", "feasratio")) and repr(rf["rows"]) == repr(r0["rows"])   # the whole iteration log
    seen = collections.Counter()
    orig = NativeMex.call

    def counting(self, name, nlhs, *args):
        seen[name] += 1
        return orig(self, name, nlhs, *args)

    NativeMex.call = counting
    try:
        for kw in (dict(device_jmul=True), dict(device_step=True), dict(device_jmul=True, device_step=True, **ALL_EARLIER)):
            seen.clear()
            r1 = solve(*pfe.small_hermitian_sdp(), hot=lp.HipHot(), **kw)
            print(kw, "iter", r0["iter"], r1["iter"], "cx", r0["cx"], r1["cx"], "by", r0["by"], r1["by"])
            assert abs(r1["iter"] - r0["iter"]) <= 1 and r1["iter"] > 3
            assert abs(r1["cx"] - r0["cx"]) <= 1e-6 * abs(r0["cx"]) and abs(r1["by"] - r0["by"]) <= 1e-6 * abs(r0["by"])
            if kw.get("device_jmul"):
                assert seen["psdjmul"] > 0
            if kw.get("device_step"):
                assert seen["maxstep_psd"] > 0 and seen["wstruct_psd"] > 0
                assert not seen["minpsdeig"] and not seen["psdinvscale"] and not seen["trydif_psd"]
    finally:
        NativeMex.call = orig
