"""Shared by the psdfactor / psdinvscale / psdscale / trydif_psd tests: the cases, the defining equations of psdfactor.m:44-80,
psdinvscale.m:40-83 and psdscale.m:76-119 evaluated in numpy.longdouble, and the checks of a case on whichever library capi is bound to.  Both
functions are .m files: there is no compiled reference, and no measured tolerance either -- the kernels obtain every entry by substitution, so the
componentwise backward error bounds of Cholesky and of a triangular solve hold for any order of the sums (Higham, Accuracy and Stability, Lemma 8.4,
Thm 10.3).  u = 2^-53, gamma_p = p u / (1 - p u), |M| = |Re M| + |Im M|; bounds are per plane and per entry, derived, with no margin on top.

psdfactor, entry (i, j), m = min(i, j) + 1:   |X - L L^H| <= gamma_p (|L| |L|^T)
    real block       p = m + 2.  l_ij = (x_ij - sum_{k<j} l_ik l_jk) / l_jj: m - 1 products and a division, gamma_m by Lemma 8.4 in any order; the
                     diagonal takes a square root, which counts twice: gamma_{m+1}; + 1 because the residual is formed from rounded inputs.
    Hermitian block  p = 2 m + 1.  Per plane the sum has two real products per k (Re: Re l_ik Re l_jk + Im l_ik Im l_jk; Im likewise): 2 (m - 1)
                     products and a division by the REAL l_jj (one rounding per plane): gamma_{2m-1}; the square root: gamma_{2m}; + 1 as above.
psdinvscale, order n:   |T Y T^H - X| <= gamma_p (2 + gamma_p) (|T| |Y| |T|^T)     (two substitutions of backward error gamma_p, |W| <= (1 + gamma_p) |T| |Y|)
    real block       p = n.  At most n - 1 products and a division per entry.
    Hermitian block  p = 2 n + 6.  Per plane at most 2 (n - 1) real products: their perturbations are gamma_{2n-2} relative to the plane's own
                     leading term.  The quotient by the complex diagonal entry t is formed as (s conj(t)) / (t conj(t)): two roundings on each
                     term of the numerator, two on the denominator, one on the quotient, so each plane of q is off by gamma_5 |q|_2 at most,
                     |t q^ - s| <= sqrt(2) gamma_5 / (1 - sqrt(2) gamma_5) |t| |q^| <= gamma_8 |t| |q^| per plane; gamma_8 + gamma_{2n-2} (1 + gamma_8)
                     <= gamma_{2n+6}.
    The .m file sets Im diag(Y) = 0 afterwards (:79).  For a Hermitian X that removes a rounding error; for any other X it removes data, so the
    residual is formed with the longdouble value of Im diag(Y) put back (and Im diag(Y) itself is checked to be exactly 0.0).
psdscale, order n:      |Y - T^H X T| <= gamma_p (2 + gamma_p) (|T|^T |X| |T|): two dot products of length <= n in a row (triu_exact's bound, twice),
    real p = n + 1, Hermitian p = 2 n + 1 (+ 1: the longdouble value rounded to double).

Exactly singular blocks are a rounding decision (a pivot of the order of u |X|) and are not tested: every failing case here has a pivot <= -2."""
import numpy as np

import psd_frames_exact as pfe
import triu_exact as te

LD, CLD = np.longdouble, np.clongdouble
gamma = te.gamma
make_K = te.make_K
CASES = te.CASES
GPU_ONLY_CASE = te.GPU_ONLY_CASE
SPECTRA = ("flat", "log")                                                 # lambda in [1, 2]; log-spaced 1 .. 1e-8 (every exact pivot >= 1e-8)
BAD_P = (0, 40, 63, 64, 100, 128)

_cache = {}


def _ro(v):
    v.setflags(write=False)
    return v


def pd_block(rng, n, herm, spectrum):
    """X = Q diag(lambda) Q^H, symmetrised; Q from the QR of a Gaussian matrix"""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if herm else 0))
    lam = rng.uniform(1.0, 2.0, n) if spectrum == "flat" else np.logspace(0.0, -8.0, n)
    X = (Q * lam) @ Q.conj().T
    return (X + X.conj().T) / 2


def make_case(kw, spectrum, seed=1):
    """x (the matrix factored), z (a second positive definite one, lambda in [1, 2]) and g (Gaussian, no symmetry) of every block.  Computed once per
    session, never modified."""
    key = (repr(sorted(kw.items())), spectrum, seed)
    if key not in _cache:
        K = make_K(kw)
        rng = np.random.default_rng(seed)
        xs, zs, gs = [], [], []
        for n, herm in pfe.block_list(K):
            xs.append(pd_block(rng, n, herm, spectrum))
            zs.append(pd_block(rng, n, herm, "flat"))
            gs.append(rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if herm else 0))
        _cache[key] = dict(K=K, kw=kw, xs=xs, zs=zs, gs=gs, x=_ro(pfe.pack_blocks(xs, K)), z=_ro(pfe.pack_blocks(zs, K)), g=_ro(pfe.pack_blocks(gs, K)))
    return _cache[key]


def _abs1(M):
    return (np.abs(np.real(M)) + np.abs(np.imag(M))).astype(LD)


def _planes(herm):
    return (("Re", np.real),) + ((("Im", np.imag),) if herm else ())


def _report(what, n, herm, name, R, Bd, mask):
    worst = float(np.max(np.where(mask, R / np.where(Bd > 0, Bd, 1), 0))) if n else 0.0
    print("%-11s n=%-4d %s %s  largest residual / bound %.3f" % (what, n, "herm" if herm else "real", name, worst))
    assert (R[mask] <= Bd[mask]).all(), (what, n, herm, name, worst)


# ------------------------------------------------------------------------------------------------ the .m files in longdouble
def ld_solve_upper(T, B):
    """T \\ B by back substitution in longdouble, T upper triangular"""
    n = T.shape[0]
    Y = np.array(B, dtype=T.dtype)
    for r in range(n - 1, -1, -1):
        Y[r] = (Y[r] - T[r, r + 1:] @ Y[r + 1:]) / T[r, r]
    return Y


def ld_psdinvscale(T, X):
    """psdinvscale.m:73 without :79: TT \\ (XX / TT')"""
    W = ld_solve_upper(T.conj(), X.T).T                                  # W T^H = X  <=>  conj(T) W^T = X^T
    return ld_solve_upper(T, W)


# ------------------------------------------------------------------------------------------------ checks of the values
def check_factor_value(xs, ux, K):
    """|X - L L^H| within the bound on the lower triangle; check 1: the mirror bit for bit, Im diag = 0.0, everything finite"""
    for X, F, (n, herm) in zip(xs, pfe.split_blocks(ux, K), pfe.block_list(K)):
        L = np.tril(F).astype(CLD if herm else LD)
        Res = X.astype(L.dtype) - L @ L.conj().T
        i, j = np.indices((n, n))
        m = np.minimum(i, j) + 1
        Bd = gamma(((2 * m + 1) if herm else (m + 2)).astype(LD)) * (_abs1(L) @ _abs1(L).T)
        low = i >= j
        for name, part in _planes(herm):
            _report("psdfactor", n, herm, name, np.abs(part(Res)), Bd, low)
        lo = np.tril(np.ones((n, n), dtype=bool), -1)
        assert np.array_equal(np.real(F)[lo], np.real(F).T[lo])
        if herm:
            assert np.array_equal(np.imag(F)[lo], -np.imag(F).T[lo])
            assert not np.imag(F).diagonal().any() and not np.signbit(np.imag(F).diagonal()).any()
        assert (np.real(F).diagonal() > 0).all()
    assert np.isfinite(ux).all()


def check_invscale_value(ud, xs, y, K):
    """|T Y T^H - X| within the bound on every entry, T = triu(ud); Im diag(Y) = 0.0 exactly"""
    for Tm, X, Y, (n, herm) in zip(pfe.split_blocks(ud, K), xs, pfe.split_blocks(y, K), pfe.block_list(K)):
        T = np.triu(Tm).astype(CLD if herm else LD)
        Yl = Y.astype(T.dtype)
        if herm:
            assert not np.imag(Y).diagonal().any()
            Yl = Yl + 1j * np.diag(np.imag(ld_psdinvscale(T, X.astype(CLD)).diagonal()))
        Res = T @ Yl @ T.conj().T - X.astype(T.dtype)
        g = gamma(LD(2 * n + 6 if herm else n))
        Bd = g * (2 + g) * (_abs1(T) @ _abs1(Yl) @ _abs1(T).T)
        for name, part in _planes(herm):
            _report("psdinvscale", n, herm, name, np.abs(part(Res)), Bd, np.ones((n, n), dtype=bool))
    assert np.isfinite(y).all()


def check_scale_value(ud, xs, y, K, transp):
    """|Y - T^H X T| within the bound, T = tril(ud) or -- transp -- triu(ud); Im diag(Y) = 0.0 exactly"""
    for Tm, X, Y, (n, herm) in zip(pfe.split_blocks(ud, K), xs, pfe.split_blocks(y, K), pfe.block_list(K)):
        T = (np.triu(Tm) if transp else np.tril(Tm)).astype(CLD if herm else LD)
        E = T.conj().T @ X.astype(T.dtype) @ T
        g = gamma(LD(2 * n + 1 if herm else n + 1))
        Bd = g * (2 + g) * (_abs1(T).T @ _abs1(X) @ _abs1(T))
        off = ~np.eye(n, dtype=bool)
        for name, part in _planes(herm):
            _report("psdscale", n, herm, name, np.abs(part(Y).astype(LD) - part(E)), Bd, off if name == "Im" else np.ones((n, n), dtype=bool))
        if herm:
            assert not np.imag(Y).diagonal().any()
    assert np.isfinite(y).all()


def _poison(mats, where, K):
    """NaN (on both planes) at the entries where(n) of every block"""
    out = []
    for M in mats:
        M = np.array(M, dtype=complex if np.iscomplexobj(M) else float)
        n = M.shape[0]
        M[where(n)] = np.nan * (1 + 1j) if np.iscomplexobj(M) else np.nan
        out.append(M)
    return out


def _upper(n):
    return np.triu(np.ones((n, n), dtype=bool), 1)


def _lower(n):
    return np.tril(np.ones((n, n), dtype=bool), -1)


# ------------------------------------------------------------------------------------------------ a case
def check_case(kw, spectrum):
    """the values, and checks 1, 2, 3 (lengths, repeats) and 6 on one case"""
    from sedumi_amd import mex
    c = make_case(kw, spectrum)
    K = c["K"]
    ux, ispos = mex.psdfactor(c["x"], K, nlhs=2)
    assert ispos is True and ux.shape == (c["x"].size, 1) and mex.psdfactor(c["x"], K).shape == ux.shape
    ux = ux.ravel()
    check_factor_value(c["xs"], ux, K)
    # 2: NaN in the strict upper triangle and in Im diag of x: the same bits
    px = _poison(c["xs"], _upper, K)
    for M in px:
        if np.iscomplexobj(M):
            M.imag[np.diag_indices(M.shape[0])] = np.nan
    uxp, ip = mex.psdfactor(pfe.pack_blocks(px, K), K, nlhs=2)
    assert ip is True and np.array_equal(ux, uxp.ravel())
    # 3: whole-cone length, two calls
    assert np.array_equal(ux, mex.psdfactor(np.concatenate(([np.nan], c["x"])), K).ravel())
    assert np.array_equal(ux, mex.psdfactor(c["x"], K).ravel())

    # psdinvscale with the device's own factor: a Hermitian x, then (check 4, on the well conditioned factor) a Gaussian one without symmetry
    for name in ("z", "g") if spectrum == "flat" else ("z",):
        xv, xm = c[name], c[name + "s"]
        y = mex.psdinvscale(ux, xv, K)
        assert y.shape == (ux.size, 1)
        y = y.ravel()
        check_invscale_value(ux, xm, y, K)
        udp = pfe.pack_blocks(_poison(pfe.split_blocks(ux, K), _lower, K), K)                 # 2: NaN below the diagonal of ud
        assert np.array_equal(y, mex.psdinvscale(udp, xv, K).ravel())
        assert np.array_equal(y, mex.psdinvscale(ux, np.concatenate(([np.nan], xv)), K).ravel())
        assert np.array_equal(y, mex.psdinvscale(ux, xv, K).ravel())

    # psdscale on the device's own factor, both triangles
    for transp in (False, True):
        s = mex.psdscale_u(ux, c["z"], K, transp)
        assert s.shape == (ux.size, 1)
        s = s.ravel()
        check_scale_value(ux, c["zs"], s, K, transp)
        udp = pfe.pack_blocks(_poison(pfe.split_blocks(ux, K), _lower if transp else _upper, K), K)
        assert np.array_equal(s, mex.psdscale_u(udp, c["z"], K, transp).ravel())
        assert np.array_equal(s, mex.psdscale_u(ux, np.concatenate(([np.nan], c["z"])), K, transp).ravel())

    # 6: the fused call
    check_fused(c["x"], c["z"], K)
    return ux


def check_fused(x, z, K):
    from sedumi_amd import mex
    ux, ispos = mex.psdfactor(x, K, nlhs=2)
    s = mex.psdscale_u(ux, z, K)
    fu, fs, fi = mex.trydif_psd(x, z, K)
    assert fi is ispos and fu.shape == ux.shape and fs.shape == s.shape
    assert np.array_equal(fu, ux) and np.array_equal(fs, s)
    lu, ls, li = mex.trydif_psd(np.concatenate(([np.nan], x)), np.concatenate(([np.nan], z)), K)
    assert li is ispos and np.array_equal(lu, ux) and np.array_equal(ls, s)
    return ux.ravel(), s.ravel(), ispos


def check_block_alone():
    """check 3: the block of order 65 alone gives the bits it has inside s=[129, 3, 65]"""
    from sedumi_amd import mex
    c = make_case(dict(s=[129, 3, 65]), "flat")
    K1 = make_K(dict(s=[65]))
    x1, z1 = c["xs"][2].ravel(order="F"), c["zs"][2].ravel(order="F")
    u3 = mex.psdfactor(c["x"], c["K"]).ravel()
    u1 = mex.psdfactor(x1, K1).ravel()
    assert np.array_equal(u3[-65 * 65:], u1) and np.abs(u1).max() > 0
    y3 = mex.psdinvscale(u3, c["z"], c["K"]).ravel()
    y1 = mex.psdinvscale(u1, z1, K1).ravel()
    assert np.array_equal(y3[-65 * 65:], y1) and np.abs(y1).max() > 0


def check_lengths_are_refused():
    """check 3: len < lenud raises; K.s empty returns the .m files' empty answers.  Needs no device: refused before anything is allocated."""
    import ctypes as C
    import pytest
    from sedumi_amd import capi, mex, problem
    from sedumi_amd.capi import SdmError
    K = problem.make_K(1, [], [4])
    one = np.ones(16)
    for call in (lambda: mex.psdfactor(np.ones(15), K), lambda: mex.psdinvscale(one, np.ones(15), K), lambda: mex.psdinvscale(np.ones(15), one, K),
                 lambda: mex.psdinvscale(np.ones(17), one, K), lambda: mex.psdscale_u(one, np.ones(15), K), lambda: mex.psdscale_u(np.ones(17), one, K),
                 lambda: mex.trydif_psd(np.ones(15), np.ones(15), K), lambda: mex.trydif_psd(one, np.ones(17), K)):
        with pytest.raises(SdmError, match="size mismatch"):
            call()
    Kc, keep = capi.make_cone(1, [], [4], 1)
    L, ip = capi.lib(), C.c_int(7)
    for rc in (L.sdm_psdfactor(C.byref(Kc), capi.pf(one), C.c_int64(15), capi.pf(one), C.byref(ip)),
               L.sdm_psdinvscale(C.byref(Kc), capi.pf(one), capi.pf(one), C.c_int64(15), capi.pf(one)),
               L.sdm_psdscale(C.byref(Kc), capi.pf(one), capi.pf(one), C.c_int64(15), C.c_int(0), capi.pf(one)),
               L.sdm_trydif_psd(C.byref(Kc), capi.pf(one), capi.pf(one), C.c_int64(15), capi.pf(one), capi.pf(one), C.byref(ip))):
        assert rc != 0 and b"size mismatch" in L.sdm_last_error()
    K0 = problem.make_K(3, [3], [])
    ux, ispos = mex.psdfactor(np.ones(6), K0, nlhs=2)
    assert ux.shape == (0, 1) and ispos is True
    assert mex.psdinvscale(np.zeros(0), np.ones(6), K0).size == 0 and mex.psdscale_u(np.zeros(0), np.ones(6), K0).size == 0
    fu, fs, fi = mex.trydif_psd(np.ones(6), np.ones(6), K0)
    assert fu.size == 0 and fs.size == 0 and fi is True


# ------------------------------------------------------------------------------------------------ check 5: not positive definite
def _minus4(X, p):
    X = X.copy()
    X[p, p] -= 4.0                                                        # lambda in [1, 2]: pivot p is <= -2, the leading p x p block is untouched
    return X


def check_not_positive_definite(kw, p):
    """one block, X - 4 e_p e_p^T: ispos is False and ux all 0.0; the fused call agrees"""
    from sedumi_amd import mex
    c = make_case(kw, "flat")
    K = c["K"]
    x = pfe.pack_blocks([_minus4(c["xs"][0], p)], K)
    ux, ispos = mex.psdfactor(x, K, nlhs=2)
    assert ispos is False and ux.shape == (x.size, 1) and not ux.any() and not np.signbit(ux).any()
    _, s, _ = check_fused(x, c["z"], K)
    assert np.isfinite(s).all()


def check_bad_block_in_a_list():
    """s=[65, 129, 64], block 1 bad at p = 64: block 0 has the bits it has alone, everything from block 1's offset on is exactly 0.0; the same with
    x_pp = NaN; the fused call is bit-equal to the two single calls on it"""
    from sedumi_amd import mex
    c = make_case(dict(s=[65, 129, 64]), "flat")
    K = c["K"]
    alone = mex.psdfactor(c["xs"][0].ravel(order="F"), make_K(dict(s=[65]))).ravel()
    good = mex.psdfactor(c["x"], K).ravel()
    assert np.array_equal(good[:65 * 65], alone) and good[65 * 65:].all()
    nanpp = c["xs"][1].copy()
    nanpp[64, 64] = np.nan
    for X1 in (_minus4(c["xs"][1], 64), nanpp):
        x = pfe.pack_blocks([c["xs"][0], X1, c["xs"][2]], K)
        ux, ispos = mex.psdfactor(x, K, nlhs=2)
        ux = ux.ravel()
        assert ispos is False and np.array_equal(ux[:65 * 65], alone)
        assert not ux[65 * 65:].any() and not np.signbit(ux[65 * 65:]).any()
        fu, fs, _ = check_fused(x, c["z"], K)
        assert np.isfinite(fs).all() and fs[:65 * 65].any() and not fs[65 * 65:].any()


# ------------------------------------------------------------------------------------------------ check 8: the driver
def check_driver_switch():
    """solve(..., device_fact=True) on the problem of urot_exact.check_driver_switch with that check's bounds (they are literals inside that function:
    restated here), alone and with the four other device switches; device_fact=False is the default run bit for bit"""
    from sedumi_amd.driver import solve
    from sedumi_amd.driver import loop as lp
    from sedumi_amd.driver.conemex import NativeMex
    assert NativeMex().device_fact is False and NativeMex(device_fact=True).device_fact is True and NativeMex(device_fact=True).device_updt is False
    r0 = solve(*pfe.small_hermitian_sdp(), hot=lp.HipHot())
    rf = solve(*pfe.small_hermitian_sdp(), hot=lp.HipHot(), device_fact=False)
    assert all(rf[k] == r0[k] for k in ("iter", "STOP", "cx", "by", "x0", "feasratio")) and repr(rf["rows"]) == repr(r0["rows"])   # the whole iteration log
    runs = []
    for kw in (dict(device_fact=True), dict(device_fact=True, device_cone=True, device_qr=True, device_rot=True, device_updt=True)):
        r1 = solve(*pfe.small_hermitian_sdp(), hot=lp.HipHot(), **kw)
        print(kw, "iter", r0["iter"], r1["iter"], "cx", r0["cx"], r1["cx"], "by", r0["by"], r1["by"])
        assert abs(r1["iter"] - r0["iter"]) <= 1 and r1["iter"] > 3
        assert abs(r1["cx"] - r0["cx"]) <= 1e-6 * abs(r0["cx"]) and abs(r1["by"] - r0["by"]) <= 1e-6 * abs(r0["by"])
        runs.append(r1)
    a, b = runs
    assert abs(a["cx"] - b["cx"]) <= 1e-6 * abs(a["cx"]) and abs(a["by"] - b["by"]) <= 1e-6 * abs(a["by"])
