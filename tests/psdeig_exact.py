"""Shared by the psdeig / minpsdeig tests: the cases, the three residuals of an eigendecomposition evaluated in numpy.longdouble for
the library's result AND for numpy.linalg.eigh (LAPACK, the solver the reference's eig and the driver use) on the same input, and the checks of a
case on whichever library capi is bound to.

A block is X = Q diag(lambda) Q^H / 2 with Q re-orthogonalised and the product formed in longdouble, rounded once; A = X + X^H, u = 2^-53:
    r1 = ||A Q^ - Q^ diag(2 lab)||_F / (n u ||A||_2)        r2 = ||Q^^H Q^ - I||_F / (n u)        r3 = max |2 lab - sort(lambda)| / (n u ||A||_2)
(r3 after the u || |A| ||_F by which rounding the input may move an eigenvalue has been taken off).  The limit of each is M max(r_i(LAPACK), 1):
a Jacobi method applies sweeps x steps 64-wide updates to every column where Householder + QR pass over the data a fixed number of times, and the
shift adds a factor ||B|| / ||A||.  M is measured, not chosen: the next power of two above twice the worst r_i(device) / max(r_i(LAPACK), 1) over all
cases, on the emulator and on the MI355X (the per-case values: profiles/), and must not exceed 256.

    worst r_i(device) / max(r_i(LAPACK), 1) seen: emulator 66.9 (r1, s=[129], log-spaced), MI355X 119.9 (r1, order 200 of s=[200,200,200] hs=[130],
    the +-1 spectrum): M = 256, the next power of two above 2 x 119.9"""
import numpy as np

import psd_frames_exact as pfe
import triu_exact as te

LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53
M = 256
make_K = te.make_K

CASES = [
    dict(s=[1]), dict(s=[2]), dict(hs=[1]), dict(hs=[2]),              # smallest orders
    dict(s=[31, 32, 33]),                                              # one column block against two
    dict(s=[63, 64, 65]),                                              # nb = 2, 2, 3: a bye, and one pair against a ragged third block
    dict(s=[129]),                                                     # nb = 5: odd, several steps, a one-column block
    dict(hs=[33]),
    dict(s=[65], hs=[33]),                                             # Hermitian beside real
]
GPU_ONLY_CASE = dict(s=[200, 200, 200], hs=[130])
SPECTRA = ("flat", "log", "sym", "pm")

_cache = {}


def _ro(v):
    v.setflags(write=False)
    return v


def spectrum(name, n):
    if name == "flat":
        return np.linspace(1.0, 2.0, n)
    if name == "log":
        return np.logspace(0.0, -8.0, n)
    if name == "sym":
        return np.linspace(-1.0, 1.0, n)
    lam = np.ones(n)                                                   # "pm": +1 on half, -1 on the rest
    lam[n // 2:] = -1.0
    return lam


def block(rng, n, herm, name):
    """X = Q diag(lambda) Q^H / 2 rounded once from longdouble, and sort(lambda)"""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if herm else 0))
    Q = Q.astype(CLD if herm else LD)
    I = np.eye(n, dtype=Q.dtype)
    for _ in range(2):                                                 # Newton-Schulz: Q^H Q - I from 1e-15 to below the longdouble unit
        Q = Q @ (3 * I - Q.conj().T @ Q) / 2
    lam = rng.permutation(spectrum(name, n))
    X = (Q * lam.astype(LD)) @ Q.conj().T / 2
    return X.astype(complex if herm else float), np.sort(lam)


def make_case(kw, name, seed=1):
    key = (repr(sorted(kw.items())), name, seed)
    if key not in _cache:
        K = make_K(kw)
        rng = np.random.default_rng(seed)
        xs, lams = [], []
        for n, herm in pfe.block_list(K):
            X, lam = block(rng, n, herm, name)
            xs.append(X); lams.append(lam)
        _cache[key] = dict(K=K, kw=kw, xs=xs, lams=lams, x=_ro(pfe.pack_blocks(xs, K)))
    return _cache[key]


def residuals(X, lam2, Q, lam):
    """(r1, r2, r3) of the decomposition (lam2 = the eigenvalues of A = X + X^H as returned, Q) in longdouble; lam: the exact eigenvalues, sorted"""
    n = X.shape[0]
    cplx = np.iscomplexobj(X)
    A = X.astype(CLD if cplx else LD)
    A = A + A.conj().T
    Ad = A.astype(complex if cplx else float)
    nrm = LD(np.abs(np.linalg.eigvalsh(Ad)).max())
    Ql, l2 = Q.astype(A.dtype), lam2.astype(LD)
    r1 = np.sqrt((np.abs(A @ Ql - Ql * l2) ** 2).sum()) / (n * U * nrm)
    r2 = np.sqrt((np.abs(Ql.conj().T @ Ql - np.eye(n)) ** 2).sum()) / (n * U)
    moved = U * np.sqrt((np.abs(A) ** 2).sum())
    r3 = max(LD(0), np.abs(l2 - lam.astype(LD)).max() - moved) / (n * U * nrm)
    return float(r1), float(r2), float(r3)


def check_values(c, lab, q, what="psdeig"):
    """the three residuals of every block against M max(r_i(LAPACK), 1), each printed before it is asserted; check 1: lab ascending.  Returns the worst
    r_i(device) / max(r_i(LAPACK), 1)"""
    K, worst, o = c["K"], 0.0, 0
    failed = []
    for X, lam, Q, (n, herm) in zip(c["xs"], c["lams"], pfe.split_blocks(q, K), pfe.block_list(K)):
        l = lab[o:o + n]; o += n
        assert np.isfinite(l).all() and np.isfinite(Q).all()
        assert (np.diff(l) >= 0).all()
        rd = residuals(X, 2 * l, Q, lam)
        w, QL = np.linalg.eigh(X + X.conj().T)
        rl = residuals(X, w, QL, lam)
        ratio = [d / max(r, 1.0) for d, r in zip(rd, rl)]
        print("%-7s n=%-4d %s  device r1 %.2f r2 %.2f r3 %.2f   LAPACK r1 %.2f r2 %.2f r3 %.2f   ratio %.2f" %
              (what, n, "herm" if herm else "real", *rd, *rl, max(ratio)))
        worst = max(worst, max(ratio))
        if max(ratio) > M:
            failed.append((n, herm, rd, rl))
    assert not failed, failed
    return worst


# ------------------------------------------------------------------------------------------------ a case
def check_case(kw, name):
    """the values; checks 1 (ascending), 2 (values-only and the minimum bit for bit), 5 (repeats), 6 (whole-cone length)"""
    from sedumi_amd import mex
    c = make_case(kw, name)
    K, x = c["K"], c["x"]
    lab, q, info = mex.psdeig(x, K, nlhs=3)
    nsum = sum(n for n, _ in pfe.block_list(K))
    assert info == -1 and lab.shape == (nsum, 1) and q.shape == (x.size, 1)
    print(kw, name, "sweeps", mex.psdeig_last_sweeps())
    lab, q = lab.ravel(), q.ravel()
    worst = check_values(c, lab, q)
    lab1 = mex.psdeig(x, K)
    assert lab1.shape == (nsum, 1) and np.array_equal(lab1.ravel(), lab)
    m, mi = mex.minpsdeig(np.concatenate(([np.nan], x)), K, nlhs=2)                        # (a whole-cone length)
    assert mi == -1 and m.shape == (1, 1) and m[0, 0] == lab.min()
    if nsum <= 100 or capi_is_device():                                                    # (the emulator takes seconds per solve of the larger cases)
        l2, q2 = mex.psdeig(np.concatenate(([np.nan, 3.0], x)), K, nlhs=2)
        assert np.array_equal(l2.ravel(), lab) and np.array_equal(q2.ravel(), q)
        l3, q3 = mex.psdeig(x, K, nlhs=2)
        assert np.array_equal(l3.ravel(), lab) and np.array_equal(q3.ravel(), q)
        assert np.array_equal(m, mex.minpsdeig(x, K))
    return worst


def capi_is_device():
    from sedumi_amd import capi
    return capi.backend() != "emu"


def check_zero_one():
    """the explicit [[0,1],[1,0]]: a sign-based Hestenes returns 0, 0 (its columns are orthogonal already)"""
    from sedumi_amd import mex
    for kw in (dict(s=[2]), dict(hs=[2])):
        K = make_K(kw)
        X = np.array([[0.0, 1.0], [1.0, 0.0]]) + (0j if "hs" in kw else 0)
        lab, q = mex.psdeig(pfe.pack_blocks([X], K), K, nlhs=2)
        c = dict(K=K, xs=[X], lams=[np.array([-2.0, 2.0])])
        check_values(c, lab.ravel(), q.ravel(), "zero-one")
        assert np.abs(lab.ravel() - [-1.0, 1.0]).max() <= 8 * U


def check_diagonal():
    """check 3: a diagonal X with distinct entries in scrambled order: q is exactly the sorting permutation, lab within 2 u sigma of the sorted
    half-diagonal... of A = 2 X, that is of the sorted diagonal of X.  sigma is the library's shift, 1.5 x a bound of ||A||_2 that is <= the largest
    absolute row sum: 3 max |x_ii| at most"""
    from sedumi_amd import mex
    for kw in (dict(s=[65]), dict(hs=[33])):
        K = make_K(kw)
        (n, herm), = pfe.block_list(K)
        d = np.random.default_rng(3).permutation(np.linspace(-1.0, 2.0, n))
        X = np.diag(d) + (0j if herm else 0)
        lab, q = mex.psdeig(pfe.pack_blocks([X], K), K, nlhs=2)
        lab, Q = lab.ravel(), pfe.split_blocks(q.ravel(), K)[0]
        order = np.argsort(d)
        P = np.zeros((n, n)); P[order, np.arange(n)] = 1.0
        assert np.array_equal(np.real(Q), P) and not np.imag(Q).any()
        assert np.abs(lab - d[order]).max() <= 2 * U * 3 * np.abs(d).max()
        assert mex.psdeig_last_sweeps() == 1


def check_imag_diagonal_ignored():
    """check 4: Im of a Hermitian block's input diagonal is not read"""
    from sedumi_amd import mex
    c = make_case(dict(s=[65], hs=[33]), "sym")
    K = c["K"]
    lab, q = mex.psdeig(c["x"], K, nlhs=2)
    Xh = c["xs"][1].copy()
    Xh.imag[np.diag_indices(33)] = np.nan
    xp = pfe.pack_blocks([c["xs"][0], Xh], K)
    assert np.isnan(xp).sum() == 33
    lp, qp = mex.psdeig(xp, K, nlhs=2)
    assert np.array_equal(lp, lab) and np.array_equal(qp, q)
    assert np.array_equal(mex.minpsdeig(xp, K), mex.minpsdeig(c["x"], K))


def check_block_alone():
    """check 5: the block of order 65 alone gives the bits it has inside s=[129, 3, 65]"""
    from sedumi_amd import mex
    c = make_case(dict(s=[129, 3, 65]), "sym")
    K1 = make_K(dict(s=[65]))
    l3, q3 = mex.psdeig(c["x"], c["K"], nlhs=2)
    l1, q1 = mex.psdeig(c["xs"][2].ravel(order="F"), K1, nlhs=2)
    assert np.array_equal(l3.ravel()[-65:], l1.ravel()) and np.array_equal(q3.ravel()[-65 * 65:], q1.ravel()) and np.abs(q1).max() > 0


def check_lengths_are_refused():
    """check 6: len < lenud raises, also without a device; an empty K.s returns empty"""
    import ctypes as C
    import pytest
    from sedumi_amd import capi, mex, problem
    from sedumi_amd.capi import SdmError
    K = problem.make_K(1, [], [4])
    for call in (lambda: mex.psdeig(np.ones(15), K), lambda: mex.psdeig(np.ones(15), K, nlhs=2), lambda: mex.minpsdeig(np.ones(15), K)):
        with pytest.raises(SdmError, match="size mismatch"):
            call()
    Kc, keep = capi.make_cone(1, [], [4], 1)
    L, one, info, m = capi.lib(), np.ones(16), C.c_int(7), C.c_double(0.0)
    for rc in (L.sdm_psdeig(C.byref(Kc), capi.pf(one), C.c_int64(15), capi.pf(one), capi.pf(one), C.byref(info)),
               L.sdm_minpsdeig(C.byref(Kc), capi.pf(one), C.c_int64(15), C.byref(m), C.byref(info))):
        assert rc != 0 and b"size mismatch" in L.sdm_last_error()
    K0 = problem.make_K(3, [3], [])
    assert mex.psdeig(np.ones(6), K0).size == 0 and mex.minpsdeig(np.ones(6), K0).size == 0
    lab, q = mex.psdeig(np.ones(6), K0, nlhs=2)
    assert lab.size == 0 and q.size == 0
    Kc0, keep0 = capi.make_cone(3, [3], [], 0)
    assert L.sdm_psdeig(C.byref(Kc0), capi.pf(one), C.c_int64(6), capi.pf(one), None, C.byref(info)) == 0 and info.value == -1


def check_nan_block_in_a_list():
    """check 7: s=[65, 129, 64] with a NaN in block 1: info = 1, lab and q of block 1 all NaN, blocks 0 and 2 bit-equal to their values without it.
    A handled path: the block is marked by the row-sum kernel and never enters a sweep."""
    from sedumi_amd import mex
    c = make_case(dict(s=[65, 129, 64]), "flat")
    K = c["K"]
    lab, q, info = mex.psdeig(c["x"], K, nlhs=3)
    assert info == -1
    X1 = c["xs"][1].copy()
    X1[100, 7] = np.nan
    x = pfe.pack_blocks([c["xs"][0], X1, c["xs"][2]], K)
    ln, qn, info = mex.psdeig(x, K, nlhs=3)
    assert info == 1 and mex.psdeig_last_sweeps() <= 30
    lab, q, ln, qn = lab.ravel(), q.ravel(), ln.ravel(), qn.ravel()
    a, b = 65 * 65, 65 * 65 + 129 * 129
    assert np.isnan(ln[65:194]).all() and np.isnan(qn[a:b]).all()
    assert np.array_equal(ln[:65], lab[:65]) and np.array_equal(ln[194:], lab[194:])
    assert np.array_equal(qn[:a], q[:a]) and np.array_equal(qn[b:], q[b:])
    assert np.array_equal(mex.psdeig(x, K).ravel(), ln, equal_nan=True)
    m, mi = mex.minpsdeig(x, K, nlhs=2)
    assert mi == 1 and np.isnan(m[0, 0])


# ------------------------------------------------------------------------------------------------ the driver
def check_driver_switch():
    """solve(..., device_eig=True) on the problem of urot_exact.check_driver_switch with that check's bounds (they are literals inside that function:
    restated here), alone and with the five other device switches; device_eig=False is the default run bit for bit"""
    from sedumi_amd.driver import solve
    from sedumi_amd.driver import loop as lp
    from sedumi_amd.driver.conemex import NativeMex
    assert NativeMex().device_eig is False and NativeMex(device_eig=True).device_eig is True and NativeMex(device_eig=True).device_fact is False
    r0 = solve(*pfe.small_hermitian_sdp(), hot=lp.HipHot())
    rf = solve(*pfe.small_hermitian_sdp(), hot=lp.HipHot(), device_eig=False)
    assert all(rf[k] == r0[k] for k in ("iter", "STOP", "cx", "by", "x0", "feasratio")) and repr(rf["rows"]) == repr(r0["rows"])   # the whole iteration log
    runs = []
    for kw in (dict(device_eig=True),
               dict(device_eig=True, device_cone=True, device_qr=True, device_rot=True, device_updt=True, device_fact=True)):
        r1 = solve(*pfe.small_hermitian_sdp(), hot=lp.HipHot(), **kw)
        print(kw, "iter", r0["iter"], r1["iter"], "cx", r0["cx"], r1["cx"], "by", r0["by"], r1["by"])
        assert abs(r1["iter"] - r0["iter"]) <= 1 and r1["iter"] > 3
        assert abs(r1["cx"] - r0["cx"]) <= 1e-6 * abs(r0["cx"]) and abs(r1["by"] - r0["by"]) <= 1e-6 * abs(r0["by"])
        runs.append(r1)
    a, b = runs
    assert abs(a["cx"] - b["cx"]) <= 1e-6 * abs(a["cx"]) and abs(a["by"] - b["by"]) <= 1e-6 * abs(a["by"])
