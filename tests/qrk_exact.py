"""Shared by the qrK tests: the cases, `exact` = the reference's own unblocked algorithm (qrK.c:86-227) restated in
numpy.longdouble on the same input, the compiled reference's answer and the checks of a case on whichever library capi is bound to.

Parts of a block of order n:  c (the lower trapezoid of columns 0 .. n-2), beta (n-1), triu(R) and, Hermitian blocks, the sign vector.
Accuracy rule per block and part:  err(library) <= 10 err(reference) + 1e-15,  err(v) = max|v - exact| / max|exact|."""
import numpy as np

import psd_frames_exact as pfe

LD, CLD = np.longdouble, np.clongdouble

CASES = [
    dict(s=[1]), dict(s=[2]), dict(hs=[1]), dict(hs=[2]),              # no reflector or one, the sign column alone
    dict(s=[15, 16, 17]), dict(s=[31, 32, 33]), dict(s=[63, 64, 65]),  # MFMA, panel and tile edges for a panel width of 16, 32 or 64
    dict(s=[130]),                                                     # several panels and tiles
    dict(s=[200, 3], hs=[66]),                                         # mixed list, offsets, a block without a trailing update beside one with many
    dict(hs=[70]),
    dict(s=[15, 16, 17], zero_col=True),                               # column n/2 zeroed: the beta = 1 identity reflector
    dict(s=[33, 65], zero_diag=True),                                  # M[0,0] = M[n/2,n/2] = 0: SIGN(0) = +1
]
GPU_ONLY_CASE = dict(s=[200, 200, 200], hs=[130])
GPU_ONLY_SEED = len(CASES)
RESIDENCE_CASE, RESIDENCE_SEED = dict(s=[65], hs=[33]), 40
# panel budgets of the residence check: every panel in global memory; the first panel of the order-65 block (65 x 32 doubles) and the
# Hermitian block's (2 x 33 x 32) in global memory, the second panel of the order-65 block (33 x 32 doubles = 8448 bytes) in LDS
RESIDENCE_BUDGETS = (1, 8448)


def exact_block(M):
    """qrfac / prpiqrfac (qrK.c:86-122, :142-227) in longdouble: dict(c, beta, R, sign)"""
    n = M.shape[0]
    herm = np.iscomplexobj(M)
    u = M.astype(CLD if herm else LD)
    c = np.zeros_like(u)
    beta = np.zeros(max(n - 1, 0), dtype=LD)
    for k in range(n - 1):
        xkk = u[k, k]
        if herm:
            absx, nrm = np.abs(xkk), np.sqrt(np.sum(np.abs(u[k:, k]) ** 2))
            ukk = -(xkk / absx) * nrm if absx > 0 else CLD(-nrm)
            c[k:, k] = u[k:, k]; c[k, k] = xkk - ukk
            beta[k] = nrm * (nrm + absx) if nrm != 0 else LD(1)
            u[k, k] = ukk
        else:
            dk = (LD(1) if xkk >= 0 else LD(-1)) * np.sqrt(np.sum(u[k:, k] ** 2))
            c[k:, k] = u[k:, k]; c[k, k] = xkk + dk
            beta[k] = dk * c[k, k] if dk * c[k, k] != 0 else LD(1)
            u[k, k] = -dk
        v = c[k:, k]
        u[k:, k + 1:] -= np.outer(v, (v.conj() @ u[k:, k + 1:]) / beta[k])
    out = dict(c=c[:, :max(n - 1, 0)], beta=beta, herm=herm)
    R = np.triu(u)
    if herm:
        d = np.diagonal(R).copy()
        sign = d / np.abs(d)
        R = R * sign.conj()[:, None]
        R[np.diag_indices(n)] = np.abs(d)
        out["sign"] = sign
    out["R"] = R
    return out


def exact_Qb(E):
    """Qb = Q_0 ... Q_{n-2} (diag(sign)) of exact_block's parts, in longdouble"""
    c, beta = E["c"], E["beta"]
    n = c.shape[0]
    Q = np.eye(n, dtype=c.dtype)
    for k in range(n - 2, -1, -1):
        v = c[k:, k]
        Q[k:, :] -= np.outer(v, (v.conj() @ Q[k:, :]) / beta[k])
    return Q * E["sign"][None, :] if E["herm"] else Q


def split_q(q, K):
    """the compact frames q (lenud + hLen) as per-block (C planes as a real / complex n x n matrix, beta of length n)"""
    q = np.asarray(q, dtype=np.float64).ravel()
    out, o = [], 0
    for n, herm in pfe.block_list(K):
        nn = n * n
        if herm:
            C = q[o:o + nn].reshape(n, n, order="F") + 1j * q[o + nn:o + 2 * nn].reshape(n, n, order="F")
            out.append((C, q[o + 2 * nn:o + 2 * nn + n].copy())); o += 2 * nn + n
        else:
            C = q[o:o + nn].reshape(n, n, order="F").copy(); o += nn
            out.append((C, C[:, n - 1].copy()))
    assert o == q.size
    return out


def parts(q, r, K):
    """per block dict(c, beta, R[, sign]) of a library's / the reference's output"""
    out = []
    for (C, b), R, (n, herm) in zip(split_q(q, K), pfe.split_blocks(np.asarray(r, dtype=np.float64).ravel(), K), pfe.block_list(K)):
        d = dict(c=np.tril(C)[:, :n - 1], beta=b[:n - 1], R=np.triu(R))
        if herm:
            d["sign"] = C[:, n - 1].copy()
        out.append(d)
    return out


def zero_mask(n, herm):
    """the entries of a block's q the reference leaves at its initial zero, as a boolean vector over the block's part of q"""
    U = np.triu(np.ones((n, n), dtype=bool), 1); U[:, n - 1:] = False
    if herm:
        b = np.zeros(n, dtype=bool); b[n - 1] = True                  # beta_{n-1}
        return np.concatenate((U.ravel(order="F"), U.ravel(order="F"), b))
    U[n - 1, n - 1] = True
    return U.ravel(order="F")


def err(v, e):
    e = np.asarray(e)
    if e.size == 0:
        return 0.0
    return float(np.max(np.abs(np.asarray(v).astype(e.dtype) - e)) / np.max(np.abs(e)))


_cache = {}


def make_case(refmex, kw, seed):
    """Inputs, the reference's answer and the longdouble one: computed once per session, shared by the emulator and the device tests."""
    key = (repr(sorted(kw.items())), seed)
    if key in _cache:
        return _cache[key]
    from sedumi_amd import problem
    K = problem.make_K(1, [], kw.get("s", []), hs=kw.get("hs", ()))
    rng = np.random.default_rng(seed)
    mats = []
    for n, herm in pfe.block_list(K):
        M = rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if herm else 0)
        if kw.get("zero_col"):
            M[:, n // 2] = 0.0
        if kw.get("zero_diag"):
            M[0, 0] = 0.0; M[n // 2, n // 2] = 0.0
        mats.append(M)
    x = pfe.pack_blocks(mats, K)
    qref, rref = refmex.call("qrK", 2, x.reshape(-1, 1), K)
    qref, rref = np.asarray(qref, dtype=np.float64).ravel(), np.asarray(rref, dtype=np.float64).ravel()
    lab = 10.0 ** rng.uniform(-3, 3, sum(n for n, _ in pfe.block_list(K)))
    E = [exact_block(M) for M in mats]
    c = dict(K=K, mats=mats, x=x, qref=qref, rref=rref, lab=lab, E=E, pref=parts(qref, rref, K))
    for v in (x, qref, rref, lab):
        v.setflags(write=False)
    _cache[key] = c
    return c


def check_rule(what, plib, c):
    """check 1: per block and part"""
    K = c["K"]
    bad = []
    for (n, herm), L, Rf, E in zip(pfe.block_list(K), plib, c["pref"], c["E"]):
        for part in ("c", "beta", "R") + (("sign",) if herm else ()):
            a, b = err(L[part], E[part]), err(Rf[part], E[part])
            print("%-14s n=%-4d %s %-5s library %.2e  reference %.2e" % (what, n, "herm" if herm else "real", part, a, b))
            if not a <= 10 * b + 1e-15:
                bad.append((what, n, herm, part, a, b))
    assert not bad, bad


def backward(q, r, c):
    """per block (max|Qb triu(R) - X| / max|X|, max|Qb^H Qb - I|), Qb rebuilt in longdouble from the compact frame q"""
    K = c["K"]
    out = []
    for Q, R, M in zip(pfe.exact_frames(q, K), pfe.split_blocks(np.asarray(r, dtype=np.float64).ravel(), K), c["mats"]):
        Rl, Ml = np.triu(R).astype(Q.dtype), M.astype(Q.dtype)
        out.append((float(np.max(np.abs(Q @ Rl - Ml)) / np.max(np.abs(Ml))), float(np.max(np.abs(Q.conj().T @ Q - np.eye(Q.shape[0]))))))
    return out


def check_backward(q, r, c):
    """check 2"""
    for (n, herm), (a1, a2), (b1, b2) in zip(pfe.block_list(c["K"]), backward(q, r, c), backward(c["qref"], c["rref"], c)):
        print("backward       n=%-4d %s  |Qb R - X| library %.2e reference %.2e   |Qb^H Qb - I| library %.2e reference %.2e" %
              (n, "herm" if herm else "real", a1, b1, a2, b2))
        assert a1 <= 10 * b1 + 1e-15 and a2 <= 10 * b2 + 1e-15, (n, herm, a1, b1, a2, b2)


def check_structure(q, r, c):
    """check 3"""
    K = c["K"]
    o = 0
    for n, herm in pfe.block_list(K):
        mk = zero_mask(n, herm)
        assert np.array_equal(q[o:o + mk.size][mk], c["qref"][o:o + mk.size][mk]) and not c["qref"][o:o + mk.size][mk].any()
        o += mk.size
    assert o == q.size
    for R, (n, herm) in zip(pfe.split_blocks(r, K), pfe.block_list(K)):
        assert not np.tril(np.real(R), -1).any()
        if herm:
            assert not np.tril(np.imag(R), -1).any() and not np.imag(R).diagonal().any() and (np.real(R).diagonal() >= 0).all()


def exact_chain(c):
    """X = Qb^H diag(lab) Qb with the exact Qb (check 6)"""
    if "X" not in c:
        c["X"] = pfe.exact_frameit([exact_Qb(E) for E in c["E"]], c["lab"])
    return c["X"]


def check_case(refmex, kw, seed, full=None):
    """Checks 1 - 6 of a case (5: the repeated call); above 20000 matrix entries, where the emulator needs seconds per call, the rule only."""
    from sedumi_amd import mex
    c = make_case(refmex, kw, seed)
    K = c["K"]
    if full is None:
        full = c["x"].size <= 20000
    q, r = mex.qrK(c["x"], K, nlhs=2)
    q, r = q.ravel(), r.ravel()
    check_rule("qrK", parts(q, r, K), c)
    if not full:
        return
    check_backward(q, r, c)
    check_structure(q, r, c)
    qe, re_ = mex.qrK(c["x"], K, nlhs=2, frame_kind=mex.FRAME_EXPLICIT)
    assert np.array_equal(qe.ravel(), mex.psdframe_explicit(q, K).ravel()) and np.array_equal(re_.ravel(), r)
    q2, r2 = mex.qrK(c["x"], K, nlhs=2)
    assert np.array_equal(q2.ravel(), q) and np.array_equal(r2.ravel(), r)
    assert np.array_equal(mex.qrK(c["x"], K).ravel(), q)                # r not asked for
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)
    if "Xref" not in c:
        c["Xref"] = np.asarray(refmex.call("psdframeit", 1, col(c["lab"]), col(c["qref"]), K)).ravel()
    pfe.check_rule("qrK -> psdframeit", mex.psdframeit(c["lab"], q, K).ravel(), c["Xref"], exact_chain(c), K)


def check_block_alone(refmex):
    """check 5: the block of order 65 factored alone gives the same bits as inside s=[200, 3, 65]"""
    from sedumi_amd import mex, problem
    rng = np.random.default_rng(77)
    mats = [rng.standard_normal((n, n)) for n in (200, 3, 65)]
    K3, K1 = problem.make_K(1, [], [200, 3, 65]), problem.make_K(1, [], [65])
    q3, r3 = mex.qrK(pfe.pack_blocks(mats, K3), K3, nlhs=2)
    q1, r1 = mex.qrK(pfe.pack_blocks(mats[2:], K1), K1, nlhs=2)
    assert np.array_equal(q3.ravel()[-65 * 65:], q1.ravel()) and np.array_equal(r3.ravel()[-65 * 65:], r1.ravel())
    assert np.abs(q1).max() > 0


def check_residences(refmex):
    """check 5: with the panel forced into global memory (all panels; the first panel only) the same bits as by default, and the rule"""
    from sedumi_amd import mex
    c = make_case(refmex, RESIDENCE_CASE, RESIDENCE_SEED)
    K = c["K"]
    q0, r0 = mex.qrK(c["x"], K, nlhs=2)
    got = []
    try:
        for budget in RESIDENCE_BUDGETS:
            mex.set_qr_panel_lds_budget(budget)
            got.append(mex.qrK(c["x"], K, nlhs=2))
    finally:
        mex.set_qr_panel_lds_budget(0)
    for q1, r1 in got:
        assert np.array_equal(q0, q1) and np.array_equal(r0, r1)
    check_rule("qrK residences", parts(q0.ravel(), r0.ravel(), K), c)
    check_backward(q0.ravel(), r0.ravel(), c)


def check_driver_switch():
    """solve() of a small SDP with a real and a Hermitian block, qrK through the library (explicit frames, the reference's sign convention
    for R) against the default driver; and with psdframeit / psdinvjmul through the library as well"""
    from sedumi_amd.driver import solve
    from sedumi_amd.driver import loop as lp
    from sedumi_amd.driver.conemex import NativeMex
    assert NativeMex().device_qr is False and NativeMex(device_qr=True).device_qr is True and NativeMex(device_qr=True).device_cone is False
    r0 = solve(*pfe.small_hermitian_sdp(), hot=lp.HipHot())
    for kw in (dict(device_qr=True), dict(device_qr=True, device_cone=True)):
        r1 = solve(*pfe.small_hermitian_sdp(), hot=lp.HipHot(), **kw)
        print(kw, "iter", r0["iter"], r1["iter"], "cx", r0["cx"], r1["cx"], "by", r0["by"], r1["by"])
        assert abs(r1["iter"] - r0["iter"]) <= 1 and r1["iter"] > 3
        assert abs(r1["cx"] - r0["cx"]) <= 1e-6 * abs(r0["cx"]) and abs(r1["by"] - r0["by"]) <= 1e-6 * abs(r0["by"])
        assert abs(r1["cx"] - r1["by"]) <= 1e-6 * (1 + abs(r1["cx"]))
