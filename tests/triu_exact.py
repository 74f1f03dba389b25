"""Shared by the triumtriu / updtransfo_psd tests: the cases, triumtriu.m:40-71 in numpy.longdouble and the checks of a case on
whichever library capi is bound to.  triumtriu has no compiled reference (it is an .m file): the expected value is the longdouble one.

Value bound, per entry (i, j), i <= j, of a block, m = j - i + 1 terms (k = i .. j), u = 2^-53, gamma_p = p u / (1 - p u):
    real block       |z - z_ld| <= gamma_{m+1}  sum_k |x_ik| |y_kj|
    Hermitian block  per plane  <= gamma_{2m+1} sum_k (|Re x_ik| + |Im x_ik|) (|Re y_kj| + |Im y_kj|)
the bound of a dot product of that length summed in any order, with or without FMA (Higham, Accuracy and Stability, section 3.1), + 1 for rounding
the longdouble value to double.  Derived, not measured; no margin on top."""
import numpy as np

import psd_frames_exact as pfe
import urot_exact as ue

LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53

# block shapes (problem.make_K(1, [], s, hs=hs)): the smallest at which the tile logic can go wrong
CASES = [
    dict(s=[1]), dict(s=[2]), dict(hs=[1]), dict(hs=[2]),
    dict(s=[63, 64, 65]),                                              # tile edge: one tile against two
    dict(s=[129]),                                                     # three tile rows: tile (0, 2) has a middle k-tile and a one-row edge
    dict(hs=[65]),
    dict(s=[70, 35]),                                                  # control07's orders
    dict(s=[5, 0, 3], hs=[4]),                                         # an empty block, and the offsets behind it
]
GPU_ONLY_CASE = dict(s=[200, 200, 200], hs=[130])
CHAIN_CASES = [dict(s=[5]), dict(hs=[2]), dict(s=[63, 64, 65]), dict(s=[70, 35]), dict(s=[65], hs=[33])]


def gamma(p):
    return p * U / (1 - p * U)


def make_K(kw):
    from sedumi_amd import problem
    return problem.make_K(1, [], kw.get("s", []), hs=kw.get("hs", ()))


_cache = {}


def make_case(kw, complex_diag, seed=1):
    """x, y with every block filled completely (the lower triangle too); the diagonal real and positive, or -- complex_diag -- complex on the
    Hermitian blocks; the longdouble answer and the bound of every entry.  Computed once per session, never modified."""
    key = (repr(sorted(kw.items())), complex_diag, seed)
    if key in _cache:
        return _cache[key]
    K = make_K(kw)
    rng = np.random.default_rng(seed)
    xs, ys, Z, Bnd = [], [], [], []
    for n, herm in pfe.block_list(K):
        pair = []
        for _ in range(2):
            M = rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if herm else 0)
            dg = np.abs(rng.standard_normal(n)) + 0.5
            M[np.diag_indices(n)] = dg + (1j * rng.standard_normal(n) if herm and complex_diag else 0)
            pair.append(M)
        X, Y = pair
        xs.append(X); ys.append(Y)
        ZZ = np.triu(X).astype(CLD if herm else LD) @ np.triu(Y).astype(CLD if herm else LD)          # triumtriu.m:63
        Z.append(ZZ + np.triu(ZZ, 1).conj().T)                                                       # :64
        ax = np.triu(np.abs(np.real(X)) + np.abs(np.imag(X))).astype(LD)
        ay = np.triu(np.abs(np.real(Y)) + np.abs(np.imag(Y))).astype(LD)
        i, j = np.indices((n, n))
        m = np.maximum(j - i + 1, 0)
        Bnd.append(gamma(((2 * m + 1) if herm else (m + 1)).astype(LD)) * (ax @ ay))
    c = dict(K=K, kw=kw, xs=xs, ys=ys, x=pfe.pack_blocks(xs, K), y=pfe.pack_blocks(ys, K), Z=Z, Bnd=Bnd)
    for v in (c["x"], c["y"]):
        v.setflags(write=False)
    _cache[key] = c
    return c


def check_value_and_mirror(c, z, complex_diag):
    """checks 1 and 2"""
    K = c["K"]
    for Zl, E, Bd, (n, herm) in zip(pfe.split_blocks(z, K), c["Z"], c["Bnd"], pfe.block_list(K)):
        up = np.triu(np.ones((n, n), dtype=bool))
        for name, part in (("Re", np.real),) + ((("Im", np.imag),) if herm else ()):
            dev = np.abs(part(Zl).astype(LD) - part(E))
            worst = float(np.max(np.where(up, dev / np.where(Bd > 0, Bd, 1), 0))) if n else 0.0
            print("triumtriu  n=%-4d %s %s  largest |z - z_ld| / bound %.3f" % (n, "herm" if herm else "real", name, worst))
            assert (dev[up] <= Bd[up]).all(), (n, herm, name, worst)
        lo = np.tril(np.ones((n, n), dtype=bool), -1)
        assert np.array_equal(np.real(Zl)[lo], np.real(Zl).T[lo])                                   # the mirror, bit for bit
        if herm:
            assert np.array_equal(np.imag(Zl)[lo], -np.imag(Zl).T[lo])
            if complex_diag and n:                                                                   # the Im diagonal is computed, not forced to 0
                assert np.imag(Zl).diagonal().any()
    assert np.isfinite(z).all()


def check_case(kw, complex_diag):
    """checks 1 - 3 and the lengths of 4 on one case"""
    from sedumi_amd import mex
    c = make_case(kw, complex_diag)
    K = c["K"]
    z = mex.triumtriu(c["x"], c["y"], K)
    assert z.shape == (c["x"].size, 1)
    z = z.ravel()
    check_value_and_mirror(c, z, complex_diag)
    # 3: NaN in the strict lower triangles of both operands: the same bits, all finite
    px, py = [], []
    for X, Y in zip(c["xs"], c["ys"]):
        n = X.shape[0]
        lo = np.tril(np.ones((n, n), dtype=bool), -1)
        X, Y = X.copy(), Y.copy()
        X[lo] = np.nan * (1 + 1j) if np.iscomplexobj(X) else np.nan
        Y[lo] = np.nan * (1 + 1j) if np.iscomplexobj(Y) else np.nan
        px.append(X); py.append(Y)
    zp = mex.triumtriu(pfe.pack_blocks(px, K), pfe.pack_blocks(py, K), K).ravel()
    assert np.isfinite(zp).all() and np.array_equal(z, zp)
    # 4: x, y at whole-cone length (K.l = 1 entry in front): the same bits as the PSD tails alone
    zl = mex.triumtriu(np.concatenate(([np.nan], c["x"])), np.concatenate(([7.0], c["y"])), K).ravel()
    assert np.array_equal(z, zl)
    assert np.array_equal(z, mex.triumtriu(c["x"], c["y"], K).ravel())                               # two calls, the same bits
    return z


def check_block_alone():
    """check 4: the block of order 65 alone gives the bits it has inside s=[129, 3, 65]"""
    from sedumi_amd import mex
    c = make_case(dict(s=[129, 3, 65]), False)
    z3 = mex.triumtriu(c["x"], c["y"], c["K"]).ravel()
    z1 = mex.triumtriu(c["xs"][2].ravel(order="F"), c["ys"][2].ravel(order="F"), make_K(dict(s=[65]))).ravel()
    assert np.array_equal(z3[-65 * 65:], z1) and np.abs(z1).max() > 0


def check_lengths_are_refused():
    """check 4: len < lenud and x, y of different sizes raise; K.s empty returns an empty result.  Needs no device: refused before anything is allocated."""
    import pytest
    from sedumi_amd import mex, problem
    from sedumi_amd.capi import SdmError
    K = problem.make_K(1, [], [4])
    with pytest.raises(SdmError, match="size mismatch"):
        mex.triumtriu(np.ones(15), np.ones(15), K)
    with pytest.raises(SdmError, match="size mismatch"):
        mex.triumtriu(np.ones(16), np.ones(17), K)
    import ctypes as C
    from sedumi_amd import capi
    Kc, keep = capi.make_cone(1, [], [4], 1)
    one = np.ones(16)
    assert capi.lib().sdm_triumtriu(C.byref(Kc), capi.pf(one), capi.pf(one), C.c_int64(15), capi.pf(one)) != 0
    assert b"size mismatch" in capi.lib().sdm_last_error()
    K0 = problem.make_K(3, [3], [])
    assert mex.triumtriu(np.ones(6), np.ones(6), K0).size == 0
    u, p, f = mex.updtransfo_psd(np.zeros(0), np.zeros(0), None, np.zeros(0), np.ones(3 + 2), K0)
    assert u.size == 0 and p.size == 0 and f.size == 0
    with pytest.raises(SdmError, match="v size mismatch"):
        mex.updtransfo_psd(np.ones(16), np.ones(16), None, np.ones(16), np.ones(3), K)
    with pytest.raises(SdmError, match="q size mismatch"):
        mex.updtransfo_psd(np.ones(16), np.ones(16), None, np.ones(15), np.ones(4), K)
    with pytest.raises(SdmError, match="perm size mismatch"):
        mex.updtransfo_psd(np.ones(16), np.ones(16), np.ones(3), np.ones(16), np.ones(4), K)


# ------------------------------------------------------------------------------------------------ the fused chain
def make_chain(kw, seed=1):
    """ux, u_in upper triangular with a positive diagonal; q unitary, vlab in [0.5, 2] and perm a permutation per block -- urot_exact.make_case's
    construction of the chain's inputs (updtransfo.m:99-107)"""
    key = ("chain", repr(sorted(kw.items())), seed)
    if key in _cache:
        return _cache[key]
    K = make_K(kw)
    rng = np.random.default_rng(seed)
    tri, qm = [[], []], []
    for n, herm in pfe.block_list(K):
        for t in tri:
            M = np.triu(rng.standard_normal((n, n)))
            if herm:
                M = M + 1j * np.triu(rng.standard_normal((n, n)), 1)
            M[np.diag_indices(n)] = np.abs(np.real(np.diagonal(M))) + 0.5
            t.append(M)
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if herm else 0))
        qm.append(Q)
    slen = sum(n for n, _ in pfe.block_list(K))
    c = dict(K=K, ux=pfe.pack_blocks(tri[0], K), u=pfe.pack_blocks(tri[1], K), q=pfe.pack_blocks(qm, K), vlab=rng.uniform(0.5, 2.0, slen),
             perm=np.concatenate([1.0 + rng.permutation(n) for n, _ in pfe.block_list(K)]))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cache[key] = c
    return c


def compose(c, perm, frame_kind):
    """updtransfo.m:99-108 through the single calls"""
    from sedumi_amd import mex
    K = c["K"]
    du = mex.triumtriu(c["ux"], c["u"], K)
    du, po, gjc, g = mex.urotorder(du, K, ue.MAXU, perm)
    q = mex.givensrot(gjc, g, c["q"], K)
    vinv = mex.sqrtinv(q, c["vlab"], K)
    frs, r = mex.qrK(vinv, K, nlhs=2, frame_kind=frame_kind)
    return mex.triumtriu(r, du, K), po, frs


def check_chain(kw, full=None):
    """check 5: the fused call bit-equal to the composition, both frame kinds, with and without perm_in, and under urot_exact.RESIDENCE_BUDGETS.
    full: every combination of the three; otherwise (the default above 2000 matrix entries, where the emulator needs a second per chain) each
    frame kind and each form of perm_in once, and the budgets on the case they were made for (urot_exact.RESIDENCE_CASE)."""
    from sedumi_amd import mex
    c = make_chain(kw)
    K = c["K"]
    if full is None:
        full = c["ux"].size <= 2000
    H, E = mex.FRAME_HOUSEHOLDER, mex.FRAME_EXPLICIT
    if full:
        combos = [(b, p, k) for b in (0,) + tuple(ue.RESIDENCE_BUDGETS) for p in (False, True) for k in (H, E)]
    else:
        combos = [(0, False, E), (0, True, H)] + ([(b, True, E) for b in ue.RESIDENCE_BUDGETS] if kw == ue.RESIDENCE_CASE else [])
    got = {}
    try:
        for budget, with_perm, kind in combos:
            mex.set_rot_lds_budget(budget)
            perm = c["perm"] if with_perm else None
            want = compose(c, perm, kind)
            got[budget, with_perm, kind] = g = mex.updtransfo_psd(c["ux"], c["u"], perm, c["q"], c["vlab"], K, maxu=ue.MAXU, frame_kind=kind)
            for name, a, b in zip(("u", "perm", "frame"), g, want):
                assert a.shape == b.shape and np.array_equal(a, b), (kw, budget, with_perm, kind, name)
            assert np.isfinite(g[0]).all() and np.abs(g[0]).max() > 0
    finally:
        mex.set_rot_lds_budget(0)
    # the whole spectral vector for vlab (K.l = 1 entry in front), whole-cone ux and u, an empty perm for none: the same bits
    b = mex.updtransfo_psd(np.concatenate(([3.0], c["ux"])), np.concatenate(([3.0], c["u"])), np.zeros(0), c["q"], np.concatenate(([1.0], c["vlab"])), K,
                           frame_kind=E)
    assert all(np.array_equal(v, w) for v, w in zip(got[0, False, E], b))


def check_chain_under_every_budget():
    """the residence case with the panel of qrK and the strips of the frame expansion out of LDS as well (qrk_exact / psd_frames_exact's budgets)"""
    import qrk_exact as qe
    from sedumi_amd import mex
    c = make_chain(ue.RESIDENCE_CASE)
    K = c["K"]
    want = compose(c, c["perm"], mex.FRAME_EXPLICIT)
    try:
        for rot, qr, fr in zip(ue.RESIDENCE_BUDGETS, qe.RESIDENCE_BUDGETS, (2112, 1024)):
            mex.set_rot_lds_budget(rot); mex.set_qr_panel_lds_budget(qr); mex.set_frame_lds_budget(fr)
            got = mex.updtransfo_psd(c["ux"], c["u"], c["perm"], c["q"], c["vlab"], K, frame_kind=mex.FRAME_EXPLICIT)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (rot, qr, fr)
    finally:
        mex.set_rot_lds_budget(0); mex.set_qr_panel_lds_budget(0); mex.set_frame_lds_budget(0)


def check_driver_switch():
    """check 7: solve(..., device_updt=True) on the problem of urot_exact.check_driver_switch with that check's bounds (they are literals inside that
    function: restated here), alone and with the other device switches; device_updt=False is the default run bit for bit"""
    from sedumi_amd.driver import solve
    from sedumi_amd.driver import loop as lp
    from sedumi_amd.driver.conemex import NativeMex
    assert NativeMex().device_updt is False and NativeMex(device_updt=True).device_updt is True and NativeMex(device_updt=True).device_rot is False
    r0 = solve(*pfe.small_hermitian_sdp(), hot=lp.HipHot())
    rf = solve(*pfe.small_hermitian_sdp(), hot=lp.HipHot(), device_updt=False)
    assert all(rf[k] == r0[k] for k in ("iter", "STOP", "cx", "by", "x0", "feasratio")) and repr(rf["rows"]) == repr(r0["rows"])   # the whole iteration log
    for kw in (dict(device_updt=True), dict(device_updt=True, device_cone=True, device_qr=True, device_rot=True)):
        r1 = solve(*pfe.small_hermitian_sdp(), hot=lp.HipHot(), **kw)
        print(kw, "iter", r0["iter"], r1["iter"], "cx", r0["cx"], r1["cx"], "by", r0["by"], r1["by"])
        assert abs(r1["iter"] - r0["iter"]) <= 1 and r1["iter"] > 3
        assert abs(r1["cx"] - r0["cx"]) <= 1e-6 * abs(r0["cx"]) and abs(r1["by"] - r0["by"]) <= 1e-6 * abs(r0["by"])
        assert abs(r1["cx"] - r1["by"]) <= 1e-6 * (1 + abs(r1["cx"]))
