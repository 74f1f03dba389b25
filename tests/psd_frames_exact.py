"""Shared by the psdframeit / psdinvjmul tests: the cases, the formulas in numpy.longdouble from qrK's compact frame,
the compiled reference's answers and the accuracy rule of tests/driver/accuracy.py per PSD block.

The frame of a block (qrK.c:86-227): real  frms = n x n, column k rows k.. = c_k, column n-1 = beta; Hermitian  [Re c, Im c, beta (n)],
column n-1 of the planes = the sign vector q.  Q_k = I - c_k c_k^H / beta_k,  Qb = Q_0 ... Q_{n-2} (diag(q))."""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble

# block shapes (problem.make_K(1, [], s, hs=hs)) and input variants
CASES = [
    dict(s=[1]), dict(s=[2]), dict(hs=[1]), dict(hs=[2]),              # no or one reflector, the sign column alone
    dict(s=[15, 16, 17]),                                              # MFMA 16-edges
    dict(s=[63, 64, 65]), dict(s=[130]), dict(s=[200, 3], hs=[66]),    # 64-tile edges, several tiles, mixed block list and offsets
    dict(hs=[70]),                                                     # Hermitian across a tile edge
    dict(s=[15, 16, 17], zero_col=True),                               # all-zero column in qrK's input: the beta = 1 identity reflector
    dict(s=[63, 64, 65], ones=True),                                   # lab all ones
]
GPU_ONLY_CASE = dict(s=[200, 200, 200], hs=[130])
STRIP_CASE = dict(s=[65], hs=[33])


def block_list(K):
    s = K["s"].ravel().astype(int)
    r = int(np.asarray(K["rsdpN"]).ravel()[0])
    return [(int(n), k >= r) for k, n in enumerate(s)]


def split_blocks(x, K):
    """the blocks of a lenud vector as real / complex n x n matrices (same dtype family as x)"""
    x = np.asarray(x).ravel()
    out, o = [], 0
    for n, herm in block_list(K):
        re = x[o:o + n * n].reshape(n, n, order="F"); o += n * n
        if herm:
            im = x[o:o + n * n].reshape(n, n, order="F"); o += n * n
            out.append(re + 1j * im)
        else:
            out.append(re.copy())
    return out


def pack_blocks(mats, K):
    parts = []
    for M, (n, herm) in zip(mats, block_list(K)):
        parts.append(np.real(M).ravel(order="F"))
        if herm:
            parts.append(np.imag(M).ravel(order="F"))
    return np.concatenate(parts) if parts else np.zeros(0)


def exact_frames(frms, K):
    """Qb of every block in longdouble out of the compact frame"""
    frms = np.asarray(frms, dtype=np.float64).ravel()
    out, o = [], 0
    for n, herm in block_list(K):
        nn = n * n
        if herm:
            c = frms[o:o + nn].reshape(n, n, order="F").astype(CLD) + 1j * frms[o + nn:o + 2 * nn].reshape(n, n, order="F").astype(CLD)
            beta = frms[o + 2 * nn:o + 2 * nn + n].astype(LD); o += 2 * nn + n
            Q = np.eye(n, dtype=CLD)
        else:
            c = frms[o:o + nn].reshape(n, n, order="F").astype(LD); o += nn
            beta = c[:, n - 1].copy()
            Q = np.eye(n, dtype=LD)
        for k in range(n - 2, -1, -1):                                 # Q <- Q_k Q
            v = c[k:, k]
            Q[k:, :] -= np.outer(v, (v.conj() @ Q[k:, :]) / beta[k])
        if herm:
            Q = Q * c[:, n - 1][None, :]
        out.append(Q)
    return out


def exact_frameit(Qs, lab):
    out, o = [], 0
    for Q in Qs:
        n = Q.shape[0]
        out.append(Q.conj().T @ (lab[o:o + n].astype(LD)[:, None] * Q)); o += n
    return out


def exact_invjmul(Qs, xlab, y, K):
    out, o = [], 0
    for Q, Y in zip(Qs, split_blocks(y, K)):
        n = Q.shape[0]
        Y = Y.astype(Q.dtype)
        Ys = np.tril(Y) + np.tril(Y, -1).conj().T                      # only the lower triangle of y is read
        x = xlab[o:o + n].astype(LD); o += n
        T = Q @ Ys @ Q.conj().T
        T = T * (2 / (x[:, None] + x[None, :]))
        out.append(Q.conj().T @ T @ Q)
    return out


def block_errs(v, exact, K):
    """err(v) = max|v - exact| / max|exact| per block"""
    return [float(np.max(np.abs(V.astype(E.dtype) - E)) / np.max(np.abs(E))) for V, E in zip(split_blocks(v, K), exact)]


def check_rule(what, lib, ref, exact, K):
    """err(library) <= 10 err(reference) + 1e-15 per block (tests/driver/accuracy.py); prints both"""
    el, er = block_errs(lib, exact, K), block_errs(ref, exact, K)
    for (n, herm), a, b in zip(block_list(K), el, er):
        print("%-22s n=%-4d %s  library %.2e  reference %.2e" % (what, n, "herm" if herm else "real", a, b))
    for (n, herm), a, b in zip(block_list(K), el, er):
        assert a <= 10 * b + 1e-15, (what, n, herm, a, b)


def check_symmetric(v, K):
    """Re symmetric, Im skew with a zero diagonal: bit for bit"""
    for M in split_blocks(v, K):
        assert np.array_equal(np.real(M), np.real(M).T)
        if np.iscomplexobj(M):
            assert np.array_equal(np.imag(M), -np.imag(M).T) and not np.imag(M).diagonal().any()


_cache = {}


def make_case(refmex, kw, seed):
    """Inputs, the reference's answers and the longdouble ones of a case: computed once per session, shared by the emulator and the
    device tests, never modified."""
    key = (repr(sorted(kw.items())), seed)
    if key in _cache:
        return _cache[key]
    from sedumi_amd import problem
    K = problem.make_K(1, [], kw.get("s", []), hs=kw.get("hs", ()))
    rng = np.random.default_rng(seed)
    mats = []
    for n, herm in block_list(K):
        M = rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if herm else 0)
        if kw.get("zero_col") and not herm and n > 2:
            M[:, n // 2] = 0.0                                         # qrK.c:105-106: beta = 1, c = 0
        mats.append(M)
    x = pack_blocks(mats, K)
    frms = np.asarray(refmex.call("qrK", 2, x.reshape(-1, 1), K)[0], dtype=np.float64).ravel()
    slen = sum(n for n, _ in block_list(K))
    lab = np.ones(slen) if kw.get("ones") else 10.0 ** rng.uniform(-3, 3, slen)
    ym = []
    for n, herm in block_list(K):
        Y = rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if herm else 0)
        Y = Y + Y.conj().T                                             # Hermitian, Im diag = 0 as its producers leave it
        ym.append(Y)
    y = pack_blocks(ym, K)
    Qs = exact_frames(frms, K)
    c = dict(K=K, frms=frms, lab=lab, y=y, Qs=Qs, qb=pack_blocks([np.asarray(Q, dtype=np.complex128 if np.iscomplexobj(Q) else np.float64) for Q in Qs], K),
             X=exact_frameit(Qs, lab), Z=exact_invjmul(Qs, lab, y, K),
             Xref=np.asarray(refmex.call("psdframeit", 1, lab.reshape(-1, 1), frms.reshape(-1, 1), K)).ravel(),
             Zref=np.asarray(refmex.call("psdinvjmul", 1, lab.reshape(-1, 1), frms.reshape(-1, 1), y.reshape(-1, 1), K)).ravel())
    y_garbage = []
    for Y in ym:
        G = Y.copy()
        iu = np.triu_indices(Y.shape[0], 1)
        G[iu] = rng.standard_normal(iu[0].size) * 1e3 + (1j * rng.standard_normal(iu[0].size) if np.iscomplexobj(Y) else 0)
        y_garbage.append(G)
    c["y_garbage"] = pack_blocks(y_garbage, K)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cache[key] = c
    return c


def check_case(refmex, kw, seed=0, full=None):
    """Every assertion of a shape on whichever library capi is bound to.  full: the repeated calls with both frame kinds and with the clean
    and the garbage y; otherwise (the default above 20000 matrix entries, where the emulator needs seconds per call) the repeated calls use
    the explicit frame, and psdinvjmul's is the one with garbage in the upper triangle of y."""
    from sedumi_amd import mex
    c = make_case(refmex, kw, seed)
    K = c["K"]
    if full is None:
        full = c["y"].size <= 20000
    # the expansion: against longdouble Qb, and unitary
    qb = mex.psdframe_explicit(c["frms"], K).ravel()
    eq = block_errs(qb, c["Qs"], K)
    eo = []
    for Q in split_blocks(qb, K):
        Ql = Q.astype(CLD if np.iscomplexobj(Q) else LD)
        eo.append(float(np.max(np.abs(Ql.conj().T @ Ql - np.eye(Q.shape[0])))))
    for (n, herm), a, b in zip(block_list(K), eq, eo):
        print("%-22s n=%-4d %s  |Qb - exact| %.2e  |Qb^H Qb - I| %.2e" % ("psdframe_explicit", n, "herm" if herm else "real", a, b))
    assert max(eq) <= 1e-14 and max(eo) <= 1e-14, (eq, eo)
    assert np.array_equal(qb, mex.psdframe_explicit(c["frms"], K).ravel())
    for kind, frame in ((mex.FRAME_HOUSEHOLDER, c["frms"]), (mex.FRAME_EXPLICIT, c["qb"])):
        x = mex.psdframeit(c["lab"], frame, K, frame_kind=kind).ravel()
        z = mex.psdinvjmul(c["lab"], frame, c["y"], K, frame_kind=kind).ravel()
        check_rule("psdframeit kind %d" % kind, x, c["Xref"], c["X"], K)
        check_rule("psdinvjmul kind %d" % kind, z, c["Zref"], c["Z"], K)
        check_symmetric(x, K); check_symmetric(z, K)
        if kind == mex.FRAME_EXPLICIT or full:
            # two calls give the same bits; garbage in the strict upper triangle of y changes nothing
            assert np.array_equal(x, mex.psdframeit(c["lab"], frame, K, frame_kind=kind).ravel())
            if full:
                assert np.array_equal(z, mex.psdinvjmul(c["lab"], frame, c["y"], K, frame_kind=kind).ravel())
            assert np.array_equal(z, mex.psdinvjmul(c["lab"], frame, c["y_garbage"], K, frame_kind=kind).ravel())


def check_strip_paths(refmex):
    """s=[65], hs=[33]: the expansion with the default strips (32 columns in LDS), with the narrowest strips (4 columns in LDS: budget =
    4 columns of the wider block, 4 * 2 * 33 * 8 = 2112 >= 4 * 65 * 8 bytes) and in global memory (budget below 4 columns of either block):
    the same bits, and longdouble's Qb to 1e-14."""
    from sedumi_amd import mex
    c = make_case(refmex, STRIP_CASE, 7)
    K = c["K"]
    try:
        q0 = mex.psdframe_explicit(c["frms"], K).ravel()
        mex.set_frame_lds_budget(2112)
        q1 = mex.psdframe_explicit(c["frms"], K).ravel()
        mex.set_frame_lds_budget(1024)
        q2 = mex.psdframe_explicit(c["frms"], K).ravel()
        x2 = mex.psdframeit(c["lab"], c["frms"], K).ravel()
    finally:
        mex.set_frame_lds_budget(0)
    assert np.array_equal(q0, q1) and np.array_equal(q0, q2)
    e = block_errs(q0, c["Qs"], K)
    print("strip paths: |Qb - exact|", e)
    assert max(e) <= 1e-14
    check_rule("psdframeit (global)", x2, c["Xref"], c["X"], K)


def small_hermitian_sdp(seed=5):
    """user-level (At, b, c, K) of a small feasible SDP: LP part, a real PSD block of order 5 and a Hermitian one of order 4 (K.scomplex)"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    Kl, n1, n2, m = 3, 5, 4, 6

    def herm(n, cplx, pd):
        B = rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if cplx else 0)
        return (B @ B.conj().T + n * np.eye(n)) if pd else (B + B.conj().T) / 2

    def vec(l, A, B):
        return np.concatenate((l, A.ravel(order="F"), B.ravel(order="F")))
    At = np.stack([vec(rng.standard_normal(Kl), herm(n1, False, False), herm(n2, True, False)) for _ in range(m)], axis=1)
    X0 = vec(1 + rng.random(Kl), herm(n1, False, True), herm(n2, True, True))
    Z0 = vec(1 + rng.random(Kl), herm(n1, False, True), herm(n2, True, True))
    return sp.csc_matrix(At), (At.conj().T @ X0).real, Z0 + At @ rng.standard_normal(m), {"l": Kl, "s": [n1, n2], "scomplex": [2]}
