"""Host-side mirror of the reference MEX interface for the hot path.

Every function has the name, argument order and argument meaning of the MEX
gateway it replaces (MATLAB conventions: 1-based indices carried as doubles,
structs as dicts, sparse matrices as scipy CSC), converts exactly what the
gateway converts, and calls the C ABI of libsedumi_hip.so (tier 1 of
include/sedumi_hip.h).  So a parity test reads like the MATLAB call site:

    ADA = getada1(ADA, A, Ablkjc[:, 2], Aord["lqperm"], d, K["qblkstart"])   # sedumi.m:450
    ADA = getada2(ADA, DAt, Aord, K)                                          # sedumi.m:451
    ADA, absd = getada3(ADA, A, Ablkjc[:, 2], Aord, udsqr, K)                 # sedumi.m:452
    LL, Ld, Lskip, Ladd = blkchol(L, ADA, pars_chol, absd)                    # sedumi.m:458
    y = bwblkslv(L, fwblkslv(L, b) / Ld)                                      # wrapPcg.m:56-59

Errors raise SdmError (the gateways call mexErrMsgTxt).  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.sparse as sp

from . import capi
from .capi import SdmError, check, f64, i64, pf, pi


def _csc(X):
    X = sp.csc_matrix(X)
    if not X.has_sorted_indices:
        X = X.copy()
        X.sort_indices()
    return X


def _field(s, name, what):
    if name not in s:
        raise SdmError(f"Missing field {what}.{name}.")
    return s[name]


def _same_pattern(X, pr):
    return sp.csc_matrix((pr, X.indices.copy(), X.indptr.copy()), shape=X.shape)


def _perm0(p, m, what):
    p = i64(np.asarray(p, dtype=np.float64).ravel()) - 1
    if p.size != m:
        raise SdmError(f"Size mismatch {what}.")
    return p


def _Kfields(K):
    l = int(np.asarray(K.get("l", 0)).ravel()[0]) if np.size(K.get("l", 0)) else 0
    q = np.asarray(K.get("q", []), dtype=np.float64).ravel()
    if q.size == 1 and q[0] == 0:
        q = q[:0]
    s = np.asarray(K.get("s", []), dtype=np.float64).ravel()
    if s.size == 1 and s[0] == 0:
        s = s[:0]
    rsdpN = int(np.asarray(K["rsdpN"]).ravel()[0]) if "rsdpN" in K else s.size
    return l, i64(q), i64(s), rsdpN


# --------------------------------------------------------------------- ADA'
def getada1(ADA, A, Ajc2, perm, d, blkstart):
    """ADA = getada1(ADA, A, Ajc2, perm, d, blkstart)   (getada1.c:161-261)"""
    ADA, A = _csc(ADA), _csc(A)
    m = A.shape[1]
    if ADA.shape != (m, m):
        raise SdmError("Size mismatch ADA.")
    Ajc2 = i64(np.asarray(Ajc2, dtype=np.float64))
    if Ajc2.size != m:
        raise SdmError("Size mismatch Ajc2.")
    p0 = _perm0(perm, m, "perm")
    dl = f64(_field(d, "l", "d"))
    ddet = f64(_field(d, "det", "d"))
    qb = i64(np.asarray(blkstart, dtype=np.float64)) - 1      # K.qblkstart, 1-based -> 0-based
    lorN = qb.size - 1
    if lorN != ddet.size:
        raise SdmError("Size d.det mismatch")
    out = np.zeros(ADA.indptr[-1], dtype=np.float64)
    jc, ir = i64(ADA.indptr), i64(ADA.indices)
    Ajc, Air, Apr = i64(A.indptr), i64(A.indices), f64(A.data)
    check(capi.lib().sdm_getada1(C.c_int64(m), pi(jc), pi(ir), C.c_int64(A.shape[0]), pi(Ajc), pi(Air), pf(Apr),
                                 pi(Ajc2), pi(p0), C.c_int64(dl.size), pf(dl), C.c_int64(lorN), pf(ddet), pi(qb), pf(out)))
    return _same_pattern(ADA, out)


def getada2(ADA, DAt, Aord, K):
    """ADA = getada2(ADA, DAt, Aord, K)   (getada2.c:127-214)"""
    ADA = _csc(ADA)
    m = ADA.shape[0]
    out = f64(ADA.data).copy()
    _, q, _, _ = _Kfields(K)
    if q.size == 0:
        return _same_pattern(ADA, out)
    Q = _csc(_field(DAt, "q", "DAt"))
    if Q.shape != (q.size, m):
        raise SdmError("Size mismatch DAt.q.")
    qperm = _perm0(_field(Aord, "qperm", "Aord"), m, "Aord.qperm")
    jc, ir = i64(ADA.indptr), i64(ADA.indices)
    Qjc, Qir, Qpr = i64(Q.indptr), i64(Q.indices), f64(Q.data)
    check(capi.lib().sdm_getada2(C.c_int64(m), pi(jc), pi(ir), pf(out), C.c_int64(q.size), pi(Qjc), pi(Qir), pf(Qpr),
                                 pi(qperm)))
    return _same_pattern(ADA, out)


def getada(ADA, A, K, d, DAt):
    """[ADA, absd] = the effect of `absd = getada(A,K,d,DAt)` on the global ADA_sedumi_ (getada.m:13-40; sedumi.m:446-448
    takes this route when sum(K.s)==0).  Python has no MATLAB globals: the global's pattern comes in as `ADA`, its new
    value goes out first.  Entries that MATLAB's sparse() would drop are kept as explicit zeros."""
    ADA, A = _csc(ADA), _csc(A)
    m = A.shape[1]
    if ADA.shape != (m, m):
        raise SdmError("Size mismatch ADA.")
    lpN, q, s, _ = _Kfields(K)
    if np.sum(s) != 0:
        raise SdmError("getada is the path of problems without PSD blocks (sedumi.m:446).")
    dl, ddet = f64(_field(d, "l", "d")), f64(_field(d, "det", "d"))
    if dl.size != lpN or ddet.size != q.size:
        raise SdmError("Size mismatch d.l / d.det.")
    qb = i64(np.asarray(_field(K, "qblkstart", "K"), dtype=np.float64)) - 1
    jc, ir = i64(ADA.indptr), i64(ADA.indices)
    Ajc, Air, Apr = i64(A.indptr), i64(A.indices), f64(A.data)
    if q.size:
        Q = _csc(_field(DAt, "q", "DAt"))
        if Q.shape != (q.size, m):
            raise SdmError("Size mismatch DAt.q.")
        Qjc, Qir, Qpr = i64(Q.indptr), i64(Q.indices), f64(Q.data)
    else:
        Qjc, Qir, Qpr = np.zeros(m + 1, dtype=np.int64), np.zeros(1, dtype=np.int64), np.zeros(1)
        qb = np.zeros(1, dtype=np.int64)
    out = np.zeros(ADA.nnz, dtype=np.float64)
    absd = np.zeros(m, dtype=np.float64)
    check(capi.lib().sdm_getada(C.c_int64(m), pi(jc), pi(ir), C.c_int64(A.shape[0]), pi(Ajc), pi(Air), pf(Apr), C.c_int64(lpN),
                                pf(dl), C.c_int64(q.size), pf(ddet), pi(qb), pi(Qjc), pi(Qir), pf(Qpr), pf(out), pf(absd)))
    return _same_pattern(ADA, out), absd.reshape(-1, 1)


def getada3(ADA, A, Ajc1, Aord, udsqr, K):
    """[ADA, absd] = getada3(ADA, A, Ajc1, Aord, udsqr, K)   (getada3.c:370-569)"""
    ADA, A = _csc(ADA), _csc(A)
    m = A.shape[1]
    if ADA.shape != (m, m):
        raise SdmError("Size mismatch ADA.")
    lpN, q, s, rsdpN = _Kfields(K)
    Ajc1 = i64(np.asarray(Ajc1, dtype=np.float64))
    if Ajc1.size != m:
        raise SdmError("Ajc1 size mismatch")
    sperm = _perm0(_field(Aord, "sperm", "Aord"), m, "Aord.sperm")
    blkstart = np.asarray(_field(K, "blkstart", "K"), dtype=np.float64).ravel()
    if blkstart.size != 2 + q.size + s.size:
        raise SdmError("Size mismatch K.blkstart.")
    psd_start = i64(blkstart[q.size + 1:]) - 1
    ud = f64(udsqr)
    lenud = int(np.sum(s[:rsdpN] ** 2) + 2 * np.sum(s[rsdpN:] ** 2))
    if ud.size != lenud:
        raise SdmError("udsqr size mismatch.")
    Kc, keep = capi.make_cone(lpN, q, s, rsdpN)
    out = f64(ADA.data).copy()
    absd = np.zeros(m, dtype=np.float64)
    jc, ir = i64(ADA.indptr), i64(ADA.indices)
    Ajc, Air, Apr = i64(A.indptr), i64(A.indices), f64(A.data)
    check(capi.lib().sdm_getada3(C.c_int64(m), pi(jc), pi(ir), pf(out), C.c_int64(A.shape[0]), pi(Ajc), pi(Air), pf(Apr),
                                 pi(Ajc1), pi(sperm), pf(ud), C.byref(Kc), pi(psd_start), pf(absd)))
    del keep
    return _same_pattern(ADA, out), absd.reshape(-1, 1)


# ------------------------------------------------------------- factor / solve
def _Lstruct(L, need_values):
    if not isinstance(L, dict):
        raise SdmError("Parameter `L' should be a structure.")
    LL = _field(L, "L", "L")
    if not sp.issparse(LL):
        raise SdmError("L.L should be sparse.")
    LL = _csc(LL)
    m = LL.shape[0]
    if LL.shape != (m, m):
        raise SdmError("Size L.L mismatch.")
    perm = _perm0(_field(L, "perm", "L"), m, "L.perm")
    xs = i64(np.asarray(_field(L, "xsuper", "L"), dtype=np.float64)) - 1
    if xs.size - 1 > m:
        raise SdmError("Size L.xsuper mismatch.")
    return m, LL, i64(LL.indptr), i64(LL.indices), (f64(LL.data) if need_values else None), perm, xs


def blkchol(L, X, pars=None, absd=None):
    """[L.L, L.d, L.skip, L.add] = blkchol(L, X, pars, absd)   (blkchol.c:239-440)"""
    m, LL, Ljc, Lir, _, perm, xs = _Lstruct(L, False)
    X = _csc(X)
    if X.shape != (m, m):
        raise SdmError("P must be square")
    cp = capi.CholPars(1e-12, 5e2, 1e-20)            # blkchol.c:292-294
    if pars is not None:
        if "canceltol" in pars:
            cp.canceltol = float(np.asarray(pars["canceltol"]).ravel()[0])
        if "maxu" in pars:
            cp.maxu = float(np.asarray(pars["maxu"]).ravel()[0])
        if "abstol" in pars:
            cp.abstol = max(float(np.asarray(pars["abstol"]).ravel()[0]), 0.0)
    ab = None
    if pars is not None and absd is not None:          # absd is only read when pars is given (blkchol.c:312-316)
        ab = f64(absd)
        if ab.size != m:
            raise SdmError("absd size mismatch")
    Xjc, Xir, Xpr = i64(X.indptr), i64(X.indices), f64(X.data)
    Lpr = np.zeros(Ljc[-1], dtype=np.float64)
    d = np.zeros(m, dtype=np.float64)
    nskip, nadd = C.c_int64(0), C.c_int64(0)
    sidx, aidx = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
    sval, aval = np.zeros(m, dtype=np.float64), np.zeros(m, dtype=np.float64)
    check(capi.lib().sdm_blkchol(C.c_int64(m), pi(Ljc), pi(Lir), pi(perm), C.c_int64(xs.size - 1), pi(xs), pi(Xjc), pi(Xir),
                                 pf(Xpr), C.byref(cp), pf(ab), pf(Lpr), pf(d), C.byref(nskip), pi(sidx), pf(sval),
                                 C.byref(nadd), pi(aidx), pf(aval)))
    ns, na = nskip.value, nadd.value
    Lout = sp.csc_matrix((Lpr, LL.indices.copy(), LL.indptr.copy()), shape=(m, m))
    skip = sp.csc_matrix((sval[:ns], sidx[:ns], np.array([0, ns])), shape=(m, 1))
    add = sp.csc_matrix((aval[:na], aidx[:na], np.array([0, na])), shape=(m, 1))
    return Lout, d.reshape(-1, 1), skip, add


def _solve(fw, L, b, ysymb):
    m, LL, Ljc, Lir, Lpr, perm, xs = _Lstruct(L, True)
    lib = capi.lib()
    if sp.issparse(b):
        if ysymb is None:
            raise SdmError("fwblkslv requires more inputs in case of sparse b.")
        B, Y = _csc(b), _csc(ysymb)
        if B.shape[0] != m:
            raise SdmError("Size mismatch b.")
        if Y.shape != B.shape:
            raise SdmError("Size mismatch y.")
        n = B.shape[1]
        Bjc, Bir, Bpr = i64(B.indptr), i64(B.indices), f64(B.data)
        Yjc, Yir = i64(Y.indptr), i64(Y.indices)
        Ypr = np.zeros(max(int(Yjc[-1]), 1), dtype=np.float64)
        if fw:
            check(lib.sdm_fwblkslv_sparse(C.c_int64(m), pi(Ljc), pi(Lir), pf(Lpr), pi(perm), C.c_int64(xs.size - 1), pi(xs),
                                          C.c_int64(n), pi(Bjc), pi(Bir), pf(Bpr), pi(Yjc), pi(Yir), pf(Ypr)))
        else:
            check(lib.sdm_bwblkslv_sparse(C.c_int64(m), pi(Ljc), pi(Lir), pf(Lpr), C.c_int64(xs.size - 1), pi(xs),
                                          C.c_int64(n), pi(Bjc), pi(Bir), pf(Bpr), pi(Yjc), pi(Yir), pf(Ypr)))
        return sp.csc_matrix((Ypr[:Yjc[-1]], Y.indices.copy(), Y.indptr.copy()), shape=Y.shape)
    b = np.asarray(b, dtype=np.float64)
    if b.ndim == 1:
        b = b.reshape(-1, 1)
    if b.shape[0] != m:
        raise SdmError("Size mismatch b.")
    n = b.shape[1]
    bf = f64(b)
    y = np.zeros(m * n, dtype=np.float64)
    fn = lib.sdm_fwblkslv if fw else lib.sdm_bwblkslv
    check(fn(C.c_int64(m), pi(Ljc), pi(Lir), pf(Lpr), pi(perm), C.c_int64(xs.size - 1), pi(xs), C.c_int64(n), pf(bf), pf(y)))
    return y.reshape((m, n), order="F")


def fwblkslv(L, b, ysymb=None):
    """y = fwblkslv(L, b [,ysymb]):  y = L.L \\ b(L.perm,:)   (fwblkslv.c:193-320)"""
    return _solve(True, L, b, ysymb)


def bwblkslv(L, b, ysymb=None):
    """y = bwblkslv(L, b [,ysymb]):  y(L.perm,:) = L.L' \\ b   (bwblkslv.c:182-298)"""
    return _solve(False, L, b, ysymb)


# ------------------------------------------------------------------ symbolic
def ordmmdmex(X):
    """perm = ordmmdmex(X): multiple-minimum-degree ordering of spones(X)   (ordmmdmex.c:75-139)"""
    if not sp.issparse(X):
        raise SdmError("Input matrix must be sparse")
    X = _csc(X)
    m = X.shape[0]
    if X.shape != (m, m):
        raise SdmError("X should be square.")
    jc, ir = i64(X.indptr), i64(X.indices)
    perm = np.zeros(m, dtype=np.int64)
    check(capi.lib().sdm_ordmmd(C.c_int64(m), pi(jc), pi(ir), pi(perm)))
    return (perm + 1).astype(np.float64).reshape(-1, 1)


def symfctmex(X, perm):
    """L = symfctmex(X, perm) -> L.{L, perm, xsuper}   (symfctmex.c:127-272)"""
    X = _csc(X)
    m = X.shape[0]
    if X.shape != (m, m):
        raise SdmError("X must be square")
    p0 = _perm0(perm, m, "perm")
    jc, ir = i64(X.indptr), i64(X.indices)
    nsuper, nnzl = C.c_int64(0), C.c_int64(0)
    lib = capi.lib()
    check(lib.sdm_symfct(C.c_int64(m), pi(jc), pi(ir), pi(p0), None, C.byref(nsuper), None, C.byref(nnzl), None, None))
    pout = np.zeros(m, dtype=np.int64)
    xs = np.zeros(nsuper.value + 1, dtype=np.int64)
    Ljc = np.zeros(m + 1, dtype=np.int64)
    Lir = np.zeros(max(nnzl.value, 1), dtype=np.int64)
    check(lib.sdm_symfct(C.c_int64(m), pi(jc), pi(ir), pi(p0), pi(pout), C.byref(nsuper), pi(xs), C.byref(nnzl), pi(Ljc), pi(Lir)))
    LL = sp.csc_matrix((np.ones(nnzl.value), Lir[:nnzl.value], Ljc), shape=(m, m))
    return {"L": LL, "perm": (pout + 1).astype(np.float64).reshape(-1, 1), "xsuper": (xs + 1).astype(np.float64).reshape(-1, 1)}


def choltmpsiz(L):
    """tmpsiz = choltmpsiz(L)   (choltmpsiz.c:110-173)"""
    LL = _csc(_field(L, "L", "L"))
    m = LL.shape[0]
    xs = i64(np.asarray(_field(L, "xsuper", "L"), dtype=np.float64)) - 1
    jc, ir = i64(LL.indptr), i64(LL.indices)
    out = C.c_int64(0)
    check(capi.lib().sdm_choltmpsiz(C.c_int64(m), pi(jc), pi(ir), C.c_int64(xs.size - 1), pi(xs), C.byref(out)))
    return np.array([[float(out.value)]])


def cholsplit(L, cachsz):
    """split = cholsplit(L, cachsz)   (cholsplit.c:118-184)"""
    LL = _csc(_field(L, "L", "L"))
    m = LL.shape[0]
    xs = i64(np.asarray(_field(L, "xsuper", "L"), dtype=np.float64)) - 1
    jc = i64(LL.indptr)
    split = np.zeros(max(m, 1), dtype=np.int64)
    check(capi.lib().sdm_cholsplit(C.c_int64(m), pi(jc), C.c_int64(xs.size - 1), pi(xs), C.c_double(float(np.asarray(cachsz).ravel()[0])), pi(split)))
    return split[:m].astype(np.float64).reshape(-1, 1)


def incorder(At, Ajc1=None, ifirst=None):
    """[perm, dz] = incorder(At [, Ajc1, ifirst])   (incorder.c:216-330).  perm 1-based m x 1; dz N x m sparse whose
    columns list their row subscripts in the order incorder introduced them (NOT sorted: the order is data for
    finsymbden / getada3 -- the returned csc_matrix keeps it as long as nobody sorts its indices)."""
    if not sp.issparse(At):
        raise SdmError("At must be a sparse matrix.")
    At = sp.csc_matrix(At)
    N, m = At.shape
    jc, ir = i64(At.indptr), i64(At.indices)
    first = 0
    a1 = None
    if Ajc1 is not None:
        a1 = i64(np.asarray(Ajc1, dtype=np.float64))
        if a1.size < m:
            raise SdmError("Ajc1 size mismatch")
        first = int(np.asarray(ifirst).ravel()[0]) - 1
    nin = int(np.sum(jc[1:] - (a1[:m] if a1 is not None else jc[:-1])))
    perm = np.zeros(max(m, 1), dtype=np.int64)
    dzjc = np.zeros(m + 1, dtype=np.int64)
    dzir = np.zeros(max(min(N - first, nin), 1), dtype=np.int64)
    check(capi.lib().sdm_incorder(C.c_int64(N), C.c_int64(m), pi(jc), pi(ir), pi(a1) if a1 is not None else None, C.c_int64(first),
                                  pi(perm), pi(dzjc), pi(dzir)))
    nnz = int(dzjc[m])
    dz = sp.csc_matrix((np.ones(nnz), dzir[:nnz].astype(np.int32), dzjc.astype(np.int32)), shape=(N, m))
    return (perm[:m] + 1).astype(np.float64).reshape(-1, 1), dz


def symbchol(ADA, cachsz=512):
    """symbchol.m:62-83 on top of the entry points above (MATLAB glue, host only)."""
    ADA = _csc(ADA)
    m = ADA.shape[0]
    if ADA.nnz < m * m:
        L = symfctmex(ADA, ordmmdmex(ADA))
    else:
        L = {"perm": np.arange(1, m + 1, dtype=np.float64).reshape(-1, 1), "L": sp.csc_matrix(np.tril(np.ones((m, m)))),
             "xsuper": np.array([[1.0], [m + 1.0]])}
    L["tmpsiz"] = choltmpsiz(L)
    L["split"] = cholsplit(L, cachsz)
    return L


# ------------------------------------------------------------- dense columns
def symbfwblk(L, b):
    """x = symbfwblk(L, b): sparsity pattern (values all 1) of L.L \\ b(L.perm,:)   (symbfwblk.c:270-377)"""
    m, LL, Ljc, Lir, _, perm, xs = _Lstruct(L, False)
    if not sp.issparse(b):
        raise SdmError("B must be sparse")
    B = _csc(b)
    if B.shape[0] != m:
        raise SdmError("L.perm size mismatches B")
    n = B.shape[1]
    Bjc, Bir = i64(B.indptr), i64(B.indices)
    Xjc = np.zeros(n + 1, dtype=np.int64)
    lib = capi.lib()
    args = (C.c_int64(m), pi(Ljc), pi(Lir), pi(perm), C.c_int64(xs.size - 1), pi(xs), C.c_int64(n), pi(Bjc), pi(Bir))
    check(lib.sdm_symbfwblk(*args, pi(Xjc), None))
    Xir = np.zeros(max(int(Xjc[-1]), 1), dtype=np.int64)
    check(lib.sdm_symbfwblk(*args, pi(Xjc), pi(Xir)))
    nnz = int(Xjc[-1])
    return sp.csc_matrix((np.ones(nnz), Xir[:nnz], Xjc), shape=(m, n))


def finsymbden(LAD, perm, dz, firstq):
    """Lden = finsymbden(LAD, perm, dz, firstq) -> dict(LAD, perm, dz, first)   (finsymbden.c:112-214)"""
    LAD, dz = _csc(LAD), sp.csc_matrix(dz)                 # dz: row order inside the columns is data, never sorted
    m, n = LAD.shape
    p = i64(np.asarray(perm, dtype=np.float64)) - 1
    nperm = p.size
    if dz.shape != (m, nperm):
        raise SdmError("dz size mismatch")
    LADjc, LADir, dzjc, dzir = i64(LAD.indptr), i64(LAD.indices), i64(dz.indptr), i64(dz.indices)
    po, jo, fo = np.zeros(max(n, 1), dtype=np.int64), np.zeros(n + 1, dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64)
    check(capi.lib().sdm_finsymbden(C.c_int64(m), C.c_int64(n), pi(LADjc), pi(LADir), C.c_int64(nperm), pi(p), pi(dzjc),
                                    pi(dzir), C.c_int64(int(np.asarray(firstq).ravel()[0]) - 1), pi(po), pi(jo), pi(fo)))
    # the reference keeps dz.ir / dz.pr and only swaps the column pointers (finsymbden.c:196-199)
    nz = int(jo[n])
    dznew = sp.csc_matrix((np.asarray(dz.data[:nz], dtype=np.float64), dzir[:nz].copy(), jo.copy()), shape=(m, n))
    return {"LAD": LAD, "perm": (po[:n] + 1).astype(np.float64).reshape(-1, 1), "dz": dznew,
            "first": (fo[:n] + 1).astype(np.float64).reshape(-1, 1)}


def _dz(dz):
    """Lden.dz / Lsymb.dz: either a scipy CSC matrix or the explicit {'jc','ir'} form produced by finsymbden."""
    if isinstance(dz, dict):
        return i64(dz["jc"]), i64(dz["ir"])
    dz = sp.csc_matrix(dz)
    return i64(dz.indptr), i64(dz.indices)


def dpr1fact(x, d, Lsymb, smult, maxu):
    """[Lden, Ld] = dpr1fact(x, d, Lsymb, smult, maxu)   (dpr1fact.c:630-848)
    Lden = dict(betajc (1-based), beta, p, pivperm (0-based, as the reference), dopiv)."""
    X = _csc(x)
    m, n = X.shape
    lab = f64(d).copy()
    if lab.size != m:
        raise SdmError("Size mismatch d.")
    sm = f64(smult)
    if sm.size != n:
        raise SdmError("Size mismatch smult.")
    dzjc, dzir = _dz(_field(Lsymb, "dz", "Lsymb"))
    colperm = _perm0(_field(Lsymb, "perm", "Lsymb"), n, "Lsymb.perm")
    first = i64(np.asarray(_field(Lsymb, "first", "Lsymb"), dtype=np.float64)) - 1
    if first.size != n:
        raise SdmError("Size mismatch Lsymb.first.")
    pnnz = int(dzjc[1:n + 1].sum())
    betajc = np.zeros(n + 1, dtype=np.int64)
    beta, p = np.zeros(max(pnnz, 1)), np.zeros(max(pnnz, 1))
    pivperm, dopiv = np.zeros(max(pnnz, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64)
    npp = C.c_int64(0)
    Xjc, Xir, Xpr = i64(X.indptr), i64(X.indices), f64(X.data)
    check(capi.lib().sdm_dpr1fact(C.c_int64(m), C.c_int64(n), pi(Xjc), pi(Xir), pf(Xpr), pf(lab), pi(dzjc), pi(dzir), pi(colperm),
                                  pi(first), pf(sm), C.c_double(float(np.asarray(maxu).ravel()[0])), pi(betajc), pf(beta), pf(p),
                                  pi(pivperm), C.byref(npp), pi(dopiv)))
    Lden = {"betajc": (betajc + 1).astype(np.float64).reshape(-1, 1), "beta": beta[:int(betajc[n])].reshape(-1, 1),
            "p": p[:pnnz].reshape(-1, 1), "pivperm": pivperm[:npp.value].astype(np.float64).reshape(-1, 1),
            "dopiv": dopiv[:n].astype(np.float64).reshape(-1, 1)}
    return Lden, lab.reshape(-1, 1)


def _pr1(fw, Lden, b):
    b = np.asarray(b, dtype=np.float64)
    if sp.issparse(b):
        raise SdmError("b should be full")
    if b.ndim == 1:
        b = b.reshape(-1, 1)
    m, nrhs = b.shape
    betajc = i64(np.asarray(_field(Lden, "betajc", "Lden"), dtype=np.float64)) - 1
    nden = betajc.size - 1
    if nden == 0:
        return b.copy()                                   # fwdpr1.c:132-135: no dense columns
    beta, p = f64(_field(Lden, "beta", "Lden")), f64(_field(Lden, "p", "Lden"))
    dopiv = i64(np.asarray(_field(Lden, "dopiv", "Lden"), dtype=np.float64))
    if dopiv.size != nden:
        raise SdmError("Size mismatch Lden.dopiv.")
    pivperm = i64(np.asarray(_field(Lden, "pivperm", "Lden"), dtype=np.float64))
    dzjc, dzir = _dz(_field(Lden, "dz", "Lden"))
    if beta.size != betajc[-1]:
        raise SdmError("Size mismatch Lden.beta.")
    y = np.zeros(m * nrhs)
    fn = capi.lib().sdm_fwdpr1 if fw else capi.lib().sdm_bwdpr1
    pv = pivperm if pivperm.size else np.zeros(1, dtype=np.int64)
    check(fn(C.c_int64(m), C.c_int64(nrhs), C.c_int64(nden), pi(dzjc), pi(dzir), pi(betajc), pf(beta if beta.size else np.zeros(1)),
             pf(p if p.size else np.zeros(1)), pi(pv), C.c_int64(pivperm.size), pi(dopiv), pf(f64(b)), pf(y)))
    return y.reshape((m, nrhs), order="F")


def fwdpr1(Lden, b):
    """y = fwdpr1(Lden, b): y = PROD_k L(p_k, beta_k) \\ b   (fwdpr1.c:101-202)"""
    return _pr1(True, Lden, b)


def bwdpr1(Lden, b):
    """y = bwdpr1(Lden, b): y = (PROD_k L(p_k, beta_k))' \\ b   (bwdpr1.c:170-275)"""
    return _pr1(False, Lden, b)


def _dense_struct(dense, nlor):
    nl = int(np.asarray(_field(dense, "l", "dense")).ravel()[0])
    q = i64(np.asarray(_field(dense, "q", "dense"), dtype=np.float64)) - 1
    cols = np.asarray(_field(dense, "cols", "dense"), dtype=np.float64).ravel()
    nden = cols.size - nl - q.size
    if nden < 0:
        raise SdmError("dense.q size mismatch.")
    dencols = i64(cols[nl + q.size:]) - 1
    if q.size and (q.min() < 0 or q.max() >= nlor):
        raise SdmError("dense.q out of range")
    return nl, q, dencols, nden


def adendotd(dense, d, sparAd, Ablk, blkstart):
    """Ad = adendotd(dense, d, sparAd, Ablk, blkstart)   (adendotd.c:135-232; getDAtm.m:45)"""
    d1, d2 = f64(_field(d, "q1", "d")), f64(_field(d, "q2", "d"))
    nl, q, dencols, nden = _dense_struct(dense, d1.size)
    A = _csc(_field(dense, "A", "dense"))
    m = A.shape[0]
    if A.shape[1] - nl != q.size + nden:
        raise SdmError("dense.A size mismatch")
    S, B = _csc(sparAd), _csc(Ablk)
    if S.shape[1] != q.size or B.shape[1] != q.size:
        raise SdmError("Size mismatch sparAD")
    bs = np.asarray(blkstart, dtype=np.float64).ravel()
    if bs.size != d1.size + 1:
        raise SdmError("blkstart size mismatch")
    firstQ = int(bs[0]) - 1
    blkend = i64(bs[q + 1]) - 1 if q.size else np.zeros(1, dtype=np.int64)
    out = np.zeros(max(B.nnz, 1), dtype=np.float64)
    adenjc = i64(A.indptr[nl:])
    check(capi.lib().sdm_adendotd(C.c_int64(m), C.c_int64(q.size), C.c_int64(nden), pi(i64(B.indptr)), pi(i64(B.indices)), pf(out),
                                  pi(i64(S.indptr)), pi(i64(S.indices)), pf(f64(S.data)), pi(adenjc), pi(i64(A.indices)), pf(f64(A.data)),
                                  pf(d1), pf(d2), C.c_int64(firstQ), pi(q if q.size else np.zeros(1, dtype=np.int64)),
                                  pi(dencols if nden else np.zeros(1, dtype=np.int64)), pi(blkend)))
    return _same_pattern(B, out[:B.nnz])


def adenscale(dense, d, blkstart):
    """smult = adenscale(dense, d, blkstart)   (adenscale.c:87-160; deninfac.m:61)"""
    detd = f64(_field(d, "det", "d"))
    nl, q, dencols, nden = _dense_struct(dense, detd.size)
    bs = np.asarray(blkstart, dtype=np.float64).ravel()
    if bs.size != detd.size + 1:
        raise SdmError("blkstart size mismatch")
    blkend = i64(bs[q + 1]) - 1 if q.size else np.zeros(1, dtype=np.int64)
    out = np.zeros(max(nden, 1), dtype=np.float64)
    check(capi.lib().sdm_adenscale(C.c_int64(q.size), C.c_int64(nden), pf(detd), pi(q if q.size else np.zeros(1, dtype=np.int64)),
                                   pi(dencols if nden else np.zeros(1, dtype=np.int64)), pi(blkend), pf(out)))
    return out[:nden].reshape(-1, 1)


# ------------------------------------------------------------- next row
def invcholfac(u, K, perm=None):
    """y = invcholfac(u, K, perm): y(perm,perm) = u'*u per PSD block, u upper triangular   (invcholfac.c:59-168).
    u: lenud vector (blocks column-major, Hermitian blocks [Re; Im]); perm: 1-based, concatenated per block (d.perm of
    the scaling), empty / None = no permutation.  Returns the lenud x 1 `udsqr` argument of getada3 (sedumi.m:452)."""
    lpN, q, s, rsdpN = _Kfields(K)
    lenud = int(np.sum(s[:rsdpN] ** 2) + 2 * np.sum(s[rsdpN:] ** 2))
    u = f64(u)
    if u.size != lenud:
        raise SdmError("u size mismatch")
    Kc, keep = capi.make_cone(lpN, q, s, rsdpN)
    y = np.zeros(lenud, dtype=np.float64)
    pp = None
    if perm is not None and np.size(perm) > 0:
        p1 = np.asarray(perm, dtype=np.float64).ravel()
        if p1.size != int(np.sum(s)):
            raise SdmError("perm size mismatch")
        pp = i64(p1 - 1)                       # local to each block (invcholfac.c:129-131), 1-based
    check(capi.lib().sdm_invcholfac(C.byref(Kc), pf(u), pi(pp) if pp is not None else None, pf(y)))
    del keep
    return y.reshape(-1, 1)


# ------------------------------------------------------------- next row
FRAME_HOUSEHOLDER, FRAME_EXPLICIT = 0, 1        # SDM_FRAME_HOUSEHOLDER, SDM_FRAME_EXPLICIT


def _frame_sizes(K, frame_kind):
    """(Cone struct, keep-alive, lenud, sum(K.s), length of the frame array, lpN, number and total order of the Lorentz cones)"""
    lpN, q, s, rsdpN = _Kfields(K)
    lenud = int(np.sum(s[:rsdpN] ** 2) + 2 * np.sum(s[rsdpN:] ** 2))
    if frame_kind not in (FRAME_HOUSEHOLDER, FRAME_EXPLICIT):
        raise SdmError("frame_kind must be SDM_FRAME_HOUSEHOLDER (0) or SDM_FRAME_EXPLICIT (1)")
    lenfr = lenud + (int(np.sum(s[rsdpN:])) if frame_kind == FRAME_HOUSEHOLDER else 0)
    Kc, keep = capi.make_cone(lpN, q, s, rsdpN)
    return Kc, keep, lenud, int(np.sum(s)), lenfr, lpN, q.size, int(np.sum(q))


def psdframe_explicit(frms, K):
    """qb = the explicit unitary factor Qb of every PSD block (n x n, Hermitian blocks [Re; Im]; lenud x 1) out of qrK's Householder
    frames `frms` (lenud + hLen; qrK.c:86-227): Qb = Q_0 ... Q_{n-2} (diag(q) for Hermitian blocks), Q_k = I - c_k c_k^H / beta_k."""
    Kc, keep, lenud, slen, lenfr, _, _, _ = _frame_sizes(K, FRAME_HOUSEHOLDER)
    frms = f64(frms)
    if frms.size != lenfr:
        raise SdmError("frms size mismatch")
    qb = np.zeros(lenud, dtype=np.float64)
    check(capi.lib().sdm_psdframe_explicit(C.byref(Kc), pf(frms), pf(qb)))
    del keep
    return qb.reshape(-1, 1)


def psdframeit(lab, frms, K, frame_kind=0):
    """x = psdframeit(lab, frms, K): X = Qb' diag(lab) Qb per PSD block   (psdframeit.c:65-168).
    lab: sum(K.s) values, or the whole spectral vector (K.l + 2 length(K.q) + sum(K.s), psdframeit.c:134-137); frms: qrK's frames
    (frame_kind 0, lenud + hLen) or the explicit Qb (frame_kind 1, lenud).  Returns lenud x 1, every block exactly symmetric / Hermitian."""
    Kc, keep, lenud, slen, lenfr, lpN, nq, _ = _frame_sizes(K, frame_kind)
    lab, frms = f64(lab), f64(frms)
    if lab.size != slen:
        if lab.size != lpN + 2 * nq + slen:
            raise SdmError("lab size mismatch")
        lab = np.ascontiguousarray(lab[lpN + 2 * nq:])
    if frms.size != lenfr:
        raise SdmError("frms size mismatch")
    x = np.zeros(lenud, dtype=np.float64)
    check(capi.lib().sdm_psdframeit(C.byref(Kc), pf(lab), pf(frms), C.c_int(frame_kind), pf(x)))
    del keep
    return x.reshape(-1, 1)


def psdinvjmul(xlab, frms, y, K, frame_kind=0):
    """z = psdinvjmul(xlab, frms, y, K): X Z + Z X = 2 Y for X = Qb' diag(xlab) Qb, per PSD block   (psdinvjmul.c:101-227).
    xlab as `lab` of psdframeit; y: lenud values or a whole cone vector (K.l + sum(K.q) + lenud, psdinvjmul.c:195-198), of which only the
    lower triangle of every block is read.  Returns lenud x 1, every block exactly symmetric / Hermitian."""
    Kc, keep, lenud, slen, lenfr, lpN, nq, qdim = _frame_sizes(K, frame_kind)
    xlab, frms, y = f64(xlab), f64(frms), f64(y)
    if y.size != lenud:
        if y.size != lpN + qdim + lenud:
            raise SdmError("size y mismatch")
        y = np.ascontiguousarray(y[lpN + qdim:])
    if xlab.size != slen:
        if xlab.size != lpN + 2 * nq + slen:
            raise SdmError("size xlab mismatch")
        xlab = np.ascontiguousarray(xlab[lpN + 2 * nq:])
    if frms.size != lenfr:
        raise SdmError("size xfrm mismatch")
    z = np.zeros(lenud, dtype=np.float64)
    check(capi.lib().sdm_psdinvjmul(C.byref(Kc), pf(xlab), pf(frms), C.c_int(frame_kind), pf(y), pf(z)))
    del keep
    return z.reshape(-1, 1)


def set_frame_lds_budget(nbytes):
    """LDS bytes per column strip of the frame expansion (sdm_set_frame_lds_budget), 0 = default."""
    check(capi.lib().sdm_set_frame_lds_budget(C.c_int64(int(nbytes))))


# ------------------------------------------------------------- next row
def qrK(x, K, nlhs=1, frame_kind=FRAME_HOUSEHOLDER):
    """[q, r] = qrK(x, K): x = Qb R per PSD block in the reference's conventions (qrK.c:86-296; include/sedumi_hip.h at sdm_qrk).
    x: lenud values, the PSD part only.  q: qrK's compact Householder frames (frame_kind 0, lenud + hLen) or the explicit Qb (frame_kind 1,
    lenud); r: lenud x 1, triu = R (real blocks: the diagonal may be negative), strict lower triangle 0; only fetched with nlhs > 1."""
    Kc, keep, lenud, slen, lenfr, _, _, _ = _frame_sizes(K, frame_kind)
    x = f64(x)
    if x.size != lenud:
        raise SdmError("size mismatch x")
    q = np.zeros(lenfr, dtype=np.float64)
    r = np.zeros(lenud, dtype=np.float64) if nlhs > 1 else None
    check(capi.lib().sdm_qrk(C.byref(Kc), pf(x), C.c_int(frame_kind), pf(q), pf(r) if r is not None else None))
    del keep
    return (q.reshape(-1, 1), r.reshape(-1, 1)) if nlhs > 1 else q.reshape(-1, 1)


def set_qr_panel_lds_budget(nbytes):
    """LDS bytes the panel of a block may take in qrK's panel step (sdm_set_qr_panel_lds_budget), 0 = default."""
    check(capi.lib().sdm_set_qr_panel_lds_budget(C.c_int64(int(nbytes))))


# ------------------------------------------------------------- next row
def urotorder(u, K, maxu, permIN=None, nlhs=4):
    """[u, perm, gjc, g] = urotorder(u, K, maxu, permIN): stable re-pivoting of the triu factor by Givens rotations per PSD block
    (urotorder.c:79-490; include/sedumi_hip.h at sdm_urotorder).  Only the upper triangle of u is read.  gjc, g: the reference's compact
    rotation form (g is g_len x 1, 0 x 1 without a rotation); perm = permIN(p), or 1 + p without permIN.  Returns the first max(nlhs, 1) outputs."""
    Kc, keep, lenud, slen, _, _, _, _ = _frame_sizes(K, FRAME_HOUSEHOLDER)
    _, _, s, rsdpN = _Kfields(K)
    u = f64(u)
    if u.size != lenud:
        raise SdmError("u size mismatch")
    pin = None
    if permIN is not None and np.size(permIN) > 0:
        pin = f64(permIN)
        if pin.size != slen:
            raise SdmError("perm size mismatch")
    tri = s * (s - 1) // 2
    gcap = int(2 * np.sum(tri[:rsdpN]) + 3 * np.sum(tri[rsdpN:]))
    uo, po, gjc = np.zeros(lenud), np.zeros(slen), np.zeros(slen)
    g = np.zeros(max(gcap, 1))
    glen = C.c_int64(0)
    check(capi.lib().sdm_urotorder(C.byref(Kc), pf(u), C.c_double(float(np.asarray(maxu).ravel()[0])), pf(pin) if pin is not None else None,
                                   pf(uo), pf(po), pf(gjc), pf(g), C.byref(glen)))
    del keep
    assert not g[glen.value:].any()                              # (nothing is written beyond g_len)
    out = (uo.reshape(-1, 1), po.reshape(-1, 1), gjc.reshape(-1, 1), g[:glen.value].copy().reshape(-1, 1))
    return out[:nlhs] if nlhs > 1 else out[0]


def givensrot(gjc, g, x, K):
    """y = givensrot(gjc, g, x, K): Y = G X per PSD block, gjc and g as urotorder leaves them (givensrot.c:60-168)."""
    Kc, keep, lenud, slen, _, _, _, _ = _frame_sizes(K, FRAME_HOUSEHOLDER)
    gjc, g, x = f64(gjc), f64(g), f64(x)
    if x.size != lenud:
        raise SdmError("x size mismatch")
    if gjc.size != slen:
        raise SdmError("gjc size mismatch")
    y = np.zeros(lenud, dtype=np.float64)
    check(capi.lib().sdm_givensrot(C.byref(Kc), pf(gjc), pf(g) if g.size else None, C.c_int64(g.size), pf(x), pf(y)))
    del keep
    return y.reshape(-1, 1)


def sqrtinv(q, vlab, K):
    """y = sqrtinv(q, vlab, K): y(i, j) = conj(q(j, i)) / sqrt(v_i) per PSD block (sqrtinv.c:58-145); vlab the whole spectral vector
    (K.l + 2 length(K.q) + sum(K.s)) or its PSD part."""
    Kc, keep, lenud, slen, _, _, _, _ = _frame_sizes(K, FRAME_HOUSEHOLDER)
    q, vlab = f64(q), f64(vlab)
    if q.size != lenud:
        raise SdmError("q size mismatch")
    y = np.zeros(lenud, dtype=np.float64)
    check(capi.lib().sdm_sqrtinv(C.byref(Kc), pf(q), pf(vlab) if vlab.size else None, C.c_int64(vlab.size), pf(y)))
    del keep
    return y.reshape(-1, 1)


def set_rot_lds_budget(nbytes):
    """LDS bytes urotorder's working copy / givensrot's column strip may take (sdm_set_rot_lds_budget), 0 = default."""
    check(capi.lib().sdm_set_rot_lds_budget(C.c_int64(int(nbytes))))


# ------------------------------------------------------------- next row
def triumtriu(x, y, K):
    """z = triumtriu(x, y, K): Z = triu(X) triu(Y) per PSD block, then the strict lower triangle = the conjugate of the strict upper one
    (triumtriu.m:40-71; include/sedumi_hip.h at sdm_triumtriu).  x, y: lenud values each or any longer vectors of one length (a whole cone vector),
    of which the last lenud are taken; only their upper triangles are read.  Returns lenud x 1; the diagonal of a Hermitian block as computed."""
    Kc, keep, lenud, slen, _, _, _, _ = _frame_sizes(K, FRAME_HOUSEHOLDER)
    x, y = f64(x), f64(y)
    if x.size != y.size or x.size < lenud:
        raise SdmError("triumtriu: size mismatch")
    z = np.zeros(lenud, dtype=np.float64)
    check(capi.lib().sdm_triumtriu(C.byref(Kc), pf(x), pf(y), C.c_int64(x.size), pf(z)))
    del keep
    return z.reshape(-1, 1)


def updtransfo_psd(ux, u, perm, q, vlab, K, maxu=1.1, frame_kind=FRAME_HOUSEHOLDER):
    """(u, perm, frame) = the PSD part of updtransfo.m:99-108 as ONE call of the library (include/sedumi_hip.h at sdm_updtransfo_psd):
        du = triumtriu(ux, u, K); [du, perm, gjc, g] = urotorder(du, K, maxu, perm); q = givensrot(gjc, g, q, K); vinv = sqrtinv(q, vlab, K);
        [frame, r] = qrK(vinv, K); u = triumtriu(r, du, K)
    bit-equal to those six calls.  ux, u: lenud values or longer vectors (the last lenud are taken, as triumtriu does); perm: sum(K.s) 1-based values,
    empty / None = none; q: lenud; vlab as sqrtinv's; frame: qrK's Householder frames (frame_kind 0, lenud + hLen) or the explicit Qb (1, lenud)."""
    Kc, keep, lenud, slen, lenfr, _, _, _ = _frame_sizes(K, frame_kind)
    ux, u, q, vlab = f64(ux), f64(u), f64(q), f64(vlab)
    if ux.size < lenud or u.size < lenud:
        raise SdmError("triumtriu: size mismatch")
    ux, u = np.ascontiguousarray(ux[ux.size - lenud:]), np.ascontiguousarray(u[u.size - lenud:])
    if q.size != lenud:
        raise SdmError("q size mismatch")
    pin = None
    if perm is not None and np.size(perm) > 0:
        pin = f64(perm)
        if pin.size != slen:
            raise SdmError("perm size mismatch")
    uo, po, fr = np.zeros(lenud), np.zeros(slen), np.zeros(lenfr)
    check(capi.lib().sdm_updtransfo_psd(C.byref(Kc), pf(ux), pf(u), pf(pin) if pin is not None else None, pf(q), pf(vlab) if vlab.size else None,
                                        C.c_int64(vlab.size), C.c_double(float(np.asarray(maxu).ravel()[0])), C.c_int(frame_kind), pf(uo), pf(po), pf(fr)))
    del keep
    return uo.reshape(-1, 1), po.reshape(-1, 1), fr.reshape(-1, 1)


# ------------------------------------------------------------- next row
def _psd_tail(who, v, lenud):
    v = f64(v)
    if v.size < lenud:
        raise SdmError(who + ": size mismatch")
    return v


def psdfactor(x, K, nlhs=1):
    """[ux, ispos] = psdfactor(x, K): X = L L' per PSD block, ux = L + tril(L,-1)' (psdfactor.m:44-80; include/sedumi_hip.h at sdm_psdfactor).
    x: lenud values or any longer vector (a whole cone vector), of which the last lenud are taken; only the lower triangles and the real part of
    the diagonals are read.  ispos False: a block is not positive definite and ux is zero from that block on.  Returns ux (lenud x 1), with
    nlhs > 1 (ux, ispos)."""
    Kc, keep, lenud, slen, _, _, _, _ = _frame_sizes(K, FRAME_HOUSEHOLDER)
    x = _psd_tail("psdfactor", x, lenud)
    ux = np.zeros(lenud, dtype=np.float64)
    ispos = C.c_int(1)
    check(capi.lib().sdm_psdfactor(C.byref(Kc), pf(x), C.c_int64(x.size), pf(ux), C.byref(ispos)))
    del keep
    return (ux.reshape(-1, 1), bool(ispos.value)) if nlhs > 1 else ux.reshape(-1, 1)


def psdinvscale(ud, x, K):
    """y = psdinvscale(ud, x, K): Y = T \\ X / T' per PSD block with T = triu(ud) (psdinvscale.m:40-83; include/sedumi_hip.h at sdm_psdinvscale).
    ud: lenud values, of which only the upper triangles are read; x: lenud values or a longer vector (the last lenud are taken), not assumed
    symmetric.  Returns lenud x 1, Im diag = 0 on Hermitian blocks."""
    Kc, keep, lenud, slen, _, _, _, _ = _frame_sizes(K, FRAME_HOUSEHOLDER)
    ud = f64(ud)
    if ud.size != lenud:
        raise SdmError("psdinvscale: ud size mismatch")
    x = _psd_tail("psdinvscale", x, lenud)
    y = np.zeros(lenud, dtype=np.float64)
    check(capi.lib().sdm_psdinvscale(C.byref(Kc), pf(ud), pf(x), C.c_int64(x.size), pf(y)))
    del keep
    return y.reshape(-1, 1)


def psdscale_u(ud, x, K, transp=False):
    """y = psdscale(ud, x, K, transp) for a bare factor ud (no pivot order): Y = T' X T per PSD block, T = tril(ud), with transp triu(ud)
    (psdscale.m:76-119; include/sedumi_hip.h at sdm_psdscale).  Lengths as psdinvscale.  Returns lenud x 1, Im diag = 0 on Hermitian blocks."""
    Kc, keep, lenud, slen, _, _, _, _ = _frame_sizes(K, FRAME_HOUSEHOLDER)
    ud = f64(ud)
    if ud.size != lenud:
        raise SdmError("psdscale: ud size mismatch")
    x = _psd_tail("psdscale", x, lenud)
    y = np.zeros(lenud, dtype=np.float64)
    check(capi.lib().sdm_psdscale(C.byref(Kc), pf(ud), pf(x), C.c_int64(x.size), C.c_int(1 if transp else 0), pf(y)))
    del keep
    return y.reshape(-1, 1)


def trydif_psd(x, z, K):
    """(ux, s, ispos) = trydif.m:62-63 / widelen.m:101-103 as ONE call of the library (include/sedumi_hip.h at sdm_trydif_psd):
        [ux, ispos] = psdfactor(x, K); s = psdscale(ux, z, K)
    bit-equal to psdfactor followed by psdscale_u.  x, z: vectors of one length, lenud or longer (the last lenud are taken)."""
    Kc, keep, lenud, slen, _, _, _, _ = _frame_sizes(K, FRAME_HOUSEHOLDER)
    x, z = _psd_tail("trydif_psd", x, lenud), _psd_tail("trydif_psd", z, lenud)
    if x.size != z.size:
        raise SdmError("trydif_psd: size mismatch")
    ux, s = np.zeros(lenud, dtype=np.float64), np.zeros(lenud, dtype=np.float64)
    ispos = C.c_int(1)
    check(capi.lib().sdm_trydif_psd(C.byref(Kc), pf(x), pf(z), C.c_int64(x.size), pf(ux), pf(s), C.byref(ispos)))
    del keep
    return ux.reshape(-1, 1), s.reshape(-1, 1), bool(ispos.value)


# ------------------------------------------------------------- next row
def psdeig(x, K, nlhs=1):
    """[lab, q] = psdeig(x, K): per PSD block the eigenvalues of X + X', halved, ascending, and -- nlhs > 1 -- the eigenvectors in that order, each of
    norm 1, Hermitian blocks as [Re; Im] planes (psdeig.m:44-93; include/sedumi_hip.h at sdm_psdeig).  x: lenud values or any longer vector (a whole
    cone vector), of which the last lenud are taken.  Returns lab (sum(K.s) x 1), with nlhs = 2 (lab, q), with nlhs = 3 (lab, q, info): info is -1,
    or the first block that is not done (an entry that is not finite, or no convergence at the sweep cap), whose lab and q are NaN.  lab is the
    same bit for bit whether q is asked for or not.  An empty K.s gives the .m file's []."""
    Kc, keep, lenud, slen, _, _, _, _ = _frame_sizes(K, FRAME_HOUSEHOLDER)
    x = _psd_tail("psdeig", x, lenud)
    if _Kfields(K)[2].size == 0:
        e = np.zeros((0, 0))
        return (e, e, -1)[:nlhs] if nlhs > 1 else e
    lab = np.zeros(slen, dtype=np.float64)
    q = np.zeros(lenud, dtype=np.float64) if nlhs > 1 else None
    info = C.c_int(-1)
    check(capi.lib().sdm_psdeig(C.byref(Kc), pf(x), C.c_int64(x.size), pf(lab), pf(q), C.byref(info)))
    del keep
    if nlhs <= 1:
        return lab.reshape(-1, 1)
    return (lab.reshape(-1, 1), q.reshape(-1, 1), int(info.value))[:nlhs]


def minpsdeig(x, K, nlhs=1):
    """mineig = minpsdeig(x, K): the smallest entry of psdeig's lab, bit for bit, from the values-only solve and a minimum on the device
    (minpsdeig.m:40-75; include/sedumi_hip.h at sdm_minpsdeig).  Returns 1 x 1 (NaN when a block is not done), with nlhs = 2 (mineig, info); an
    empty K.s gives the .m file's []."""
    Kc, keep, lenud, slen, _, _, _, _ = _frame_sizes(K, FRAME_HOUSEHOLDER)
    x = _psd_tail("minpsdeig", x, lenud)
    if _Kfields(K)[2].size == 0:
        return (np.zeros((0, 0)), -1) if nlhs > 1 else np.zeros((0, 0))
    m, info = C.c_double(0.0), C.c_int(-1)
    check(capi.lib().sdm_minpsdeig(C.byref(Kc), pf(x), C.c_int64(x.size), C.byref(m), C.byref(info)))
    del keep
    out = np.array([[m.value]], dtype=np.float64)
    return (out, int(info.value)) if nlhs > 1 else out


def psdeig_last_sweeps():
    """the sweeps the calling thread's last psdeig / minpsdeig call made"""
    return int(capi.lib().sdm_psdeig_last_sweeps())


# ------------------------------------------------------------- next row
def psdjmul(x, y, K):
    """z = psdjmul(x, y, K): Z = (X Y + (X Y)') / 2 per PSD block (psdjmul.m:40-73; include/sedumi_hip.h at sdm_psdjmul).  x, y: lenud values each
    or any longer vectors of one length (a whole cone vector), of which the last lenud are taken; the full blocks are read, no symmetry assumed.
    Returns lenud x 1, every block exactly symmetric / Hermitian with Im diag = 0; an empty K.s gives the .m file's []."""
    Kc, keep, lenud, slen, _, _, _, _ = _frame_sizes(K, FRAME_HOUSEHOLDER)
    x, y = f64(x), f64(y)
    if x.size != y.size or x.size < lenud:
        raise SdmError("psdjmul: size mismatch")
    z = np.zeros(lenud, dtype=np.float64)
    check(capi.lib().sdm_psdjmul(C.byref(Kc), pf(x), pf(y), C.c_int64(x.size), pf(z)))
    del keep
    return z.reshape(-1, 1)


def maxstep_psd(ud, dx, K, nlhs=1):
    """mineig = maxstep.m:63 as ONE call of the library (include/sedumi_hip.h at sdm_maxstep_psd): minpsdeig(psdinvscale(ud, dx, K), K), bit-equal to
    those two calls.  ud: lenud values; dx: lenud values or a longer vector (the last lenud are taken).  Returns 1 x 1 (NaN when a block is not done),
    with nlhs = 2 (mineig, info); without PSD blocks +Inf and -1."""
    Kc, keep, lenud, slen, _, _, _, _ = _frame_sizes(K, FRAME_HOUSEHOLDER)
    ud = f64(ud)
    if ud.size != lenud:
        raise SdmError("maxstep_psd: ud size mismatch")
    dx = _psd_tail("maxstep_psd", dx, lenud)
    m, info = C.c_double(0.0), C.c_int(-1)
    check(capi.lib().sdm_maxstep_psd(C.byref(Kc), pf(ud), pf(dx), C.c_int64(dx.size), C.byref(m), C.byref(info)))
    del keep
    out = np.array([[m.value]], dtype=np.float64)
    return (out, int(info.value)) if nlhs > 1 else out


def wstruct_psd(x, z, K):
    """(ux, s, lab, ispos, info) = widelen.m:101-104 / trydif.m:62-64 as ONE call of the library (include/sedumi_hip.h at sdm_wstruct_psd):
        [ux, ispos] = psdfactor(x, K); s = psdscale(ux, z, K); lab = psdeig(s, K)
    bit-equal to trydif_psd followed by psdeig (the values alone).  x, z: vectors of one length, lenud or longer (the last lenud are taken); info is
    -1, or the first block of s whose eigenvalues are not done (lab NaN there)."""
    Kc, keep, lenud, slen, _, _, _, _ = _frame_sizes(K, FRAME_HOUSEHOLDER)
    x, z = _psd_tail("wstruct_psd", x, lenud), _psd_tail("wstruct_psd", z, lenud)
    if x.size != z.size:
        raise SdmError("wstruct_psd: size mismatch")
    ux, s, lab = np.zeros(lenud, dtype=np.float64), np.zeros(lenud, dtype=np.float64), np.zeros(slen, dtype=np.float64)
    ispos, info = C.c_int(1), C.c_int(-1)
    check(capi.lib().sdm_wstruct_psd(C.byref(Kc), pf(x), pf(z), C.c_int64(x.size), pf(ux), pf(s), pf(lab), C.byref(ispos), C.byref(info)))
    del keep
    return ux.reshape(-1, 1), s.reshape(-1, 1), lab.reshape(-1, 1), bool(ispos.value), int(info.value)
