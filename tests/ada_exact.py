"""tests/ada_exact.py -- TEST INFRASTRUCTURE: ADA' and absd in extended precision (numpy longdouble, 64-bit mantissa) from the
library's own inputs, real symmetric AND Hermitian PSD blocks, with the componentwise scale every entry's error is judged by.

Semantics (getada1.c / getada2.c / getada3.c, spscale.c's real and complex D X D):

  ada_ij  = sum_r a_ri dsqr_r a_rj  +  sum_k q_ki q_kj  +  sum_blocks sum_p a_i[p] z_j[p]          (then symmetrised)
  z_j     = planes of Z_j = D herm(X_j) D per block, herm(X) = (X + X^H) / 2, X_j the stored (folded) nonzeros of constraint j read
            as Re X + i Im X (Hermitian blocks: rows [vec(Re); vec(Im)], D likewise); p runs over the stored nonzeros of a_i
  absd_j  = (LP / Lorentz part of ada_jj) + sum_p |a_j[p] z_j[p]|   for constraints with PSD nonzeros, 0 for the others

The scale s_ij is the same sum with every TERM replaced by its absolute value, down to the products d_ra h_ab d_bc of which
z_j[p] is made (real plane: the products with an even number of imaginary factors, imaginary plane: those with an odd number).
A correctly rounded evaluation in any order stays within (number of terms) x 2^-53 of it: err(M) = max_ij |M_ij - X_ij| / s_ij is
a componentwise measure, in which a wrong small entry is not hidden under a large one.

Plain numpy, no reference text; only tests import this module."""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
CLD = np.clongdouble


def _layout(K):
    q = np.asarray(K["q"], dtype=np.float64).ravel().astype(np.int64)
    s = np.asarray(K["s"], dtype=np.float64).ravel().astype(np.int64)
    nreal = int(np.asarray(K.get("rsdpN", s.size)).ravel()[0])
    bs = np.asarray(K["blkstart"], dtype=np.float64).ravel().astype(np.int64) - 1
    return int(np.asarray(K["l"]).ravel()[0]), q, s, nreal, bs[1 + q.size:]


def block_matrices(x, n, herm, dtype):
    """The n x n matrix a block's rows stand for: vec(X) (real block) or [vec(Re X); vec(Im X)] (Hermitian block)."""
    if not herm:
        return x.reshape(n, n, order="F").astype(dtype)
    return x[:n * n].reshape(n, n, order="F").astype(dtype) + 1j * x[n * n:].reshape(n, n, order="F").astype(dtype)


def block_scalings(K, udsqr):
    """[D_k] in extended precision (real blocks real, Hermitian blocks complex) from udsqr = [vec(D_k)], Hermitian blocks
    [vec(Re D_k); vec(Im D_k)]."""
    _, _, s, nreal, _ = _layout(K)
    ud = np.asarray(udsqr, dtype=np.float64).ravel()
    out, off = [], 0
    for k, n in enumerate(s):
        ln = (1 if k < nreal else 2) * n * n
        out.append(block_matrices(ud[off:off + ln], n, k >= nreal, CLD if k >= nreal else LD))
        off += ln
    return out


def ada_exact(At, K, d, DAtq, udsqr, drop=None):
    """(ADA', absd, S, sabsd): dense ADA' (m x m) and absd in longdouble and their scales (float64), see the module text.
    drop = (j, k, part, col): leave the nonzeros of column `col` of plane `part` (0 real, 1 imaginary) of block k out of X_j when
    forming z_j -- a deliberately WRONG value, for tests that prove a comparison can fail."""
    At = sp.csc_matrix(At)
    N, m = At.shape
    lpN, q, s, nreal, psd = _layout(K)
    psd0 = int(psd[0]) if s.size else N
    det = np.asarray(d["det"], dtype=np.float64).ravel()
    dsqr = np.concatenate([np.asarray(d["l"], dtype=np.float64).ravel()[:lpN], -det] + [np.full(nk - 1, det[k]) for k, nk in enumerate(q)])[:psd0]
    Alq = At[:psd0, :].toarray()
    X = (Alq.T.astype(LD) * dsqr.astype(LD)) @ Alq.astype(LD)
    S = (np.abs(Alq).T * np.abs(dsqr)) @ np.abs(Alq)
    if DAtq is not None and DAtq.shape[0] > 0:
        Q = sp.csc_matrix(DAtq).toarray()
        X = X + Q.T.astype(LD) @ Q.astype(LD)
        S = S + np.abs(Q).T @ np.abs(Q)
    base, sbase = np.diag(X).copy(), np.diag(S).copy()
    absd, sabsd = np.zeros(m, dtype=LD), np.zeros(m)
    Ds = block_scalings(K, udsqr)
    Acsr = sp.csr_matrix(At)
    haspsd = np.zeros(m, dtype=bool)
    for k, n in enumerate(s):
        herm = k >= nreal
        B = sp.csc_matrix(Acsr[int(psd[k]):int(psd[k + 1]), :])                    # the block's rows, all constraints
        U = np.unique(B.indices)                                                    # union pattern: the only places z is read at
        if U.size == 0:
            continue
        BU = B[U, :].toarray()
        D = Ds[k]
        Dr, Di = np.abs(D.real).astype(np.float64), np.abs(D.imag).astype(np.float64)
        ZU, ZS = np.zeros((U.size, m), dtype=LD), np.zeros((U.size, m))
        plane, pos = U // (n * n), U % (n * n)
        rr, cc = pos % n, pos // n
        for j in range(m):
            x = np.zeros(B.shape[0])
            sl = slice(B.indptr[j], B.indptr[j + 1])
            if sl.start == sl.stop:
                continue
            haspsd[j] = True
            x[B.indices[sl]] = B.data[sl]
            if drop is not None and drop[0] == j and drop[1] == k:
                x[drop[2] * n * n + drop[3] * n:drop[2] * n * n + (drop[3] + 1) * n] = 0.0
            Xj = block_matrices(x, n, herm, CLD if herm else LD)
            H = (Xj + Xj.conj().T) / 2
            act = np.flatnonzero((H != 0).any(axis=0))                              # herm(X) lives on act x act
            if act.size == 0:
                continue
            Hs = H[np.ix_(act, act)]
            Z = D[:, act] @ Hs @ D[act, :]
            Hr, Hi = np.abs(Hs.real).astype(np.float64), np.abs(Hs.imag).astype(np.float64)
            ar, ai = Dr[:, act], Di[:, act]
            if herm:
                even = ar @ Hr @ ar.T + ai @ Hi @ ar.T + ai @ Hr @ ai.T + ar @ Hi @ ai.T
                odd = ai @ Hr @ ar.T + ar @ Hi @ ar.T + ar @ Hr @ ai.T + ai @ Hi @ ai.T
                ZU[:, j] = np.where(plane == 0, Z.real[rr, cc], Z.imag[rr, cc])
                ZS[:, j] = np.where(plane == 0, even[rr, cc], odd[rr, cc])
            else:
                ZU[:, j] = Z[rr, cc]
                ZS[:, j] = (ar @ Hr @ ar.T)[rr, cc]
        X = X + BU.T.astype(LD) @ ZU
        S = S + np.abs(BU).T @ ZS
        absd += np.abs(BU.astype(LD) * ZU).sum(axis=0)
        sabsd += (np.abs(BU) * ZS).sum(axis=0)
    absd = np.where(haspsd, base + absd, LD(0)) if s.size else base.copy()
    sabsd = np.where(haspsd, sbase + sabsd, 0.0) if s.size else sbase.copy()
    return (X + X.T) / 2, absd, (S + S.T) / 2, sabsd


def err(M, X, S):
    """max over entries of |M - X| / S; an entry without any term (S = 0) must be exactly 0."""
    M = np.asarray(M.toarray() if sp.issparse(M) else M, dtype=np.float64).reshape(np.shape(X))
    diff = np.abs(M.astype(LD) - X)
    S = np.broadcast_to(np.asarray(S, dtype=np.float64), diff.shape)
    if (diff[S == 0] != 0).any():
        return float("inf")
    return float((diff[S > 0] / S[S > 0]).max()) if (S > 0).any() else 0.0


def negate_imaginary_plane(K, udsqr, k):
    """udsqr with the imaginary plane of D_k negated (D_k -> its transpose): a deliberately WRONG scaling for sensitivity checks."""
    _, _, s, nreal, _ = _layout(K)
    assert k >= nreal
    ud = np.array(udsqr, dtype=np.float64).ravel()
    off = int(sum((1 if i < nreal else 2) * s[i] ** 2 for i in range(k)))
    n = int(s[k])
    ud[off + n * n:off + 2 * n * n] *= -1.0
    return ud
