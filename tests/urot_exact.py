"""Shared by the urotorder / givensrot / sqrtinv tests: the cases, a numpy restatement of rotorder / prpirotorder
(urotorder.c:79-180, :197-304), the compiled reference's answers and the checks of a case on whichever library capi is bound to.

A case is ADMITTED only if the restatement -- run in float64 in the reference's operation order, and again with d kept in numpy.longdouble --
reproduces the compiled reference's perm and gjc exactly both times and every decision it takes (ukmax against maxu^2 d, the two largest d
at an argmax, d against h) has a relative gap >= 1e-7: the device's d differs from the reference's by rounding only, orders of magnitude
below that, so on an admitted case perm and gjc must be EQUAL.  `exact` = the restatement in longdouble with the reference's decisions
forced (gjc fixes them: step k pivots on position k + gjc[k+1] - gjc[k]).

Accuracy rule per block and part:  err(library) <= 10 err(reference) + 1e-15,  err(v) = max|v - exact| / max|exact|."""
import numpy as np

import psd_frames_exact as pfe
import qrk_exact as qe

LD = np.longdouble
MINGAP = 1e-7
MAXU = 1.1

# block shapes (problem.make_K(1, [], s, hs=hs)) and input variants; the seed of a case is its number in this list + 1 unless it names one
CASES = [
    dict(s=[1]), dict(s=[2]), dict(hs=[1]), dict(hs=[2]),              # no step or one step
    dict(s=[5]),
    dict(s=[63, 64, 65]),                                              # wavefront and tile edges
    dict(s=[130]),
    dict(s=[70, 35]),                                                  # control07's orders; the block offsets into gjc and g
    dict(s=[200, 3], hs=[66]),
    dict(hs=[70]),
    dict(s=[65], graded=True), dict(s=[130], graded=True),             # rows scaled by 10^(-14 i / n): the d-recompute branch several times per block
    dict(s=[33], hs=[34], junk=True),                                  # random junk below the diagonal: not read
    dict(s=[5, 33], hs=[6], maxu=1e3),                                 # already stable: identity perm, empty g, gjc all 0
    dict(s=[5, 33], hs=[6], perm_in=True),                             # permIN given (every other case omits it)
    dict(s=[300]),                                                     # more columns than work-items, a step with more rotations than one chunk (256)
]
GPU_ONLY_CASE = dict(s=[200, 200, 200], hs=[130])
GPU_ONLY_SEED = 1
RESIDENCE_CASE, RESIDENCE_SEED = dict(s=[65], hs=[33]), 1
# budgets of the residence check: everything in global memory (working copy, perm / pos / d, givensrot's strips); the Hermitian block's working
# copy (2 x 33 x 33 doubles = 17424 bytes) in LDS and the real one's (65 x 65 doubles = 33800 bytes) in global memory
RESIDENCE_BUDGETS = (1, 20000)


def seed_of(i):
    return CASES[i].get("seed", i + 1)


def _relgap(a, b):
    m = max(abs(a), abs(b))
    return float(abs(a - b) / m) if m > 0 else 0.0


def rotorder(M, maxusqr, work=np.float64, dd=np.float64, force=None):
    """rotorder / prpirotorder on triu(M): arithmetic on u and g in `work`, d in `dd`, every operation in the reference's order (float64 twice: the
    reference's bits up to the sign of zeros).  force: the number of rotations of every step (then d is not kept and no decision is taken).
    Returns dict(perm, gjc, g (flat, the reference's layout), U = triu(u(:, perm)), gaps)."""
    n = M.shape[0]
    herm = np.iscomplexobj(M)
    T = np.triu(M)
    ur = np.real(T).astype(work)
    ui = np.imag(T).astype(work) if herm else None
    if herm:
        ui[np.diag_indices(n)] = 0                                     # Im diag is never read (urotorder.c:224, :260)
    perm = np.arange(n)
    gjc = np.zeros(n, dtype=np.int64)
    gs = []
    d = np.zeros(n, dtype=dd)
    h = dd(1.0)
    gaps = dict(thr=np.inf, top=np.inf, h=np.inf)
    inz, recomp = 0, []
    for k in range(n - 1):
        gjc[k] = inz
        if force is None:
            pk = perm[k]
            gaps["h"] = min(gaps["h"], _relgap(d[pk], h))
            if d[pk] <= h:                                             # :102-108: every column summed from row k down, in order
                cols = perm[k:]
                s = np.cumsum(ur[k:, cols].astype(dd) ** 2, axis=0)[-1]
                if herm:
                    s = s + np.cumsum(ui[k:, cols].astype(dd) ** 2, axis=0)[-1]
                d[cols] = s
                h = d[pk] * dd(1e-10)
                recomp.append(k)
            later = perm[k + 1:]
            v = ur[k, later].astype(dd) ** 2
            if herm:
                v = v + ui[k, later].astype(dd) ** 2
            ukmax, thr = v.max(), dd(maxusqr) * d[pk]
            gaps["thr"] = min(gaps["thr"], _relgap(ukmax, thr))
            m = 0
            if ukmax > thr:
                dl = d[later]
                j = int(np.argmax(dl))                                 # the first among equal maxima (:123-128)
                assert dl[j] > 0
                if dl.size > 1:
                    two = np.sort(dl)[-2:]
                    gaps["top"] = min(gaps["top"], _relgap(two[1], two[0]))
                m = j + 1
        else:
            m = int(force[k])
        if m:
            pivk = k + m
            cp = perm[pivk]
            xr = ur[k:k + m, cp].copy()
            xi = ui[k:k + m, cp].copy() if herm else None
            last = ur[pivk, cp]
            sq = xr * xr + xi * xi if herm else xr * xr
            ys = np.cumsum(np.concatenate(([last * last], sq[::-1])))  # :139-143: y in the reference's order
            ny = np.sqrt(ys[1:][::-1])                                 # nexty of rotation r = 0 .. m-1
            prev = np.concatenate((ny[1:], [last]))
            gx, gy = xr / ny, prev / ny
            gxi = xi / ny if herm else None
            gs.append(np.stack((gx, gxi, gy), axis=1).ravel() if herm else np.stack((gx, gy), axis=1).ravel())
            ur[k, cp] = ny[0]; ur[k + 1:pivk + 1, cp] = 0              # (:149; the rotated-away entries are never read again)
            if herm:
                ui[k:pivk + 1, cp] = 0
            perm[k + 1:pivk + 1] = perm[k:pivk].copy(); perm[k] = cp
            cols = perm[k + 1:]
            # below its diagonal every column is 0 here, so the full form on all later columns equals givensrotuj on the first m of them
            ix = np.ix_(np.arange(k, pivk + 1), cols)
            Zr = ur[ix]
            Zi = ui[ix] if herm else None
            z2 = Zr[m].copy()
            z2i = Zi[m].copy() if herm else None
            for i in range(m, 0, -1):
                x, y = gx[i - 1], gy[i - 1]
                z1 = Zr[i - 1]
                if not herm:
                    Zr[i] = y * z1 - x * z2                            # auxgivens.c:57-58
                    z2 = x * z1 + y * z2
                else:
                    xim, z1i = gxi[i - 1], Zi[i - 1]
                    Zr[i] = y * z1 - x * z2 + xim * z2i                # :91-95
                    Zi[i] = y * z1i - x * z2i - xim * z2
                    t2 = x * z1 + xim * z1i + y * z2
                    z2i = x * z1i - xim * z1 + y * z2i
                    z2 = t2
            Zr[0] = z2
            ur[ix] = Zr
            if herm:
                Zi[0] = z2i
                ui[ix] = Zi
            if force is None:
                a = ur[k, cols].astype(dd)
                d[cols] -= (a * a + ui[k, cols].astype(dd) ** 2) if herm else a * a   # :169-172
            inz += m
    if n:
        gjc[n - 1] = inz
    U = np.triu(ur[:, perm])
    if herm:
        Ui = np.triu(ui[:, perm], 1)
        U = U + 1j * Ui if work is np.float64 else U.astype(np.clongdouble) + 1j * Ui.astype(np.clongdouble)
    return dict(perm=perm, gjc=gjc, g=np.concatenate(gs) if gs else np.zeros(0, dtype=work), U=U, gaps=gaps, recomp=recomp)


def apply_G(gjc, g, X, herm, work=LD):
    """Y = G X (matgivens / prpimatgivens, givensrot.c:60-84) in `work`, all columns at once"""
    n = X.shape[0]
    w = 3 if herm else 2
    g = np.asarray(g).astype(work).reshape(-1, w)
    Yr = np.real(X).astype(work)
    Yi = np.imag(X).astype(work) if herm else None
    for k in range(n - 1):
        g0, m = int(gjc[k]), int(gjc[k + 1] - gjc[k])
        if not m:
            continue
        z2 = Yr[k + m].copy()
        z2i = Yi[k + m].copy() if herm else None
        for i in range(m, 0, -1):
            z1 = Yr[k + i - 1]
            if not herm:
                x, y = g[g0 + i - 1]
                Yr[k + i] = y * z1 - x * z2
                z2 = x * z1 + y * z2
            else:
                x, xim, y = g[g0 + i - 1]
                z1i = Yi[k + i - 1]
                Yr[k + i] = y * z1 - x * z2 + xim * z2i
                Yi[k + i] = y * z1i - x * z2i - xim * z2
                t2 = x * z1 + xim * z1i + y * z2
                z2i = x * z1i - xim * z1 + y * z2i
                z2 = t2
        Yr[k] = z2
        if herm:
            Yi[k] = z2i
    if not herm:
        return Yr
    return (Yr + 1j * Yi) if work is np.float64 else Yr.astype(np.clongdouble) + 1j * Yi.astype(np.clongdouble)


def split(perm, gjc, g, K):
    """per block (perm as the gateway returned it, gjc as integers, the block's part of g) of a gateway's outputs"""
    perm, gjc, g = (np.asarray(v, dtype=np.float64).ravel() for v in (perm, gjc, g))
    out, o, og = [], 0, 0
    for n, herm in pfe.block_list(K):
        cnt = int(gjc[o + n - 1]) * (3 if herm else 2) if n else 0
        out.append((perm[o:o + n], gjc[o:o + n].astype(np.int64), g[og:og + cnt]))
        o += n; og += cnt
    assert og == g.size, (og, g.size)
    return out


def err(v, e):
    return qe.err(v, e)


_cache = {}


def make_case(refmex, kw, seed):
    """Inputs, the reference's answers, the admission of the case and the longdouble answers: computed once per session, shared by the emulator and
    the device tests, never modified."""
    key = (repr(sorted(kw.items())), seed)
    if key in _cache:
        return _cache[key]
    from sedumi_amd import problem
    K = problem.make_K(1, [], kw.get("s", []), hs=kw.get("hs", ()))
    rng = np.random.default_rng(seed)
    maxu = float(kw.get("maxu", MAXU))
    mats, ins = [], []
    for n, herm in pfe.block_list(K):
        M = np.triu(rng.standard_normal((n, n)))
        if herm:
            M = M + 1j * np.triu(rng.standard_normal((n, n)), 1)
        M[np.diag_indices(n)] = np.abs(np.real(np.diagonal(M))) + 0.5
        if kw.get("graded"):
            M = M * (10.0 ** (-14.0 * np.arange(n) / n))[:, None]
        mats.append(M)
        J = np.tril(rng.standard_normal((n, n)) * 1e3 + (1j * rng.standard_normal((n, n)) if herm else 0), -1) if kw.get("junk") else 0
        ins.append(M + J)
    u = pfe.pack_blocks(ins, K)
    slen = sum(n for n, _ in pfe.block_list(K))
    pin = np.concatenate([1.0 + rng.permutation(n) for n, _ in pfe.block_list(K)]) if kw.get("perm_in") else None
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)
    args = (col(u), K, maxu) + ((col(pin),) if pin is not None else ())
    uo, perm, gjc, g = (np.asarray(v, dtype=np.float64).ravel() for v in refmex.call("urotorder", 4, *args))
    ref = split(perm, gjc, g, K)
    # ---- admission, and `exact` with the reference's decisions
    E, recomp, mingap = [], [], dict(thr=np.inf, top=np.inf, h=np.inf)
    o = 0
    for M, (n, herm), (pr, gj, gg) in zip(mats, pfe.block_list(K), ref):
        p0 = (np.array([int(np.flatnonzero(pin[o:o + n] == v)[0]) for v in pr]) if pin is not None else pr - 1).astype(np.int64)
        for dd in (np.float64, LD):
            R = rotorder(M, maxu * maxu, np.float64, dd)
            assert np.array_equal(R["perm"], p0) and np.array_equal(R["gjc"], gj), ("not admitted: the restatement's decisions differ", kw, seed, n, dd)
            for name in mingap:
                mingap[name] = min(mingap[name], R["gaps"][name])
        recomp.append(R["recomp"])
        E.append(rotorder(M, maxu * maxu, LD, LD, force=np.diff(gj)))
        assert np.array_equal(E[-1]["perm"], p0)
        o += n
    print("admission", kw, "seed", seed, "smallest gaps", mingap)
    assert min(mingap.values()) >= MINGAP, ("not admitted: a decision is too close", kw, seed, mingap)
    # ---- givensrot on a random full x with the reference's rotations, sqrtinv
    xm = [rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if herm else 0) for n, herm in pfe.block_list(K)]
    x = pfe.pack_blocks(xm, K)
    yref = np.asarray(refmex.call("givensrot", 1, col(gjc), col(g), col(x), K), dtype=np.float64).ravel()
    Yx = [apply_G(gj, gg, X, herm) for X, (n, herm), (_, gj, gg) in zip(xm, pfe.block_list(K), ref)]
    vlab = 10.0 ** rng.uniform(-3, 3, slen)
    sref = np.asarray(refmex.call("sqrtinv", 1, col(x), col(np.concatenate(([1.0], vlab))), K), dtype=np.float64).ravel()   # (K.l = 1: the whole spectral vector)
    # the chain's inputs as updtransfo.m:102-107 hands them on: q unitary (the eigenvector frame), lab the spectrum of a point in the neighbourhood of
    # the central path (within a factor 2 of 1) -- qrK's input (G q diag(lab)^-1/2)^H then has condition number <= 2, so the unitary factor, which is as
    # sensitive as that number says, is determined to rounding and the rule compares roundings, not two amplifications of them
    qm = []
    for n, herm in pfe.block_list(K):
        Q, R = np.linalg.qr(rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if herm else 0))
        qm.append(Q)
    qchain, vchain = pfe.pack_blocks(qm, K), rng.uniform(0.5, 2.0, slen)
    c = dict(K=K, kw=kw, mats=mats, u=u, pin=pin, maxu=maxu, uo=uo, perm=perm, gjc=gjc, g=g, ref=ref, E=E, recomp=recomp, x=x, xm=xm, yref=yref, Yx=Yx, vlab=vlab,
             sref=sref, qm=qm, qchain=qchain, vchain=vchain, lab=10.0 ** rng.uniform(-3, 3, slen))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cache[key] = c
    return c


def check_rule(what, lib, ref, exact, K, part=""):
    """err(library) <= 10 err(reference) + 1e-15 per block; lib, ref, exact: one array per block"""
    bad = []
    for (n, herm), L, R, E in zip(pfe.block_list(K), lib, ref, exact):
        a, b = err(L, E), err(R, E)
        print("%-26s n=%-4d %s %-4s library %.2e  reference %.2e" % (what, n, "herm" if herm else "real", part, a, b))
        if not a <= 10 * b + 1e-15:
            bad.append((what, part, n, herm, a, b))
    assert not bad, bad


def run_library(c):
    from sedumi_amd import mex
    return tuple(np.asarray(v).ravel() for v in mex.urotorder(c["u"], c["K"], c["maxu"], c["pin"]))


def check_urotorder(c, out):
    """checks 1 - 3"""
    K = c["K"]
    uo, perm, gjc, g = out
    assert np.array_equal(perm, c["perm"]) and np.array_equal(gjc, c["gjc"])                      # 1
    lib = split(perm, gjc, g, K)
    check_rule("urotorder", [b[2] for b in lib], [b[2] for b in c["ref"]], [e["g"] for e in c["E"]], K, "g")   # 2
    check_rule("urotorder", [np.triu(U) for U in pfe.split_blocks(uo, K)], [np.triu(U) for U in pfe.split_blocks(c["uo"], K)], [e["U"] for e in c["E"]], K, "u")
    for U, (n, herm), (_, gj, gg) in zip(pfe.split_blocks(uo, K), pfe.block_list(K), lib):          # 3
        assert np.array_equal(np.real(U), np.real(U).T)
        if herm:
            assert np.array_equal(np.imag(U), -np.imag(U).T) and not np.imag(U).diagonal().any()
        assert gg.size == (3 if herm else 2) * (gj[n - 1] if n else 0)
    if c["kw"].get("maxu", MAXU) > 100:                                                             # the stable case
        assert g.size == 0 and not gjc.any() and np.array_equal(perm, c["pin"] if c["pin"] is not None else np.concatenate(
            [1.0 + np.arange(n) for n, _ in pfe.block_list(K)]))


def givens_matrices(gjc, g, K, call):
    """G of every block: call(gjc, g, identities, K)"""
    eye = pfe.pack_blocks([np.eye(n) + (0j if herm else 0) for n, herm in pfe.block_list(K)], K)
    return pfe.split_blocks(np.asarray(call(gjc, g, eye, K), dtype=np.float64).ravel(), K)


def check_invariants(refmex, c, out):
    """check 4: (G triu(u_in))(:, p) = triu(u_out) with G from the library's givensrot on the identity; |G^H G - I| by the rule against the reference's
    givensrot; the stability criterion on the output."""
    from sedumi_amd import mex
    K = c["K"]
    uo, perm, gjc, g = out
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)
    Gl = givens_matrices(gjc, g, K, mex.givensrot)
    Gr = givens_matrices(c["gjc"], c["g"], K, lambda a, b, x, K_: refmex.call("givensrot", 1, col(a), col(b), col(x), K_))
    el, er = [], []
    for G, Gf, M, U, e, (_, gj, _), rc in zip(Gl, Gr, c["mats"], pfe.split_blocks(uo, K), c["E"], split(perm, gjc, g, K), c["recomp"]):
        n = M.shape[0]
        cl = np.clongdouble if np.iscomplexobj(M) else LD
        GM = G.astype(cl) @ M.astype(cl)
        # Every entry passes at most two rotations per step, 2 n in all; a rotation applied in floating point, with its rounded x and y, perturbs a
        # column by at most 16 u of its 2-norm (u = 2^-53; real 6 u, Higham, Accuracy and Stability, Lemma 19.7; complex and the rounding of x, y on top).
        tol = 2 * n * 16 * 2.0 ** -53 * max(float(np.max(np.sqrt(np.sum(np.abs(M) ** 2, axis=0)))), 1e-300)
        dev = float(np.max(np.abs(GM[:, e["perm"]] - np.triu(U).astype(cl)))) if n else 0.0
        print("invariant  n=%-4d |(G triu(u))(:, p) - triu(u_out)| %.2e  bound %.2e" % (n, dev, tol))
        assert dev <= tol
        el.append(float(np.max(np.abs(G.astype(cl).conj().T @ G.astype(cl) - np.eye(n)))) if n else 0.0)
        er.append(float(np.max(np.abs(Gf.astype(cl).conj().T @ Gf.astype(cl) - np.eye(n)))) if n else 0.0)
        # The stability criterion on the output, as the reference's algorithm keeps it.  Its d_k is NOT u(k, k)^2: d is downdated only inside the pivot
        # branch (urotorder.c:169-172), so at step k the d of a column is the sum of |u(r, .)|^2 over the rows r from the last recompute (:102-108) on
        # that were not the row of a pivot step before k, and the reference's own output exceeds maxu^2 u(k, k)^2 (s=[5], seed 5: perm the identity,
        # row 1 has 2.41 u(1,1)^2; at pivot steps too, s=[65] of seed 6, row 48).  perm and gjc must EQUAL the reference's, so what holds on either
        # output, and is asserted, is what the reference tests (:122) and how it picks (:123-128), with d read off the output (rows above k are final at
        # step k, the rotations of later steps keep the norm of the rows from k down); the recompute steps are the float64 restatement's:
        #   a stable step k:  max_j |u(k, j)|^2 <= maxu^2 d_k;      a pivot step k:  d_k >= max_{j > k} d_j.
        # Slack: the running d is recomputed once it falls to 1e-10 of its value at the last recompute, so downdating leaves it a relative error of at
        # most n 2^-53 / 1e-10 (+ the 1e-12 of the criterion's own statement).
        a2, slack = np.abs(np.triu(U)) ** 2, 1 + n * 2.0 ** -53 / 1e-10 + 1e-12
        rows = np.zeros(n, dtype=bool)
        for r in range(n - 1):
            if r in rc:
                rows[:] = False; rows[r:] = True
            dcol = a2[rows].sum(axis=0)
            if gj[r + 1] > gj[r]:
                assert dcol[r + 1:].max() <= dcol[r] * slack, (n, r)
                rows[r] = False
            else:
                assert a2[r, r + 1:].max() <= c["maxu"] ** 2 * dcol[r] * slack, (n, r)
    for (n, herm), a, b in zip(pfe.block_list(K), el, er):
        print("invariant  n=%-4d |G^H G - I| library %.2e  reference %.2e" % (n, a, b))
        assert a <= 10 * b + 1e-15, (n, herm, a, b)


def check_givensrot(c):
    """check 5: the reference's gjc, g and a random full x"""
    from sedumi_amd import mex
    K = c["K"]
    y = mex.givensrot(c["gjc"], c["g"], c["x"], K).ravel()
    check_rule("givensrot", pfe.split_blocks(y, K), pfe.split_blocks(c["yref"], K), c["Yx"], K)
    return y


def check_sqrtinv(c):
    """check 6: one correctly rounded sqrt and one division per entry: within 2 ulp of the reference's, entry by entry (both forms of vlab)"""
    from sedumi_amd import mex
    K = c["K"]
    y = mex.sqrtinv(c["x"], c["vlab"], K).ravel()
    ulp = np.abs(y - c["sref"]) / np.spacing(np.abs(c["sref"]))
    print("sqrtinv    largest difference %.1f ulp%s" % (ulp.max() if ulp.size else 0.0, "  (bit-equal)" if np.array_equal(y, c["sref"]) else ""))
    assert (ulp <= 2).all()
    assert np.array_equal(y, mex.sqrtinv(c["x"], np.concatenate(([1.0], c["vlab"])), K).ravel())
    return y


def check_chain(refmex, c, out):
    """check 10: urotorder -> givensrot -> sqrtinv -> qrK -> psdframeit in the library against the same chain in the reference, by the rule;
    exact: the chain in longdouble on the reference's decisions"""
    from sedumi_amd import mex
    K = c["K"]
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)
    uo, perm, gjc, g = out
    X = mex.psdframeit(c["lab"], mex.qrK(mex.sqrtinv(mex.givensrot(gjc, g, c["qchain"], K), c["vchain"], K), K), K).ravel()
    if "chain" not in c:
        q = refmex.call("givensrot", 1, col(c["gjc"]), col(c["g"]), col(c["qchain"]), K)
        vinv = refmex.call("sqrtinv", 1, q, col(np.concatenate(([1.0], c["vchain"]))), K)
        frs = refmex.call("qrK", 2, vinv, K)[0]
        Xref = np.asarray(refmex.call("psdframeit", 1, col(c["lab"]), frs, K), dtype=np.float64).ravel()
        Qs, o = [], 0
        for Xm, e, (n, herm) in zip(c["qm"], c["E"], pfe.block_list(K)):
            Y = apply_G(e["gjc"], e["g"], Xm, herm)
            V = (Y / np.sqrt(c["vchain"][o:o + n].astype(LD))[None, :]).conj().T
            Qs.append(qe.exact_Qb(qe.exact_block(V))); o += n
        c["chain"] = (Xref, pfe.exact_frameit(Qs, c["lab"]))
    pfe.check_rule("chain -> psdframeit", X, c["chain"][0], c["chain"][1], K)


def check_case(refmex, kw, seed, full=None):
    """Checks 1 - 7 and 10 of a case; above 20000 matrix entries, where the emulator needs seconds per call, 1 - 3, 5 and 6 only."""
    c = make_case(refmex, kw, seed)
    if full is None:
        full = c["u"].size <= 20000
    out = run_library(c)
    check_urotorder(c, out)
    y = check_givensrot(c)
    s = check_sqrtinv(c)
    if not full:
        return
    check_invariants(refmex, c, out)
    from sedumi_amd import mex
    for a, b in zip(out, run_library(c)):                                                           # 7: two calls, the same bits
        assert np.array_equal(a, b)
    assert np.array_equal(y, mex.givensrot(c["gjc"], c["g"], c["x"], c["K"]).ravel()) and np.array_equal(s, mex.sqrtinv(c["x"], c["vlab"], c["K"]).ravel())
    if c["pin"] is None:                                                                            # an empty permIN is an absent one
        assert np.array_equal(np.asarray(mex.urotorder(c["u"], c["K"], c["maxu"], np.zeros(0))[1]).ravel(), out[1])
    check_chain(refmex, c, out)


def check_block_alone(refmex):
    """check 8: the block of order 65 alone gives the bits it has inside s=[130, 3, 65] (all three gateways)"""
    from sedumi_amd import mex, problem
    c3, c1 = make_case(refmex, dict(s=[130, 3, 65]), 1), None
    K3, K1 = c3["K"], problem.make_K(1, [], [65])
    M = c3["mats"][2]
    a3 = run_library(c3)
    a1 = tuple(np.asarray(v).ravel() for v in mex.urotorder(M.ravel(order="F"), K1, c3["maxu"]))
    l3 = split(a3[1], a3[2], a3[3], K3)[2]
    assert np.array_equal(a3[0][-65 * 65:], a1[0]) and np.array_equal(l3[0], a1[1]) and np.array_equal(l3[1], a1[2].astype(np.int64)) and np.array_equal(l3[2], a1[3])
    assert a1[3].size > 0
    x1 = c3["x"][-65 * 65:]
    assert np.array_equal(mex.givensrot(a3[2], a3[3], c3["x"], K3).ravel()[-65 * 65:], mex.givensrot(a1[2], a1[3], x1, K1).ravel())
    assert np.array_equal(mex.sqrtinv(c3["x"], c3["vlab"], K3).ravel()[-65 * 65:], mex.sqrtinv(x1, c3["vlab"][-65:], K1).ravel())


def check_residences(refmex):
    """check 9: with the working copy, perm / pos / d and the strips forced into global memory (all blocks; the real block only) the same bits as
    by default, and checks 1 - 5"""
    from sedumi_amd import mex
    c = make_case(refmex, RESIDENCE_CASE, RESIDENCE_SEED)
    out = run_library(c)
    y = mex.givensrot(c["gjc"], c["g"], c["x"], c["K"]).ravel()
    got = []
    try:
        for budget in RESIDENCE_BUDGETS:
            mex.set_rot_lds_budget(budget)
            got.append((run_library(c), mex.givensrot(c["gjc"], c["g"], c["x"], c["K"]).ravel()))
    finally:
        mex.set_rot_lds_budget(0)
    for o1, y1 in got:
        assert all(np.array_equal(a, b) for a, b in zip(out, o1)) and np.array_equal(y, y1)
    check_urotorder(c, out)
    check_invariants(refmex, c, out)
    check_givensrot(c)


def check_driver_switch():
    """check 12: solve() of a small SDP with a real and a Hermitian block with urotorder / givensrot / sqrtinv through the library (the reference's
    compact rotations and its pivot rule) against the default driver -- qe.check_driver_switch's bounds; and together with device_qr, device_cone"""
    from sedumi_amd.driver import solve
    from sedumi_amd.driver import loop as lp
    from sedumi_amd.driver.conemex import NativeMex
    assert NativeMex().device_rot is False and NativeMex(device_rot=True).device_rot is True and NativeMex(device_rot=True).device_qr is False
    r0 = solve(*pfe.small_hermitian_sdp(), hot=lp.HipHot())
    for kw in (dict(device_rot=True), dict(device_rot=True, device_qr=True, device_cone=True)):
        r1 = solve(*pfe.small_hermitian_sdp(), hot=lp.HipHot(), **kw)
        print(kw, "iter", r0["iter"], r1["iter"], "cx", r0["cx"], r1["cx"], "by", r0["by"], r1["by"])
        assert abs(r1["iter"] - r0["iter"]) <= 1 and r1["iter"] > 3
        assert abs(r1["cx"] - r0["cx"]) <= 1e-6 * abs(r0["cx"]) and abs(r1["by"] - r0["by"]) <= 1e-6 * abs(r0["by"])
        assert abs(r1["cx"] - r1["by"]) <= 1e-6 * (1 + abs(r1["cx"]))
