"""ADA' with Hermitian PSD blocks: the generic stage-1 kernel (k_psd_stage1, sedumi_amd/csrc/sdm_ada.hip) at the shapes its Hermitian
branch divides on, every stage-2 form a Hermitian problem can take, against an extended-precision ADA' (tests/ada_exact.py).

One Hermitian block sends the whole problem -- real blocks included -- to k_psd_stage1 (ada_psd: `A.sdpN == A.rsdpN` fails), so here
are: Hermitian orders 63 / 64 / 65 (one row group per lane pass), 70 and 130 (a dense task spans several chunks of CC slots), 260
(> 256); nslot = 1, 7, 8, 9 (the `flat` deal at 8 wavefronts), CC - 1, CC, CC + 1 and 2 n; tasks in the imaginary plane only, on the
real diagonal only, of one nonzero, of more nonzeros than are ever staged in LDS; real blocks of order 24 / 70 / 96 beside them
(register targets); LP rows and a Lorentz cone under the PSD part.

The measure is componentwise (ada_exact.err): |M_ij - X_ij| over the sum of the absolute values of all terms of entry (i, j).  The
library may be 10 x as far from the extended-precision value as the compiled reference is on the same inputs (+ 1e-15), the rule
tests/test_driver.py applies to ADA' on real scalings; the inputs are such that the reference itself is below 1e-13.

CPU tests run the emulator build of the same source, GPU tests (`-m gpu`) the hipcc build; both call the same check functions.
Every comparison prints its figures (pytest -s); profiles/r13a_ada_hermitian.txt holds those of a run on the MI355X."""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

import ada_exact as ax
from helpers import ROOT, TOL, relerr, use_emu, use_hip

NW = 8                                       # wavefronts of a k_psd_stage1 task (512 work-items): fewer slots than that are dealt `flat`
HS, SR = (63, 64, 65, 70, 130, 260), (24, 70, 96)
EDGES_REAL = (1, 4, 5, 31, 32, 33, 64, 65)


@functools.lru_cache(maxsize=None)
def plan_constants():
    """(S1_GEN_LDS, S1_NZ, S1_MAXN) from sedumi_amd/csrc/sdm_plan.h itself, compiled as the emulator build compiles the header."""
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "c.cpp"), os.path.join(tmp, "c")
        with open(src, "w") as f:
            f.write('#include "sdm_plan.h"\n#include <cstdio>\nint main() { std::printf("%d %d %d\\n", sdm::S1_GEN_LDS, sdm::S1_NZ, sdm::S1_MAXN); }\n')
        subprocess.check_call(["g++", "-std=c++17", "-DSDM_EMU", "-I", os.path.join(ROOT, "tests", "hipemu"), "-I", os.path.join(ROOT, "sedumi_amd", "csrc"),
                               "-o", exe, src])
        return tuple(int(x) for x in subprocess.check_output([exe], text=True).split())


def chunk_slots(n, herm, maxn, any_herm=True):
    """CC of a task of order n as ada_psd and k_psd_stage1 compute it: the launch's Y / D-row area is max(one slot of the largest block,
    min(stage1_lds, S1_GEN_LDS)) bytes (stage1_lds = max(96 KB, one slot)), a slot takes 2 n doubles (Hermitian: 4 n)."""
    gen = plan_constants()[0]
    one = (4 if any_herm else 2) * maxn * 8
    ldsy = max(one, min(max(96 * 1024, one), gen)) // 8
    return max(1, ldsy // (n * (4 if herm else 2)))


# ------------------------------------------------------------------ problems
def _hslots(rng, n, nslot, per, planes=(0, 1)):
    """(plane, row, col) positions in `nslot` distinct (plane, column) slots of a Hermitian block of order n, up to `per` rows in each:
    real plane rows >= col, imaginary plane rows > col (folded lower triangle; Im X has no diagonal)."""
    cand = [(0, c) for c in range(n) if 0 in planes] + [(1, c) for c in range(n - 1) if 1 in planes]
    pos = []
    for i in sorted(rng.choice(len(cand), size=nslot, replace=False)):
        p, c = cand[i]
        rows = c + p + rng.choice(n - c - p, size=min(per, n - c - p), replace=False)
        pos += [(p, int(r), c) for r in sorted(rows)]
    return pos


def _all_slots(rng, n):
    """Every real and every imaginary column: 2 n slots.  Column n - 1 of the imaginary plane has no strictly lower row, so its slot is
    the diagonal position (n - 1, n - 1): herm(X) and Im Z are zero there -- in the reference (spscale.c: both halves of the difference
    are the same sums), in the kernel and in exact arithmetic -- but the slot is formed and multiplied like any other."""
    return _hslots(rng, n, 2 * n - 1, 2) + [(1, n - 1, n - 1)]


def _rslots(rng, n, nslot, per):
    return [(0, r, c) for (_, r, c) in _hslots(rng, n, nslot, per, planes=(0,))]


def herm_specs(rng, n, cc, big=False, dense=True):
    """The tasks of a Hermitian block of order n (cc = its chunk length)."""
    specs = [_hslots(rng, n, ns, 3) for ns in sorted({1, NW - 1, NW, NW + 1, cc - 1, cc, cc + 1}) if ns <= 2 * n - 1]
    if dense:
        specs.append(_all_slots(rng, n))
    specs.append(_hslots(rng, n, 5, 4, planes=(1,)))                            # imaginary plane only
    specs.append(_hslots(rng, n, min(cc + 2, n - 1), 2, planes=(1,)))
    specs.append([(0, i, i) for i in range(n)])                                 # real diagonal only
    specs.append([(0, int(i), int(i)) for i in sorted(rng.choice(n, size=3, replace=False))])
    c = int(rng.integers(0, n - 1)); r = int(rng.integers(c + 1, n))
    specs += [[(0, c, c)], [(0, r, c)], [(1, r, c)]]                            # one nonzero: diagonal, real plane, imaginary plane
    if big:                                                                      # more nonzeros than S1_NZ: never staged
        tri = [(0, r, c) for c in range(n) for r in range(c, n)] + [(1, r, c) for c in range(n) for r in range(c + 1, n)]
        specs.append([tri[i] for i in sorted(rng.choice(len(tri), size=plan_constants()[1] + 464, replace=False))])
    return specs


def real_specs(rng, n):
    if n <= 32:
        return [_rslots(rng, n, 1, z) for z in (1, 2, 5)] + [_rslots(rng, n, ns, 2) for ns in (4, 5, n - 1, n)]
    return [_rslots(rng, n, ns, 3) for ns in EDGES_REAL + (n - 1, n) if ns <= n]


def assemble(K, per_col, rng, lp, name):
    """Problem from per_col[j] = [(block, [(plane, row, col), ...]), ...]: every constraint also gets the `lp` LP rows and entries in the
    Lorentz cones of K (trace and norm-bound rows)."""
    from sedumi_amd import problem
    start = K["sblkstart"].ravel().astype(np.int64) - 1
    ns = K["s"].ravel().astype(np.int64)
    bs = K["blkstart"].ravel().astype(np.int64) - 1
    nq = K["q"].size
    rows, cols, vals = [], [], []
    for j, tasks in enumerate(per_col):
        for r in range(1, lp + 1):
            rows.append(r); cols.append(j); vals.append(rng.standard_normal())
        for k in range(nq):
            if rng.random() < 0.8:
                rows.append(lp + 1 + k); cols.append(j); vals.append(rng.standard_normal())
            for r in range(bs[1 + k], bs[2 + k]):
                if rng.random() < 0.5:
                    rows.append(r); cols.append(j); vals.append(rng.standard_normal())
        for (k, pos) in tasks:
            n = int(ns[k])
            for (p, r, c) in pos:
                rows.append(start[k] + p * n * n + r + c * n); cols.append(j); vals.append(rng.standard_normal() * (1.0 if r == c else 2.0))
    At = sp.csc_matrix((vals, (rows, cols)), shape=(int(K["N"]), len(per_col)))
    return problem.Problem(At, K, name)


def herm_edge_problem(s=SR, hs=HS, seed=0, lp=3, q=(4,), big=True):
    """Every constraint has one task in every block; block k's task list is walked with an offset of 3 k, so single nonzeros sit beside
    dense tasks in a constraint.  The largest tasks (2 n slots, > S1_NZ nonzeros) are made for the blocks of order <= 130."""
    from sedumi_amd import problem
    rng = np.random.default_rng(seed)
    K = problem.make_K(lp + 1, list(q), list(s), list(hs))
    maxn = max(tuple(s) + tuple(hs))
    nbig = max([n for n in hs if n <= 70] or [min(hs)])
    specs = [real_specs(rng, n) for n in s] + [herm_specs(rng, n, chunk_slots(n, True, maxn), big=big and n == nbig, dense=n <= 130) for n in hs]
    m = max(len(x) for x in specs)
    per_col = [[(k, specs[k][(j + 3 * k) % len(specs[k])]) for k in range(len(specs))] for j in range(m)]
    return assemble(K, per_col, rng, lp, f"herm_edge_problem(s={s}, hs={hs})")


def mixed_pair(seed=5):
    """(real-only problem, the same constraints and real blocks with further constraints in a Hermitian block of order 66 behind them).
    No LP / Lorentz rows: the two ADA' share their leading m1 x m1 part, formed by k_psd_stage1_mfma in one and k_psd_stage1 in the other."""
    from sedumi_amd import problem
    rng = np.random.default_rng(seed)
    Kr, Kh = problem.make_K(1, [], list(SR)), problem.make_K(1, [], list(SR), [66])
    specs = [real_specs(rng, n) for n in SR]
    m1 = max(len(x) for x in specs)
    per_col = [[(k, specs[k][(j + 3 * k) % len(specs[k])]) for k in range(len(SR))] for j in range(m1)]
    hsp = herm_specs(rng, 66, chunk_slots(66, True, 96))
    st = np.random.default_rng(seed + 1).bit_generator.state
    out = []
    for K, pc in ((Kr, per_col), (Kh, per_col + [[(len(SR), x)] for x in hsp])):
        g = np.random.default_rng(); g.bit_generator.state = st                      # the same values in the shared constraints
        out.append(assemble(K, pc, g, 0, "mixed_pair"))
    return out[0], out[1], m1


def local_problem(seed=7, groups=6, per=8, n=10):
    """`groups` sets of constraints, each with a Hermitian block and an LP row of its own: a block-diagonal (sparse) ADA' pattern, an
    ordering that is not the identity, and more than 48 PSD nonzeros per constraint (stage 2 by wavefront, no ELL copy: pattern < 20 % full)."""
    from sedumi_amd import problem
    rng = np.random.default_rng(seed)
    K = problem.make_K(groups + 1, [], [], [n] * groups)
    tri = [(0, r, c) for c in range(n) for r in range(c, n)] + [(1, r, c) for c in range(n) for r in range(c + 1, n)]
    start = K["sblkstart"].ravel().astype(np.int64) - 1
    rows, cols, vals = [], [], []
    for j in rng.permutation(groups * per):
        g = int(j) % groups
        rows.append(1 + g); cols.append(int(j)); vals.append(rng.standard_normal())
        for i in sorted(rng.choice(len(tri), size=60, replace=False)):
            p, r, c = tri[i]
            rows.append(start[g] + p * n * n + r + c * n); cols.append(int(j)); vals.append(rng.standard_normal() * (1.0 if r == c else 2.0))
    At = sp.csc_matrix((vals, (rows, cols)), shape=(int(K["N"]), groups * per))
    return problem.Problem(At, K, "local_problem")


def variant_problem(kind):
    """Small blocks (the emulator's time), one per stage-2 form: see test_stage2_variants."""
    from sedumi_amd import problem
    if kind == "thread":
        return problem.random_sdp(m=40, lp=4, q=(3,), s=(6,), hs=(9, 5), dens=0.15, seed=21)
    if kind == "wave":
        return local_problem()
    m = {"ell1": 60, "ell2": 520, "ell4": 1030}[kind]
    return problem.random_sdp(m=m, lp=4, q=(3,), s=(12,), hs=(14, 9), dens=0.5, seed=22)


def stage2_kernel(P, pattern_nnz):
    """The stage-2 kernel ada_build / ada_psd choose for a problem with a Hermitian block: the ELL sweep when the rows are long (>= 48 PSD
    nonzeros per constraint), the pattern at least 20 % full and the full-length z (every block's union pattern) fits 96 KB; as many
    columns per workgroup (4 / 2 / 1) as m and 64 KB allow."""
    T = task_shapes(P)
    start = P.K["sblkstart"].ravel().astype(np.int64) - 1
    r = P.At.indices[P.At.indices >= start[0]]
    zmax = np.unique(r).size
    if sum(t["nnz"] for t in T) / P.m < 48 or pattern_nnz < 0.2 * P.m * P.m or zmax * 8 > 96 * 1024:
        return "k_psd_stage2"
    jb = 4 if (4 * zmax * 8 <= 64 * 1024 and P.m >= 1024) else 2 if (2 * zmax * 8 <= 64 * 1024 and P.m >= 512) else 1
    return f"k_psd_stage2_ell<{jb}>"


STAGE2 = {"thread": "k_psd_stage2", "wave": "k_psd_stage2", "ell1": "k_psd_stage2_ell<1>", "ell2": "k_psd_stage2_ell<2>", "ell4": "k_psd_stage2_ell<4>"}


# ------------------------------------------------------------------ shapes
def task_shapes(P):
    """Of every stage-1 task of P, as ada_build cuts them: dict(k, n, herm, nslot, nnz, imag (nonzeros in the imaginary plane), diag
    (nonzeros on the real diagonal))."""
    start = P.K["sblkstart"].ravel().astype(np.int64) - 1
    ns = P.K["s"].ravel().astype(np.int64)
    nreal = int(P.K["rsdpN"])
    out = []
    for j in range(P.m):
        r = P.At.indices[P.At.indptr[j]:P.At.indptr[j + 1]]
        for k, n in enumerate(ns):
            q = r[(r >= start[k]) & (r < start[k + 1])] - start[k]
            if q.size:
                part = q // (n * n); pos = q - part * n * n
                out.append(dict(j=j, k=k, n=int(n), herm=k >= nreal, nslot=int(np.unique(part * n + pos // n).size), nnz=int(q.size),
                                imag=int(part.sum()), diag=int(((part == 0) & (pos % n == pos // n)).sum())))
    return out


def test_edge_problem_has_the_shapes_it_is_for():
    gen, s1_nz, s1_maxn = plan_constants()
    P = herm_edge_problem()
    T = task_shapes(P)
    H = [t for t in T if t["herm"]]
    assert {t["n"] for t in H} == set(HS) and {63, 64, 65} <= set(HS) and max(HS) > 256
    for n in HS:
        cc = chunk_slots(n, True, max(HS))
        assert cc == (gen // 8) // (4 * n)
        want = {1, NW - 1, NW, NW + 1, cc - 1, cc, cc + 1} | ({2 * n} if n <= 130 else set())
        assert {t["nslot"] for t in H if t["n"] == n} >= want, (n, cc)
        assert any(t["imag"] == t["nnz"] and t["nslot"] > cc for t in H if t["n"] == n)          # imaginary plane only, more than a chunk
        assert any(t["diag"] == t["nnz"] == t["nslot"] == n for t in H if t["n"] == n)           # real diagonal only
        assert sum(1 for t in H if t["n"] == n and t["nnz"] == 1) >= 3                           # one nonzero
        assert any(t["nnz"] == 1 and t["imag"] == 1 for t in H if t["n"] == n)
    for n in (70, 130):                                                                          # a dense task spans several chunks
        assert 4 * chunk_slots(n, True, max(HS)) < 2 * n
    assert any(t["nnz"] > s1_nz for t in H)                                                     # never staged
    assert {t["n"] for t in T if not t["herm"]} == {24, 70, 96} and max(SR) <= s1_maxn           # real blocks the MFMA kernel would take alone
    assert int(P.K["l"]) > 1 and P.K["q"].size >= 1
    assert min(np.diff(P.At.indptr)) > 0 and all(sum(1 for t in T if t["j"] == j) == len(HS) + len(SR) for j in range(P.m))


# ------------------------------------------------------------------ the two sides of every comparison
def lorentz_values(P, d):
    """DAt.q (getDAtm.m: q1 times the trace rows plus q2' times the norm-bound rows of every Lorentz cone) on lorentz_pattern(P)."""
    from sedumi_amd import problem
    Q = problem.lorentz_pattern(P)
    nq = P.K["q"].size
    if nq == 0:
        return Q
    lpN = int(P.K["l"])
    bs = P.K["blkstart"].ravel().astype(np.int64) - 1
    A = sp.csr_matrix(P.At)
    Qd = np.asarray(d["q1"]).reshape(-1, 1) * A[lpN:lpN + nq, :].toarray()
    q2 = np.asarray(d["q2"]).ravel()
    for k in range(nq):
        Qd[k, :] += q2[bs[1 + k] - bs[1]:bs[2 + k] - bs[1]] @ A[bs[1 + k]:bs[2 + k], :].toarray()
    cols = np.repeat(np.arange(P.m), np.diff(Q.indptr))
    return sp.csc_matrix((Qd[Q.indices, cols], Q.indices, Q.indptr), shape=Q.shape)


def scaling(P, seed):
    from helpers import ref_scaling
    d, ud = ref_scaling(P, seed)
    return d, ud, lorentz_values(P, d)


def plan_ada(P, d, ud, Q, L=None, pattern=None, panels=None):
    """Dense ADA', absd and the kernels that ran (kprof) of the resident plan; panels = [(j0, j1), ...]: by getada_cols over them."""
    from sedumi_amd import problem
    from sedumi_amd.plan import Plan
    plan = Plan(0)
    plan.set_chol(L or problem.dense_symbolic(P.m), pattern if pattern is not None else problem.dense_pattern(P.m))
    plan.set_ada(P.At, P.Ablkjc, P.K, Q)
    plan.upload("dl", d["l"]); plan.upload("ddet", d["det"]); plan.upload("udsqr", ud)
    if Q.nnz:
        plan.upload("qpr", Q.data)
    plan.kprof(True)
    if panels is None:
        plan.getada()
    else:
        plan.upload("ada", np.full(plan.nnzADA, np.nan)); plan.upload("absd", np.full(P.m, np.nan))
        for j0, j1 in panels:
            plan.getada_cols(j0, j1)
    plan.sync()
    prof = plan.kprof_summary()
    plan.kprof(False)
    pat = plan.ADA_pattern
    ada = sp.csc_matrix((plan.download("ada"), pat.indices, pat.indptr), shape=pat.shape).toarray()
    absd = plan.download("absd")
    plan.close()
    return ada, absd, prof


def reference_ada(glue, P, d, ud, Q):
    """(setup, ADA2, ADA', absd) of the compiled reference: getada1 -> getada2 -> getada3 on its own pattern and orderings."""
    from oracle import glue as gl
    S = glue.setup(P.At, P.K)
    assert np.array_equal(S["Ablkjc"], P.Ablkjc)                           # (no dense column was split off)
    ref = glue.ref
    ADA1 = ref.call("getada1", 1, S["ADA"], S["A"], S["Ablkjc"][:, 2], S["Aord"]["lqperm"], {"l": gl._col(d["l"]), "det": gl._col(d["det"])},
                    P.K["qblkstart"])
    ADA2 = ref.call("getada2", 1, ADA1, {"q": Q}, S["Aord"], P.K)
    ADA3, absd3 = ref.call("getada3", 2, ADA2, S["A"], S["Ablkjc"][:, 2], S["Aord"], gl._col(ud), P.K)
    return S, ADA2, sp.csc_matrix(ADA3).toarray(), np.asarray(absd3).ravel()


def record(case, **figures):
    from sedumi_amd import capi
    print(f"ada_hermitian {capi.backend():10s} {case:20s} " + "  ".join(f"{k} {v:.2e}" for k, v in figures.items()))


def check_against_exact(glue, P, seed, case, stage2, sparse=False):
    """The resident plan and getada3 of the MEX route against the extended-precision ADA' (10 x the reference's own error + 1e-15,
    componentwise) and against the compiled reference (TOL); k_psd_stage1 and the stage-2 kernel `stage2` ran, k_psd_stage1_mfma did not."""
    from sedumi_amd import mex
    d, ud, Q = scaling(P, seed)
    X, xabsd, S, sabsd = ax.ada_exact(P.At, P.K, d, Q, ud)
    G, ADA2, R, rabsd = reference_ada(glue, P, d, ud, Q)
    e_ref, e_ref_d = ax.err(R, X, S), ax.err(rabsd, xabsd, sabsd)
    assert e_ref < 1e-13 and e_ref_d < 1e-13, (case, e_ref, e_ref_d)       # the allowance below cannot grow into a real error
    if sparse:
        assert G["ADA"].nnz < 0.2 * P.m * P.m and not np.array_equal(G["Aord"]["sperm"].ravel(), np.arange(1, P.m + 1))
        M, mabsd, prof = plan_ada(P, d, ud, Q, L=G["L"], pattern=G["ADA"])
    else:
        M, mabsd, prof = plan_ada(P, d, ud, Q)
    assert "k_psd_stage1" in prof and "k_psd_stage1_mfma" not in prof and stage2 in prof, sorted(prof)
    assert not [k for k in prof if k.startswith("k_psd_") and k not in ("k_psd_stage1", stage2)], sorted(prof)
    e_lib, e_lib_d = ax.err(M, X, S), ax.err(mabsd, xabsd, sabsd)
    A3, absd3 = mex.getada3(ADA2, G["A"], G["Ablkjc"][:, 2], G["Aord"], ud, P.K)
    absd3 = np.asarray(absd3).ravel()
    e_mex, e_mex_d = ax.err(A3, X, S), ax.err(absd3, xabsd, sabsd)
    record(case, e_ref=e_ref, e_plan=e_lib, e_getada3=e_mex, absd_ref=e_ref_d, absd_plan=e_lib_d, absd_getada3=e_mex_d)
    assert e_lib <= 10 * e_ref + 1e-15 and e_lib_d <= 10 * e_ref_d + 1e-15, (case, e_lib, e_ref, e_lib_d, e_ref_d)
    assert e_mex <= 10 * e_ref + 1e-15 and e_mex_d <= 10 * e_ref_d + 1e-15, (case, e_mex, e_ref, e_mex_d, e_ref_d)
    assert relerr(M, R) < TOL and relerr(mabsd, rabsd) < TOL and relerr(A3, R) < TOL and relerr(absd3, rabsd) < TOL
    return prof


def check_stage2_variant(glue, kind):
    P = variant_problem(kind)
    npsd = sum(t["nnz"] for t in task_shapes(P)) / P.m
    assert (npsd < 48) == (kind == "thread") and int(P.K["rsdpN"]) < P.K["s"].size
    assert {"ell1": P.m < 512, "ell2": 512 <= P.m < 1024, "ell4": P.m >= 1024}.get(kind, True)
    assert stage2_kernel(P, 0 if kind == "wave" else P.m * P.m) == STAGE2[kind]
    prof = check_against_exact(glue, P, 30 + len(kind), "stage2:" + kind, STAGE2[kind], sparse=kind == "wave")
    assert len([k for k in prof if k.startswith("k_psd_stage2")]) == 1


def check_edge_problem(glue):
    for P, seed, case in ((herm_edge_problem(), 41, "edge(63..260)"), (herm_edge_problem(s=(70,), hs=(64, 33), seed=3, q=(3, 5), big=False), 42, "edge(64,33)")):
        check_against_exact(glue, P, seed, case, stage2_kernel(P, P.m * P.m))


def check_column_panels():
    """sdm_plan_getada_cols over panels cut inside the constraints' task ranges (every constraint has a task in every block; a panel
    launch starts at task0 > 0 and cannot use the task ordering table): the union of the panels is plan.getada() bit for bit.  Without
    LP / Lorentz rows: their part of a whole ADA' may take the fused Gram form (ada_lq_q), which a panel never does."""
    P = herm_edge_problem(s=(24, 70), hs=(65, 130), seed=6, lp=0, q=())
    d, ud, Q = scaling(P, 43)
    M, mabsd, prof = plan_ada(P, d, ud, Q)
    cuts = [0, 1, 5, 6, P.m - 2, P.m]
    Mp, pabsd, pprof = plan_ada(P, d, ud, Q, panels=list(zip(cuts[:-1], cuts[1:])))
    assert "k_psd_stage1" in pprof and pprof["k_psd_stage1"][0] == len(cuts) - 1 and "k_psd_stage1_mfma" not in pprof
    assert np.array_equal(M, Mp) and np.array_equal(mabsd, pabsd)
    assert not np.isnan(M).any() and np.abs(M).min() > 0


def check_mixed_against_real_only(glue):
    """Blocks of order 24 / 70 / 96 alone (k_psd_stage1_mfma) and beside a Hermitian block on other constraints (k_psd_stage1, register
    targets): the same sums in another order.  Both within the allowance of the extended-precision value of the shared part, which is
    the same number for both problems; the rest of the larger ADA' couples nothing to it (exact zeros)."""
    Pr, Ph, m1 = mixed_pair()
    assert np.array_equal(Ph.At[:Pr.At.shape[0], :m1].toarray(), Pr.At.toarray()) and Ph.At[:Pr.At.shape[0], m1:].nnz == 0 and Ph.At[Pr.At.shape[0]:, :m1].nnz == 0
    d, udh, Q = scaling(Ph, 44)
    udr = udh[:sum(n * n for n in SR)]
    X, xabsd, S, sabsd = ax.ada_exact(Pr.At, Pr.K, d, None, udr)
    Mr, rabsd, rprof = plan_ada(Pr, d, udr, sp.csc_matrix((0, Pr.m)))
    Mh, habsd, hprof = plan_ada(Ph, d, udh, sp.csc_matrix((0, Ph.m)))
    assert "k_psd_stage1_mfma" in rprof and "k_psd_stage1" not in rprof and "k_psd_stage1" in hprof and "k_psd_stage1_mfma" not in hprof
    e_r, e_h = ax.err(Mr, X, S), ax.err(Mh[:m1, :m1], X, S)
    e_rd, e_hd = ax.err(rabsd, xabsd, sabsd), ax.err(habsd[:m1], xabsd, sabsd)
    _, _, R, refabsd = reference_ada(glue, Pr, dict(d, det=np.zeros(0)), udr, sp.csc_matrix((0, Pr.m)))
    e_ref, e_ref_d = ax.err(R, X, S), ax.err(refabsd, xabsd, sabsd)
    assert e_ref < 1e-13 and e_ref_d < 1e-13
    assert max(e_r, e_h) <= 10 * e_ref + 1e-15 and max(e_rd, e_hd) <= 10 * e_ref_d + 1e-15, (e_r, e_h, e_ref, e_rd, e_hd, e_ref_d)
    record("mixed(24,70,96|66)", e_ref=e_ref, e_mfma=e_r, e_generic=e_h, absd_ref=e_ref_d, absd_mfma=e_rd, absd_generic=e_hd)
    assert (Mh[:m1, m1:] == 0).all() and (Mh[m1:, :m1] == 0).all()


def check_determinism():
    P = herm_edge_problem()
    d, ud, Q = scaling(P, 41)
    a = plan_ada(P, d, ud, Q)
    b = plan_ada(P, d, ud, Q)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ------------------------------------------------------------------ the helper and the restatement themselves (CPU)
def test_exact_ada_agrees_with_the_restatement_on_real_problems():
    """Two plain evaluations of the same sums, one in longdouble: 1e-13 relative."""
    from oracle import restate
    from sedumi_amd import problem
    from test_stage1_mfma import edge_problem
    for P, seed in ((problem.random_sdp(seed=0), 1), (problem.random_sdp(m=35, lp=8, q=(4, 3, 5), s=(), seed=2), 2),
                    (edge_problem(s=(18, 35, 66), seed=3, big=False), 4)):
        d, ud, Q = scaling(P, seed)
        X, xabsd, S, sabsd = ax.ada_exact(P.At, P.K, d, Q, ud)
        A_o, absd_o = restate.getada(P.At, P.K, d, Q, ud)
        assert relerr(A_o, X.astype(np.float64)) < 1e-13 and relerr(absd_o, xabsd.astype(np.float64)) < 1e-13
        assert ax.err(A_o, X, S) < 1e-13 and ax.err(absd_o, xabsd, sabsd) < 1e-13


def test_reference_is_within_tolerance_of_exact_and_restated_hermitian_ada(glue):
    """The compiled reference against the extended-precision helper and against oracle/restate.getada (plain double, the checker that
    travels) on Hermitian problems: hs = (5, 3) and an edge problem."""
    from oracle import restate
    from sedumi_amd import problem
    for P, seed in ((problem.random_sdp(seed=11, m=24, lp=3, q=(3,), s=(4,), hs=(5, 3)), 1),
                    (herm_edge_problem(s=(24,), hs=(33, 70), seed=8), 2)):
        d, ud, Q = scaling(P, seed)
        X, xabsd, S, sabsd = ax.ada_exact(P.At, P.K, d, Q, ud)
        _, _, R, rabsd = reference_ada(glue, P, d, ud, Q)
        A_o, absd_o = restate.getada(P.At, P.K, d, Q, ud)
        assert relerr(R, X.astype(np.float64)) < TOL and relerr(rabsd, xabsd.astype(np.float64)) < TOL
        assert relerr(A_o, R) < TOL and relerr(absd_o, rabsd) < TOL
        assert ax.err(A_o, X, S) < 1e-13 and ax.err(R, X, S) < 1e-13


def test_the_measure_catches_a_negated_plane_and_a_dropped_slot(glue):
    """The proof that these checks can fail: the reference's (correct) ADA' measured against two deliberately WRONG expected values --
    the imaginary plane of one D block negated; one slot of one task that spans several chunks left out -- is beyond the limit the
    library is held to by a factor of more than 1e6, in ADA' and in absd.  No library code is involved."""
    P = herm_edge_problem(s=(24,), hs=(33, 70), seed=8)
    d, ud, Q = scaling(P, 2)
    X, xabsd, S, sabsd = ax.ada_exact(P.At, P.K, d, Q, ud)
    _, _, R, rabsd = reference_ada(glue, P, d, ud, Q)
    limit = 10 * ax.err(R, X, S) + 1e-15
    limit_d = 10 * ax.err(rabsd, xabsd, sabsd) + 1e-15
    k = 2                                                                    # the block of order 70
    Xn, xn, _, _ = ax.ada_exact(P.At, P.K, d, Q, ax.negate_imaginary_plane(P.K, ud, k))
    assert ax.err(R, Xn, S) > 1e6 * limit and ax.err(rabsd, xn, sabsd) > 1e6 * limit_d
    cc = chunk_slots(70, True, 70)
    t = max((t for t in task_shapes(P) if t["k"] == k), key=lambda t: t["nslot"])
    assert t["nslot"] > 2 * cc
    start = int(P.K["sblkstart"].ravel()[k]) - 1
    r = P.At.indices[P.At.indptr[t["j"]]:P.At.indptr[t["j"] + 1]]
    q = np.unique((r[(r >= start) & (r < start + 2 * 70 * 70)] - start) // 70)    # its slots: plane * n + column
    assert q.size == 140 and q[-1] == 139                                    # (the last slot is the imaginary diagonal entry, worth exactly 0)
    for slot in (int(q[cc]), int(q[-2])):                                    # the first slot of the second chunk, a slot of the tail
        Xd, xd, _, _ = ax.ada_exact(P.At, P.K, d, Q, ud, drop=(t["j"], k, slot // 70, slot % 70))
        assert ax.err(R, Xd, S) > 1e6 * limit and ax.err(rabsd, xd, sabsd) > 1e6 * limit_d, slot


# ------------------------------------------------------------------ emulator build (CPU)
@pytest.fixture
def emu():
    from sedumi_amd import capi
    use_emu()
    yield
    capi.use_library(None)


def test_edge_problems_on_the_emulator(emu, glue):
    """Both work-item schedules of the emulator: a missing barrier in the chunk loop shows up in one of them."""
    import ctypes
    from sedumi_amd import capi
    rev = ctypes.CDLL(capi._lib_path)._Z15emu_set_reversei
    try:
        for r in (0, 1):
            rev(r)
            check_edge_problem(glue)
    finally:
        rev(0)


@pytest.mark.parametrize("kind", ["thread", "wave", "ell1", "ell2", "ell4"])
def test_stage2_variants_on_the_emulator(emu, glue, kind):
    """k_psd_stage2 with one pattern entry per work-item (fewer than 48 PSD nonzeros per constraint) and per wavefront (a sparse ADA'
    pattern with the reference's orderings), k_psd_stage2_ell<1> / <2> / <4> (m < 512, < 1024, >= 1024).  Unreachable with a Hermitian
    block: k_psd_direct, k_psd_direct_cols and stage 2 riding in the stage-1 task (all three ask for `A.sdpN == A.rsdpN`), and any
    sweep restricted by d_invperm: every caller of ada_psd passes a null pointer (getada3's Aord.sperm only orders the reference's
    fill; the sum does not depend on it)."""
    check_stage2_variant(glue, kind)


def test_column_panels_on_the_emulator(emu):
    check_column_panels()


def test_mixed_against_real_only_on_the_emulator(emu, glue):
    check_mixed_against_real_only(glue)


def test_determinism_on_the_emulator(emu):
    check_determinism()


# ------------------------------------------------------------------ MI355X
@pytest.mark.gpu
def test_edge_problems_on_the_gpu(glue):
    use_hip()
    check_edge_problem(glue)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["thread", "wave", "ell1", "ell2", "ell4"])
def test_stage2_variants_on_the_gpu(glue, kind):
    use_hip()
    check_stage2_variant(glue, kind)


@pytest.mark.gpu
def test_column_panels_on_the_gpu():
    use_hip()
    check_column_panels()


@pytest.mark.gpu
def test_mixed_against_real_only_on_the_gpu(glue):
    use_hip()
    check_mixed_against_real_only(glue)


@pytest.mark.gpu
def test_determinism_on_the_gpu():
    use_hip()
    check_determinism()
