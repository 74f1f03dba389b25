"""sdm_plan_wrappcg at the cone and vector shapes its kernels stride over (sdm_wrappcg.hip), against the host loop of
sedumi_amd.driver.loop with test_wrappcg.py's rule, unchanged: the device call takes the host loop's k, refinement trials and STOP
and lies within RATIO x the host loop's own rounding spread (host loop (1) against the same loop with exact inner products (2)).

The shapes (SHAPES) follow the constants parsed from the source: WP_T work-items and at most WP_G workgroups per partial
reduction, LQ = the work-items of a Lorentz / LP workgroup, TILE = the edge of a psdscale tile.
  - Lorentz cones whose norm-bound length is 1, LQ - 1, LQ, LQ + 1, 2 LQ, 2 LQ + 1 and about 500 beside cones of order 3: the
    second and the partial last trip of the per-cone loops, full butterflies, the double-double x'y share of a long cone;
  - these behind K.l = 0 (no LP workgroup), LQ - 1, LQ, LQ + 1 and 2 LQ + 2 LP entries (nlpb = 0, 1, 1, 2, 3);
  - real PSD blocks of order TILE, TILE + 1, 2 TILE + 2, Hermitian ones of order TILE + 1 and 2 TILE + 2, an order-3 block beside
    a wide one, with and without d.perm; PSD only (neither LP nor Lorentz: k_wp_dx_lq / k_wp_popk_lq are not launched);
  - Lorentz only, LP only;
  - m = 1, 2, WP_T, WP_T + 1, 2 WP_T, 2 WP_T + 1 (grids of 1, 1, 1, 2, 2, 3 workgroups);
  - d.l, d.det and diag(d.u) graded over six decades, dx judged per segment too (LP part, every cone, every PSD block relative to
    its own largest entry, bound measured as for the whole vector on that segment);
  - one skipped pivot (a duplicated constraint: L.d = 0 there).  The host loop accepts that factor: PlanHot.factor sets the skipped
    pivot's d to 1 (deninfac.m:87-94), which is what k_wp_divd_dot does with d = 0.
  - the long reduction (GPU only): m = WP_T WP_G + 300 = 16 684, LP row i on constraints i and i + 1 inside blocks of 32 (ADA' block-diagonal) and
    three Lorentz cones on a few constraints: the grid is capped at WP_G and k_wp_divd_dot, k_wp_step_quadadd, k_wp_amax and k_wp_dot
    take a second trip over an m-vector.  (Not on the emulator: its factor of 16 000 supernodes takes two minutes there
    and one host-loop call, with two sweeps over them per CG step, more than four.)

What the PSD shapes do NOT check: k_psdscale itself.  The host loop takes Amul, vecsym and psdscale from the same resident plan
as the device call (Sedumi._ops: the d of the last factor), so a wrong k_psdscale is wrong in (1), (2) and (3) alike -- which is why
these shapes give ratio 1.000.  They check what wrappcg does around psdscale: the offsets into the cone vectors, the perm flag, the
N-length reductions and PopK's sum of squares over wide blocks.  The check of k_psdscale that does not go through the kernel is
test_pcg_ops.py (psdscale.m restated), whose cases run on both backends.

Conditions checked before the device result is looked at: (1) and (2) disagree on k / STOP in at most MAX_LEFT_OUT of a shape's
calls, and every shape keeps a call with k >= 2 (the CG step kernels ran, not only the first-step return).  restol is 1e-7 -- at 1e-10, the
edge cases' value, the recomputed residual of these larger problems sits at its rounding level and (1) and (2) part -- and d.l, d.det and d.u all move away from the factor's scaling after the factorisation.

presence(): every shape is what the table says (from K and Plan.kprof_summary()).  The self-check runs the host loop with three
deliberately wrong operators and has judge() refuse each.  Measured ratios: profiles/r14a_wrappcg_shapes.txt."""
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import helpers
from test_wrappcg import CG, MAX_LEFT_OUT, RATIO, _rel, judge, synthetic, three_versions


def _constants():
    src = open(os.path.join(helpers.ROOT, "sedumi_amd", "csrc", "sdm_wrappcg.hip")).read()
    t = int(re.search(r"constexpr int WP_T = (\d+);", src).group(1))
    g = int(re.search(r"constexpr int WP_G = (\d+);", src).group(1))
    lq = {int(v) for v in re.findall(r"__launch_bounds__\((\d+)\) k_wp_(?:dx|popk)_lq", src)}
    assert len(lq) == 1
    lq = lq.pop()
    assert f"nlpb = (l + {lq - 1}) / {lq}" in src and set(re.findall(r"i < b1; i \+= (\d+)\)", src)) == {str(lq)}
    pcg = open(os.path.join(helpers.ROOT, "sedumi_amd", "csrc", "sdm_pcg.hip")).read()
    tile = int(re.search(r"const int nt = \(bn\[k\] \+ (\d+)\) / (\d+);", pcg).group(2))
    return t, g, lq, tile


WP_T, WP_G, LQ, TILE = _constants()
CGS = dict(CG, restol=1e-7)
ALL = ("l", "det", "u")


# ---------------------------------------------------------------- problems
def cone_problem(m, l, q=(), s=(), hs=(), seed=0, dens=0.3, dens_lp=None, dup=None):
    """At (N x m, internal form) with K.l = l LP rows (no row is special), Lorentz cones q, real PSD blocks s, Hermitian ones hs: every
    constraint takes each LP row with probability dens_lp and each other cone row (PSD: folded lower triangle) with probability dens,
    plus one LP or cone row of its own.  dup = (i, j): constraint j is a copy of constraint i."""
    from sedumi_amd import problem
    rng = np.random.default_rng(seed)
    K = problem.make_K(l, q, s, hs)
    N, nq = int(K["N"]), len(q)
    start, ns = problem._psd_rows(K)
    rows, wts = [np.arange(l, int(K["lq"]))], [np.ones(int(K["lq"]) - l)]
    for k, n in enumerate(ns):
        r, c = np.tril_indices(n)
        rows.append(start[k] + r + c * n); wts.append(np.where(r == c, 1.0, 2.0))
        if k >= len(s):
            r, c = np.tril_indices(n, -1)
            rows.append(start[k] + n * n + r + c * n); wts.append(np.full(r.size, 2.0))
    rows, wts = np.concatenate(rows).astype(np.int64), np.concatenate(wts)
    parts = []
    if l:
        M = sp.random(l, m, density=min(1.0, dens if dens_lp is None else dens_lp), random_state=rng, format="coo", data_rvs=rng.standard_normal)
        parts.append((M.row, M.col, M.data))
    if rows.size:
        M = sp.random(rows.size, m, density=min(1.0, dens), random_state=rng, format="coo", data_rvs=rng.standard_normal)
        parts.append((rows[M.row], M.col, M.data * wts[M.row]))
    own = np.arange(m) % l if l else rows[np.arange(m) % rows.size]
    parts.append((own, np.arange(m), 2.0 + rng.random(m)))
    At = sp.csc_matrix((np.concatenate([p[2] for p in parts]), (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))), shape=(N, m))
    if dup is not None:
        At = sp.lil_matrix(At); At[:, dup[1]] = At[:, dup[0]]; At = sp.csc_matrix(At)
    return problem.Problem(At, K, f"cone_problem(m={m},l={l},q={tuple(q)},s={tuple(s)},hs={tuple(hs)})")


def long_problem(seed=0):
    """m just above WP_T * WP_G: LP row i touches constraints i and i + 1 inside blocks of 32 constraints (ADA' block-diagonal with
    tridiagonal blocks: an elimination tree of depth 32, not of depth m), three Lorentz cones on a few constraints of the first blocks"""
    from sedumi_amd import problem
    rng = np.random.default_rng(seed)
    m = WP_T * WP_G + 300
    q = (3, LQ + 6, 4)
    K = problem.make_K(m, q, (), ())
    N = int(K["N"])
    qb = K["qblkstart"].ravel().astype(int) - 1
    nb = np.arange(m - 1)[(np.arange(1, m) % 32) != 0]                  # rows i that also touch constraint i + 1
    r, c, v = [np.arange(m), nb], [np.arange(m), nb + 1], [2.0 + rng.random(m), 0.5 * rng.standard_normal(nb.size)]
    for k in range(len(q)):                                             # cone k on constraints 100 k .. 100 k + 7: its trace and half its norm-bound rows
        for j in range(100 * k, 100 * k + 8):
            rr = np.concatenate(([m + k], np.arange(qb[k], qb[k + 1])))
            keep = rng.random(rr.size) < 0.5
            keep[0] = True
            r.append(rr[keep]); c.append(np.full(keep.sum(), j)); v.append(rng.standard_normal(keep.sum()))
    return problem.Problem(sp.csc_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(c))), shape=(N, m)), K, f"long_problem(m={m})")


Q3 = (3, 3)
SHAPES = {
    # name: (arguments of cone_problem, arguments of synthetic, what presence() expects)
    "lorentz_l0": (dict(m=24, l=0, q=(2, LQ, 3, LQ + 1, LQ + 2, 3, 2 * LQ + 1, 2 * LQ + 2, 501), dens=0.2), {}, dict(nlpb=0, qmax=500)),
    **{f"lorentz_l{l}": (dict(m=24, l=l, q=(LQ + 2, 3, 2 * LQ + 2, 2, 501, 3, LQ, LQ + 1), dens=0.2), {}, dict(nlpb=(l + LQ - 1) // LQ, qmax=500))
       for l in (LQ - 1, LQ, LQ + 1, 2 * LQ + 2)},
    **{f"psd_real{n}_{'perm' if p else 'noperm'}": (dict(m=24, l=3, q=Q3, s=(n, 3), dens=0.1), dict(perm=p), dict(nlpb=1, smax=n))
       for n in (TILE, TILE + 1, 2 * TILE + 2) for p in (True, False)},
    **{f"psd_herm{n}_{'perm' if p else 'noperm'}": (dict(m=24, l=3, q=Q3, s=(4,), hs=(3, n), dens=0.1), dict(perm=p), dict(nlpb=1, hmax=n))
       for n in (TILE + 1, 2 * TILE + 2) for p in (True, False)},
    "psd_only": (dict(m=24, l=0, s=(TILE + 1, 3), hs=(TILE + 2,), dens=0.1), {}, dict(nlpb=0, smax=TILE + 1, hmax=TILE + 2, no_lq=True)),
    "lorentz_only": (dict(m=24, l=0, q=(LQ + 3, 3, 2 * LQ + 5), dens=0.3), {}, dict(nlpb=0, qmax=2 * LQ + 4, no_psd=True)),
    "lp_only": (dict(m=24, l=2 * LQ + 2, dens=0.2), {}, dict(nlpb=3, no_psd=True)),
    **{f"m{m}": (dict(m=m, l=2 * m + 8, q=(3, 5), s=(6, 4), hs=(3,), dens=0.3, dens_lp=min(1.0, 6.0 / (2 * m + 8))), {}, dict(m=m, grid=g, **({"restol": 1e-17} if m == 1 else {})))
       for m, g in ((1, 1), (2, 1), (WP_T, 1), (WP_T + 1, 2), (2 * WP_T, 2), (2 * WP_T + 1, 3))},
    "graded": (dict(m=24, l=LQ + 1, q=(3, LQ + 2, 3, 501, 2), s=(TILE + 1, 3), hs=(4,), dens=0.15), dict(graded=3.0), dict(nlpb=2, qmax=500, smax=TILE + 1)),
    "skipped_pivot": (dict(m=24, l=30, q=(3, 5), s=(6, 4), hs=(3,), dens=0.3, dup=(3, 17)), {}, dict(nlpb=1, nskip=1, no_rb=True)),
}
BITS = ["lorentz_l0", f"psd_herm{2 * TILE + 2}_perm", f"m{2 * WP_T + 1}"]


def build(name, seed=5):
    pk, sk, want = SHAPES[name]
    P = cone_problem(seed=seed, **pk)
    S, L, d, DAt, rng = synthetic(seed=seed, P=P, u_off=0.5, detune=ALL, **sk)
    return S, L, d, DAt, rng, want


def segments(K):
    """index sets of dx: the LP part, every Lorentz cone (its trace entry and norm-bound rows), every PSD block"""
    l, nq = int(K["l"]), K["q"].size
    qb = K["qblkstart"].ravel().astype(int) - 1
    sb = K["sblkstart"].ravel().astype(int) - 1
    seg = [("lp", np.arange(l))] if l else []
    seg += [(f"q{k}", np.concatenate(([l + k], np.arange(qb[k], qb[k + 1])))) for k in range(nq)]
    seg += [(f"s{k}", np.arange(sb[k], sb[k + 1])) for k in range(K["s"].size)]
    return seg


def judge_segments(recs, K, name):
    """judge()'s rule for dx on every segment by itself: relative to the segment's own largest entry, the bound = spread of (1) against
    (2) on that segment, floored at the segment's median over the calls"""
    kept = [c for c in recs if c["one"][2] == c["two"][2] and c["i1"]["stop"] == c["i2"]["stop"]]
    worst, fails = 0.0, []
    for sname, ix in segments(K):
        s = [_rel(c["two"][1][ix], c["one"][1][ix]) for c in kept]
        med = float(np.median(s))
        for j, c in enumerate(kept):
            bound, dlt = max(s[j], med), _rel(c["three"][1][ix], c["one"][1][ix])
            ratio = dlt / bound if bound > 0 else (0.0 if dlt == 0 else math.inf)
            worst = max(worst, ratio)
            if ratio > RATIO:
                fails.append((sname, j, dlt, bound))
    print(f"wrappcg parity {name}: dx per segment, largest ratio {worst:.3f}", flush=True)
    assert not fails, fails[:5]
    return worst


def conditions(recs, name):
    """what the yardstick itself must give at a shape, from (1) and (2) alone"""
    left = sum(1 for c in recs if c["one"][2] != c["two"][2] or c["i1"]["stop"] != c["i2"]["stop"])
    ks = [c["one"][2] for c in recs]
    print(f"wrappcg shape {name}: k of the host loop {ks}, left out {left}", flush=True)
    assert left <= MAX_LEFT_OUT * len(recs), (name, left)
    assert max(ks) >= 2, (name, ks)


def presence(S, L, want, prof):
    K, cn = S.K, S.cone
    N, m = S.A.shape
    ran = lambda k: prof.get(k, (0, 0.0))[0] > 0
    if "qmax" in want:
        assert int(K["q"].max()) - 1 == want["qmax"] > LQ
    if "nlpb" in want:
        assert (cn.l + LQ - 1) // LQ == want["nlpb"]
    if "smax" in want:
        assert int(cn.s[:cn.nreal].max()) == want["smax"] >= TILE
    if "hmax" in want:
        assert int(cn.s[cn.nreal:].max()) == want["hmax"] > TILE
    if "m" in want:
        assert m == want["m"] and max(1, min(WP_G, (m + WP_T - 1) // WP_T)) == want["grid"]
    if "nskip" in want:
        assert L["nskip"] == want["nskip"] and np.count_nonzero(S.hot.plan.download("d") == 0.0) == want["nskip"]
    lq_ran = ran("k_wp_dx_lq") and ran("k_wp_popk_lq")
    psd_ran = ran("k_psdscale<1>") and ran("k_psdscale<2>")
    assert lq_ran == (cn.l + cn.nq > 0) and not (want.get("no_lq") and (ran("k_wp_dx_lq") or ran("k_wp_popk_lq")))
    assert psd_ran == (cn.lenud > 0) and not (want.get("no_psd") and psd_ran)
    for k in ("k_wp_dot", "k_wp_divd_dot", "k_wp_step_quadadd", "k_wp_amax", "k_wp_finish"):
        assert ran(k), (k, sorted(prof))


def six_calls(S, L, d, DAt, rng, want={}, n=6):
    """m = 1: the first step is the exact solution (one preconditioned CG step on a 1 x 1 system), so k >= 2 needs a restol below the
    rounding of that step -- the loop then runs on the rounding residual, and (1) and (2) still agree on every branch.
    Skipped pivot: no rb.  ADA' is singular there, and an rb outside the range of A leaves a residual that no step removes: every loop
    then ends by stagnation on its last bits and (1) and (2) disagree on k in six calls of six; with r = A D dx the system is consistent."""
    N, m = S.A.shape
    cg = dict(CGS, restol=want["restol"]) if "restol" in want else CGS
    return [three_versions(S, L, d, DAt, None if want.get("no_rb") else 0.1 * rng.standard_normal(m), rng.standard_normal(N), cg, 1.0) for _ in range(n)]


def profiled_call(S, d, rng, want={}):
    N, m = S.A.shape
    pl = S.hot.plan
    pl.kprof(True)
    cg = dict(CGS, restol=want["restol"]) if "restol" in want else CGS
    out = pl.wrappcg(rng.standard_normal(N), None if want.get("no_rb") else 0.1 * rng.standard_normal(m), 1.0, cg, bool(np.size(d["perm"])))
    prof = pl.kprof_summary()
    pl.kprof(False)
    assert out[2] >= 2
    return prof


def shape_case(name):
    S, L, d, DAt, rng, want = build(name)
    recs = six_calls(S, L, d, DAt, rng, want)
    conditions(recs, name)
    presence(S, L, want, profiled_call(S, d, rng, want))
    worst = judge(recs, "shape " + name)
    if name == "graded":
        worst = max(worst, judge_segments(recs, S.K, "shape " + name))
    S.hot.plan.close()
    return worst


def long_case():
    S, L, d, DAt, rng = synthetic(seed=7, P=long_problem(7), detune=ALL)
    N, m = S.A.shape
    recs = six_calls(S, L, d, DAt, rng)
    conditions(recs, "long")
    assert m > WP_T * WP_G and min(WP_G, (m + WP_T - 1) // WP_T) == WP_G
    presence(S, L, dict(nlpb=(m + LQ - 1) // LQ, qmax=LQ + 5, no_psd=True), profiled_call(S, d, rng))
    worst = judge(recs, "shape long")
    S.hot.plan.close()
    return worst


def repeats(name):
    """determinism()'s check at a shape of the table"""
    S, L, d, DAt, rng, want = build(name, seed=6)
    N, m = S.A.shape
    rv, rb = rng.standard_normal(N), rng.standard_normal(m)
    pl = S.hot.plan
    if S.cone.nq:
        pl.upload("qauxdet", d["auxdet"]); pl.upload("qauxtr", d["auxtr"])
    use = bool(np.size(d["perm"]))
    a = pl.wrappcg(rv, rb, 1.0, CGS, use)
    b = pl.wrappcg(rv, rb, 1.0, CGS, use)
    assert a[2] >= 2 and a[2] == b[2] and a[4] == b[4]
    for i in (0, 1, 3):
        assert a[i].tobytes() == b[i].tobytes()
    pl.close()


# ---------------------------------------------------------------- the rule has teeth at these shapes
def _wrong_run(S, L, d, DAt, rb, rv, wrong):
    """the host loop with one operator of the cone layer replaced; the cone object is restored afterwards"""
    from sedumi_amd.driver import loop as lp
    cn = S.cone
    l, nq, qb = cn.l, cn.nq, S.K["qblkstart"].ravel().astype(int) - 1
    ddot0, psd0 = cn.ddot, S.psdscale

    def ddot_truncated(x2, y):                                          # only the first LQ norm-bound rows of each cone
        keep = np.concatenate([np.arange(qb[k], min(qb[k] + LQ, qb[k + 1])) for k in range(nq)])
        yy = np.zeros_like(y); yy[keep] = y[keep]
        return ddot0(x2, yy)

    def ddot_shifted(x2, y):                                            # cone k gets cone k + 1's sum, when l > LQ
        v = ddot0(x2, y)
        return np.roll(v, -1) if l > LQ else v

    def psd_conj(dd, x, transp=False):                                  # the imaginary plane of the last Hermitian block negated
        out = np.array(psd0(dd, x, transp))
        n = int(cn.s[-1])
        out[out.size - n * n:] *= -1.0
        return out

    if wrong.startswith("last_"):
        return _wrong_last(S, L, d, DAt, rb, rv, wrong)
    if wrong == "truncated":
        cn.ddot = ddot_truncated
    elif wrong == "shifted":
        cn.ddot = ddot_shifted
    else:
        S.psdscale = psd_conj
    try:
        out = lp.Sedumi.wrapPcg(S, L, d, DAt, rb, rv, CGS, 1.0)
        return out, dict(S.pcg_info)
    finally:
        if wrong == "conj":
            del S.psdscale
        else:
            del cn.ddot


def _wrong_last(S, L, d, DAt, rb, rv, wrong):
    """a wrong operator that keeps every branch: only the D A' y of the LAST loopPcg of the call (loopPcg.m:159-165, what wrapPcg
    subtracts from dx) is wrong -- last_drop: the last norm-bound row of the longest cone is not written; last_conj: the imaginary
    plane of the last Hermitian block has the other sign.  k, trials and STOP stay; dx and the final r carry the error."""
    from sedumi_amd.driver import loop as lp
    cn = S.cone
    lp.Sedumi.wrapPcg(S, L, d, DAt, rb, rv, CGS, 1.0)
    last, seen = S.pcg_info["trials"], [0]
    qb = S.K["qblkstart"].ravel().astype(int) - 1

    def loop(*a):
        dy, dk, xx = lp.Sedumi.loopPcg(S, *a)
        if seen[0] == last and xx is not None:
            xx = np.array(xx)
            if wrong == "last_drop":
                xx[qb[int(np.argmax(cn.q)) + 1] - 1] = 0.0
            else:
                xx[xx.size - int(cn.s[-1]) ** 2:] *= -1.0
        seen[0] += 1
        return dy, dk, xx

    S.loopPcg = loop
    try:
        out = lp.Sedumi.wrapPcg(S, L, d, DAt, rb, rv, CGS, 1.0)
        return out, dict(S.pcg_info)
    finally:
        del S.loopPcg


def excess(recs, name):
    """by how many times the judged differences exceed their bounds (inf: another k, trials or STOP)"""
    kept = [c for c in recs if c["one"][2] == c["two"][2] and c["i1"]["stop"] == c["i2"]["stop"]]
    worst = 0.0
    for i in (0, 1, 3):
        s = [_rel(c["two"][i], c["one"][i]) for c in kept]
        med = float(np.median(s))
        for j, c in enumerate(kept):
            same = c["one"][2] == c["three"][2] and c["i1"] == {k: c["i3"][k] for k in c["i1"]}
            bound = max(s[j], med)
            worst = max(worst, (_rel(c["three"][i], c["one"][i]) / bound if bound > 0 else math.inf) if same else math.inf)
    print(f"wrappcg self-check {name}: limit exceeded {worst / RATIO:.3g} times", flush=True)
    return worst / RATIO


# (wrong operator, shape, whether it must be caught by the RATIO bound itself: the first four change k or STOP)
TEETH = [("truncated", "lorentz_l0", False), ("shifted", f"lorentz_l{LQ + 1}", False), ("shifted", f"lorentz_l{2 * LQ + 2}", False),
         ("conj", f"psd_herm{TILE + 1}_perm", False), ("last_drop", "lorentz_l0", True), ("last_conj", f"psd_herm{TILE + 1}_perm", True)]


def teeth_case(wrong, name, by_ratio):
    S, L, d, DAt, rng, want = build(name)
    N, m = S.A.shape
    recs = []
    for _ in range(6):
        rb, rv = 0.1 * rng.standard_normal(m), rng.standard_normal(N)
        c = three_versions(S, L, d, DAt, rb, rv, CGS, 1.0)
        good = (c["three"], c["i3"])
        c["three"], c["i3"] = _wrong_run(S, L, d, DAt, rb, rv, wrong)
        c["good"] = good
        recs.append(c)
    conditions(recs, name)
    with pytest.raises(AssertionError):
        judge(recs, f"self-check {wrong} on {name}")
    times = excess(recs, f"{wrong} on {name}")
    assert times > 1.0 and (math.isfinite(times) or not by_ratio)
    if by_ratio:
        assert all(c["one"][2] == c["three"][2] and c["i1"] == {k: c["i3"][k] for k in c["i1"]} for c in recs)
    for c in recs:                                                      # (the same calls with the device's own result pass)
        c["three"], c["i3"] = c["good"]
    judge(recs, f"self-check device on {name}")
    S.hot.plan.close()


# ---------------------------------------------------------------- CPU: the fiber emulator
def test_the_shapes_follow_the_source():
    assert min(WP_T, WP_G, LQ, TILE) > 3                                # (the table above is built from them: a change there moves the edges)
    assert sorted(set(int(q) - 1 for q in SHAPES["lorentz_l0"][0]["q"])) == [1, 2, LQ - 1, LQ, LQ + 1, 2 * LQ, 2 * LQ + 1, 500]


# over about a minute in the emulator (its matrix-core tiles and dense factors are slow): the wide PSD blocks and m >= WP_T
SLOW = [n for n in SHAPES if re.match(r"psd_(herm|only|real%d)|m\d\d\d" % (2 * TILE + 2), n)]


def _marked(names):
    return [pytest.param(n, marks=pytest.mark.slow) if n in SLOW else n for n in names]


@pytest.mark.parametrize("name", _marked(SHAPES))
def test_wrappcg_shapes_emulated(name):
    helpers.use_emu()
    shape_case(name)


@pytest.mark.parametrize("name", _marked(BITS))
def test_wrappcg_shapes_repeat_their_bits_emulated(name):
    helpers.use_emu()
    repeats(name)


@pytest.mark.parametrize("wrong,name,by_ratio", [pytest.param(*t, marks=pytest.mark.slow) if t[1] in SLOW else t for t in TEETH])
def test_the_rule_refuses_a_wrong_operator_emulated(wrong, name, by_ratio):
    helpers.use_emu()
    teeth_case(wrong, name, by_ratio)


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_wrappcg_shapes_gpu(name):
    helpers.use_hip()
    shape_case(name)


@pytest.mark.gpu
def test_wrappcg_long_reduction_gpu():
    helpers.use_hip()
    long_case()


@pytest.mark.gpu
@pytest.mark.parametrize("name", BITS)
def test_wrappcg_shapes_repeat_their_bits_gpu(name):
    helpers.use_hip()
    repeats(name)
