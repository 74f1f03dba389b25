"""sdm_plan_wrappcg / Plan.wrappcg: wrapPcg.m with loopPcg.m as ONE call on the resident plan, against the host loop of
sedumi_amd.driver.loop (Sedumi.wrapPcg / Sedumi.loopPcg), which is the yardstick.

Tolerance (measured, not chosen): per call, s = relative difference between the host loop (1) and the same host loop with every
inner product taken in extended precision (2) -- both are the reference algorithm and differ only in rounding -- floored at the
median s of the problem's calls.  The device call (3) must take the same k, refinement trials and STOP as (1) and lie within
10 s of (1) in y, dx and r: the device also reorders the sums inside the Lorentz scaling and PopK at every CG step, which (2)
leaves in numpy's order.  A wrong term, sign or branch shows at the size of restol (5e-3 relative) or as another k.  Calls on
which (1) and (2) disagree on k or STOP are left out: at most 10 % of a problem's calls.

Measured (profiles/r11a_wrappcg_parity.txt): largest ratio 1.0 on the calls of nb, quantum (emulator), arch0 and control07 (MI355X),
at most 2.0 on the synthetic edge cases.  (Before the device took its inner products in double-double, nb reached 3.1e6 and
control07 1.1e7: where the host loop and its exact variant agree to the last bit, a one-ulp change of alpha from reordered sums is
O(1) of r, and late CG loops of control07 amplify it to 1e-3 in y.)"""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import helpers

RATIO = 10.0
MAX_LEFT_OUT = 0.10


# ---------------------------------------------------------------- extended-precision inner products for version (2)
def _two_prod(a, b):
    """a*b = p + e exactly (Dekker / Veltkamp)"""
    p = a * b
    s = 134217729.0
    ah = a * s; ah = ah - (ah - a); al = a - ah
    bh = b * s; bh = bh - (bh - b); bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def _xdot(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    p, e = _two_prod(a, b)
    return math.fsum(np.concatenate((p, e)))


def _xsum(v):
    return math.fsum(np.asarray(v, dtype=np.float64).ravel())


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def three_versions(S, L, d, DAt, rb, rv, cg, y0):
    """(1) the host loop, (2) the same with exact inner products, (3) plan.wrappcg -- on the same plan state"""
    from sedumi_amd.driver import loop as lp
    one = lp.Sedumi.wrapPcg(S, L, d, DAt, rb, rv, cg, y0)
    i1 = dict(S.pcg_info)
    S._dot, S._sum = _xdot, _xsum
    try:
        two = lp.Sedumi.wrapPcg(S, L, d, DAt, rb, rv, cg, y0)
        i2 = dict(S.pcg_info)
    finally:
        del S._dot, S._sum
    pl = S.hot.plan
    if S.cone.nq:
        pl.upload("qauxdet", d["auxdet"]); pl.upload("qauxtr", d["auxtr"])
    y, dx, k, r, info = pl.wrappcg(rv, rb, y0, cg, bool(np.size(d["perm"])))
    return {"one": one, "i1": i1, "two": two, "i2": i2, "three": (y, dx, k, r), "i3": info}


def judge(recs, name):
    """the rule of the module docstring over the recorded calls of one problem; prints the figures before asserting"""
    kept = [c for c in recs if c["one"][2] == c["two"][2] and c["i1"]["stop"] == c["i2"]["stop"]]
    left = len(recs) - len(kept)
    s = {o: [_rel(c["two"][i], c["one"][i]) for c in kept] for i, o in enumerate("y dx".split() + [None, "r"]) if o}
    med = {o: float(np.median(v)) if v else 0.0 for o, v in s.items()}
    worst, fails = 0.0, []
    for j, c in enumerate(kept):
        one, three = c["one"], c["three"]
        same = one[2] == three[2] and c["i1"]["stop"] == c["i3"]["stop"] and c["i1"]["trials"] == c["i3"]["trials"]
        if not same:
            fails.append((j, "branch", one[2], three[2], c["i1"], c["i3"]))
            continue
        for i, o in ((0, "y"), (1, "dx"), (3, "r")):
            bound = max(s[o][j], med[o])
            d = _rel(three[i], one[i])
            ratio = d / bound if bound > 0 else (0.0 if d == 0 else math.inf)
            worst = max(worst, ratio)
            if ratio > RATIO:
                fails.append((j, o, d, bound))
    deep = [c for c in recs if c["one"][2] >= 3]
    refined = [c for c in recs if c["i1"]["trials"] > 0]
    print(f"wrappcg parity {name}: calls {len(recs)} left out {left} median s y {med['y']:.3e} dx {med['dx']:.3e} r {med['r']:.3e} "
          f"largest ratio {worst:.3f} (k >= 3: {len(deep)}, refinement trials: {len(refined)})", flush=True)
    assert recs
    assert left <= MAX_LEFT_OUT * len(recs), (left, len(recs))
    if deep:
        assert any(c["one"][2] >= 3 for c in kept)
    if refined:
        assert any(c["i1"]["trials"] > 0 for c in kept)
    assert not fails, fails[:5]
    return worst


def whole_solve_parity(name):
    import test_driver as td
    from sedumi_amd.driver import loop as lp
    recs = []

    class Tri(lp.Sedumi):
        def wrapPcg(self, L, d, DAt, rb, rv, cgpars, y0):
            c = three_versions(self, L, d, DAt, rb, rv, cgpars, y0)
            recs.append(c)
            return c["one"]

    At, K, g = td.problem(name)
    Tri(At, g["b"], g["c"], K, hot=lp.PlanHot(), internal=True).solve()
    return judge(recs, name)


# ---------------------------------------------------------------- synthetic problems
KW = dict(m=24, lp=4, q=(3, 5), s=(6, 4), hs=(3,), dens=0.4)


def synthetic(seed=1, perm=True, kw=KW, P=None, graded=0.0, u_off=None, detune=("l",)):
    """a Sedumi on problem.random_sdp (LP, Lorentz, real and Hermitian PSD blocks) with a factored resident plan for a scaling
    whose d.u comes from test_invcholfac.scaling_factor_case (lower triangle mirrored, as the scaling update stores it).
    Hooks of test_wrappcg_shapes.py (the defaults leave every number of this function as it was without them):
    kw / P: other arguments of random_sdp, or a problem built by the caller -- any cone mix, also K.l = 0, no Lorentz cone, no PSD block;
    graded = g > 0: d.l, d.det and the diagonal of d.u are 10^(g (2 rand - 1)), spread over 2 g decades, not 0.5 + rand;
    u_off = c: the strict upper triangle of a d.u block of order n times c / sqrt(n) (a wide random triangle is otherwise singular to rounding);
    detune: which of "l", "det", "u" move away from the factor's scaling afterwards (the Lorentz fields and DAt.q follow d.det)"""
    from sedumi_amd import problem
    from sedumi_amd.driver import loop as lp
    from test_invcholfac import scaling_factor_case
    if P is None:
        P = problem.random_sdp(seed=seed, **kw)
    rng = np.random.default_rng(seed)
    N, m = P.At.shape
    S = lp.Sedumi(P.At, rng.standard_normal(m), rng.standard_normal(N), P.K, internal=True)
    cn = S.cone
    d = {}

    def spread(n):
        return 10.0 ** (graded * (2.0 * rng.random(n) - 1.0)) if graded else 0.5 + rng.random(n)

    def lorentz(det):                                                   # det(d.q) = d.det, and what updtransfo.m derives from it
        d["det"] = det
        d["q1"] = np.sqrt(det + cn.ddot(d["q2"], np.concatenate((np.zeros(cn.i2), d["q2"], np.zeros(N - cn.i3)))))
        d["auxdet"] = np.sqrt(2 * det)
        d["auxtr"] = np.sqrt(2) * (d["q1"] + d["auxdet"])

    d["l"] = spread(cn.l)
    det = spread(cn.nq)
    d["q2"] = 0.3 * rng.standard_normal(cn.i3 - cn.i2)
    lorentz(det)
    if cn.lenud:
        u, pm = scaling_factor_case(P.K, seed=seed + 3, garbage_lower=False)
    else:
        u, pm = np.zeros(0), np.zeros(0)
    mats = [M + np.triu(M, 1).conj().T for M, _ in cn._blocks(np.concatenate((np.zeros(cn.lq), u)))]
    if u_off is not None or graded:
        for k, M in enumerate(mats):
            n = M.shape[0]
            dg = spread(n) if graded else np.real(np.diag(M)).copy()
            if u_off is not None:
                M *= u_off / math.sqrt(n)
            M[np.arange(n), np.arange(n)] = dg
    d["u"] = cn._pack(mats)
    d["perm"] = pm if perm else np.zeros(0)
    DAt = S.G.getDAtm(S.S, d)
    L = S.hot.factor(S.S, d, DAt, dict(S.S["L"]), S.pars["chol"])
    # the operator's LP scaling moved away from the factor's: the factor becomes a preconditioner that leaves the CG loop real work
    # (with the exact factor every loop would end at the rounding level of the solves, where branches are decided by the last bits)
    pl = S.hot.plan
    if "l" in detune:
        d["l"] = d["l"] * (1.0 + rng.random(cn.l))
        pl.upload("dl", d["l"])
    if "det" in detune and cn.nq:
        lorentz(d["det"] * (1.0 + rng.random(cn.nq)))
        DAt = S.G.getDAtm(S.S, d)
        pl.upload("ddet", d["det"]); pl.upload("q1", d["q1"]); pl.getdatq()
    if "u" in detune and cn.lenud:
        d["u"] = cn._pack([M * (1.0 + 0.5 * rng.random()) for M, _ in cn._blocks(np.concatenate((np.zeros(cn.lq), d["u"])))])
        pl.upload("u", d["u"])
    return S, L, d, DAt, rng


CG = {"qprec": 1, "restol": 5e-3, "stagtol": 5e-14, "maxiter": 49, "refine": 1}
EDGE = [("zero", {}), ("maxiter1", {"maxiter": 1, "restol": 1e-10}), ("refine0", {"refine": 0, "restol": 1e-10}),
        ("refine1", {"refine": 1, "restol": 1e-10}), ("qprec0", {"qprec": 0, "restol": 1e-10}), ("qprec1", {"qprec": 1, "restol": 1e-10}),
        ("no_rb", {"restol": 1e-10}), ("no_perm", {"restol": 1e-10})]


def edge_case(name, over):
    S, L, d, DAt, rng = synthetic(seed=2, perm=name != "no_perm")
    N, m = S.A.shape
    cg = dict(CG, **over)
    recs = []
    for trial in range(6):
        rv = np.zeros(N) if name == "zero" else rng.standard_normal(N)
        rb = None if name == "no_rb" else (np.zeros(m) if name == "zero" else 0.1 * rng.standard_normal(m))
        recs.append(three_versions(S, L, d, DAt, rb, rv, cg, 1.0))
    if name == "zero":
        for c in recs:
            y, dx, k, r = c["three"]
            assert k == 0 and not np.any(y) and np.array_equal(dx, np.zeros(N)) and c["i3"]["exit"] == 0
    if name == "maxiter1":
        assert any(c["i1"]["stop"] == 2 for c in recs)
    judge(recs, "synthetic " + name)
    S.hot.plan.close()


def determinism():
    S, L, d, DAt, rng = synthetic(seed=3)
    N, m = S.A.shape
    rv, rb = rng.standard_normal(N), rng.standard_normal(m)
    pl = S.hot.plan
    pl.upload("qauxdet", d["auxdet"]); pl.upload("qauxtr", d["auxtr"])
    cg = dict(CG, restol=1e-10)
    a = pl.wrappcg(rv, rb, 1.0, cg, True)
    b = pl.wrappcg(rv, rb, 1.0, cg, True)
    assert a[2] >= 2 and a[2] == b[2] and a[4] == b[4]
    for i in (0, 1, 3):
        assert a[i].tobytes() == b[i].tobytes()
    pl.close()


# ---------------------------------------------------------------- CPU: the fiber emulator
@pytest.mark.parametrize("name", ["nb", "quantum"])
def test_wrappcg_matches_the_host_loop_on_every_call_of_a_solve_emulated(name):
    helpers.use_emu()
    whole_solve_parity(name)


@pytest.mark.parametrize("case", [c[0] for c in EDGE])
def test_wrappcg_edge_cases_emulated(case):
    helpers.use_emu()
    edge_case(case, dict(EDGE)[case])


def test_wrappcg_repeats_its_bits_emulated():
    helpers.use_emu()
    determinism()


def test_wrappcg_refusals_launch_nothing():
    """dense columns, no factor, missing "u": SdmError before any launch (per-kernel timing records none)"""
    from sedumi_amd import problem
    from sedumi_amd.capi import SdmError
    from sedumi_amd.plan import Plan
    helpers.use_emu()
    P = problem.random_sdp(seed=4, **KW)
    N, m = P.At.shape
    plan = Plan(0)
    plan.set_chol(problem.dense_symbolic(m), problem.dense_pattern(m))
    plan.set_ada(P.At, P.Ablkjc, P.K, problem.lorentz_pattern(P))
    plan.pcg_init()
    rv = np.ones(N)

    def refused(match):
        plan.kprof(True)                                                # (clears the records)
        with pytest.raises(SdmError, match=match):
            plan.wrappcg(rv, None, 1.0, CG)
        assert plan.kprof_summary() == {}

    refused("no factor")
    LL = sp.csc_matrix(problem.dense_symbolic(m)["L"]).astype(np.float64)
    LL.data[:] = 0.0
    LL.setdiag(1.0)
    plan.load_factor(LL, np.ones(m))
    refused('"u"')
    plan.pcg_init([2.0, 5.0], sp.csc_matrix(P.At)[[1, 4], :].T)
    refused("dense columns")
    plan.close()


def test_quadadd_kernel_is_not_contracted(tmp_path):
    """the gfx950 code of the kernel that applies quadadd holds no fused multiply-add: fl(alpha*p) is rounded before it is added"""
    import re
    from sedumi_amd import build
    from test_abi import _disassemble_gfx950
    dis = _disassemble_gfx950(build.build(), tmp_path)
    parts = re.findall(r"^[0-9a-f]+ <([^>]*k_wp_step_quadadd[^>]*)>:\n(.*?)(?=^[0-9a-f]+ <[^>]*>:|\Z)", dis, flags=re.S | re.M)
    assert parts
    for sym, body in parts:
        assert "v_mul_f64" in body and not re.search(r"\bv_fmac?_f64", body), sym


def test_product_driver_with_device_pcg_solves_the_examples_emulated():
    import test_driver as td
    from oracle import refmex
    from sedumi_amd.driver import loop as lp
    from test_native_driver import _check_against_reference_run
    if not refmex.available():
        pytest.skip("oracle/_ref is not built")
    helpers.use_emu()
    for name in ("nb", "quantum"):
        At, K, g = td.problem(name)
        hot = lp.PlanHot(device_pcg=True)
        S = lp.Sedumi(At, g["b"], g["c"], K, hot=hot, internal=True)
        r = S.solve()
        assert hasattr(hot, "last_pcg_info")                            # the device call ran
        _check_against_reference_run(name, r, margin=0)


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["arch0", "control07"])
def test_wrappcg_matches_the_host_loop_on_every_call_of_a_solve_gpu(name):
    helpers.use_hip()
    whole_solve_parity(name)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c[0] for c in EDGE])
def test_wrappcg_edge_cases_gpu(case):
    helpers.use_hip()
    edge_case(case, dict(EDGE)[case])


@pytest.mark.gpu
def test_wrappcg_repeats_its_bits_gpu():
    helpers.use_hip()
    determinism()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["nb", "quantum", "arch0", "control07"])
def test_product_driver_with_device_pcg_solves_the_examples_gpu(name):
    """margins of the default path's test (test_native_driver.py): 0 for nb and quantum, 1 for arch0 and control07"""
    import test_driver as td
    from sedumi_amd.driver import loop as lp
    from test_native_driver import _check_against_reference_run
    helpers.use_hip()
    At, K, g = td.problem(name)
    hot = lp.PlanHot(device_pcg=True)
    r = lp.Sedumi(At, g["b"], g["c"], K, hot=hot, internal=True).solve()
    assert hasattr(hot, "last_pcg_info")
    _check_against_reference_run(name, r, margin=1 if name in ("arch0", "control07") else 0)
