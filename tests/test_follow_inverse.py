"""The inverse BEHIND a one-launch front (sdm_follow.h: sinv_follow_body / follow_trisolve): the follower workgroups of k_ldl_front
solve L(r, r) X(r, c) = -sum against the 16-column groups of the diagonal block AS THE FACTOR PUBLISHES THEM, and the sweeps apply X.

Per case: factor once, then fwsolve and bwsolve with three different right-hand sides in turn (a stale work vector cannot pass as a result).
Each sweep is compared with a forward / backward substitution in numpy.longdouble on the DOWNLOADED factor; the yardstick is the
compiled reference (fwblkslv / bwblkslv, oracle/_ref) on the same factor and right-hand sides:

    |y_lib - y_exact| <= BOUND * |y_ref - y_exact| + FLOOR * eps * |y_exact|            (2-norms)

BOUND guards against a wrong or unfinished tile (off by many orders of magnitude), not against rounding.  It is twice the largest ratio
|y_lib - y_exact| / |y_ref - y_exact| of the PARENT build (explicit 64x64 inverses, product with X(r, r)) over these same cases and
sweeps on the emulator, and at least 1.  Measured parent ratios, largest of the six sweeps per case:

    case             parent   substitution by groups (this follower)
    dense-112        1.479    1.646
    dense-128        1.261    1.272
    dense-129        1.892    1.970
    dense-154        1.274    1.470
    dense-330        1.374    1.473
    dense-666        1.153    1.227
    skip_last-154    1.336    1.755
    probe_last-330   1.063    1.163

so BOUND = 2 * 1.892.  (The forward sweeps sit at 0.3 - 0.5 of the reference's error on the dense cases, the backward sweeps at 1.0 - 1.9.)

The one-launch path and the launch-per-panel path must agree in L, d (array_equal) and in y (1e-12), as helpers.check_one_launch_front asks.
Emulator: every case phase by phase; m = 154 and both rank-deficient cases also with one process per workgroup (the polls are live there),
work-items and workgroups in reversed order too.  GPU: every case, and 20 repeats of m = 154 and m = 666 with array_equal y."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import helpers
from helpers import relerr

EPS = float(np.finfo(np.float64).eps)
BOUND = 2 * 1.892    # = 2 * max(1, largest parent ratio): see the table above
FLOOR = 4.0          # "a few eps |y|"

# (kind, m): dense SPD fronts as helpers.check_one_launch_front draws them, and two rank-deficient ones of the kind of
# tests/test_gpu_parity.py (X = B B' of rank < m + a diagonal of 1e-13 .. 1e-3)
#   112: the smallest one-launch front, last block 48 rows     128: two full blocks     129: a last block of ONE row
#   154: 2 * 64 + 26 = control07's last-block shape at three tile rows     330, 666 (control07: 11 tile rows)
#   skip_last 154: skipped pivots in the LAST block     probe_last 330: the last block takes the column probe's (general) path -- its
#   groups arrive all at once, from the epilogue of the block's LDL'
CASES = [("dense", 112), ("dense", 128), ("dense", 129), ("dense", 154), ("dense", 330), ("dense", 666), ("skip_last", 154), ("probe_last", 330)]
IDS = ["%s-%d" % c for c in CASES]


def make_case(kind, m):
    """(X, pars, [three right-hand sides])"""
    from oracle import glue as gl
    pars = dict(gl.default_pars_chol())
    if kind == "dense":
        rng = np.random.default_rng(m)
        B = rng.standard_normal((m, m))
        X = B @ B.T + m * np.eye(m)
    else:
        # skip_last: rank 140 of 154 under a diagonal of at most 1e-12 -- the pivots 140 .. 153 (all in the last block) are a hundred times below
        # their threshold canceltol * X_kk and skipped.  probe_last: rank 324 of 330, maxu = 2 -- pivots of the last block are added to
        rank, seed, maxu, lo, hi = {"skip_last": (140, 3, 5e5, -15, -12), "probe_last": (324, 15, 2.0, -13, -3)}[kind]
        rng = np.random.default_rng(seed)
        B = rng.standard_normal((m, rank))
        X = B @ B.T + np.diag(10.0 ** rng.uniform(lo, hi, m))
        pars["maxu"] = maxu
    X = sp.csc_matrix((X.ravel(order="F"), np.tile(np.arange(m), m), np.arange(0, m * m + 1, m)), shape=(m, m))
    rhss = [rng.standard_normal(m), np.cos(0.37 * np.arange(m)) + 2.0, rng.standard_normal(m) * 10.0 ** rng.uniform(-3, 3, m)]
    return X, pars, rhss


def factor_and_sweep(kind, m, one_launch=True):
    """dict: lpr, d, pivots, fw[3], bw[3], y (ldlsolve of the first right-hand side), kernels"""
    from sedumi_amd import problem
    from sedumi_amd.plan import Plan
    X, pars, rhss = make_case(kind, m)
    plan = Plan(0)
    plan.set_one_launch_fronts(one_launch)
    plan.set_chol(problem.dense_symbolic(m), X)
    plan.upload("ada", X.data)
    plan.kprof(True)
    plan.blkchol(pars, False)
    out = {"lpr": plan.download("lpr"), "d": plan.download("d"), "pivots": plan.pivots(), "fw": [], "bw": []}
    for r in rhss:
        plan.upload("rhs", r); plan.fwsolve(); out["fw"].append(plan.download("y"))
        plan.upload("rhs", r); plan.bwsolve(); out["bw"].append(plan.download("y"))
    plan.upload("rhs", rhss[0]); plan.ldlsolve(); out["y"] = plan.download("y")
    out["kernels"] = set(plan.kprof_summary().keys())
    plan.kprof(False)
    # (the factor in the symbolic pattern, zeros stored: the reference's supernodal sweeps index a skipped pivot's column like any other)
    out["Lcsc"] = sp.csc_matrix((out["lpr"], plan.L_pattern.indices.copy(), plan.L_pattern.indptr.copy()), shape=(m, m))
    out["L"] = out["Lcsc"].toarray()
    plan.close()
    return out


@functools.lru_cache(maxsize=None)
def cached_run(backend, kind, m, one_launch=True):
    """(one factorisation per backend and case, shared by the tests below and left unchanged)"""
    (helpers.use_emu if backend == "emu" else helpers.use_hip)()
    return factor_and_sweep(kind, m, one_launch)


def exact_sweeps(L, rhss):
    """forward and backward substitution with the unit lower triangular L in numpy.longdouble, all right-hand sides at once"""
    m = L.shape[0]
    Ll = np.tril(L, -1).astype(np.longdouble)
    fw = np.array(rhss, dtype=np.longdouble).T.copy()
    for j in range(m - 1):
        fw[j + 1:] -= np.outer(Ll[j + 1:, j], fw[j])
    bw = np.array(rhss, dtype=np.longdouble).T.copy()
    for j in range(m - 1, 0, -1):
        bw[:j] -= np.outer(Ll[j, :j], bw[j])
    return fw, bw


def sweep_ratios(refmex, out, kind, m):
    """[(what, |lib - exact|, |ref - exact|, |exact|)] of the six sweeps of a case"""
    from sedumi_amd import problem
    _, _, rhss = make_case(kind, m)
    L = out["L"]
    Lref = dict(problem.dense_symbolic(m)); Lref["L"] = out["Lcsc"]
    fw, bw = exact_sweeps(L, rhss)
    res = []
    for i, r in enumerate(rhss):
        for what, got, want in (("fw", out["fw"][i], fw[:, i]), ("bw", out["bw"][i], bw[:, i])):
            ref = np.asarray(refmex.call(what + "blkslv", 1, Lref, r.reshape(-1, 1))).ravel()
            res.append(("%s%d" % (what, i), float(np.linalg.norm(got.astype(np.longdouble) - want)),
                        float(np.linalg.norm(ref.astype(np.longdouble) - want)), float(np.linalg.norm(want))))
    return res


def check_accuracy(refmex, out, kind, m):
    for what, elib, eref, ynorm in sweep_ratios(refmex, out, kind, m):
        print("%s-%d %s: |lib - exact| %.3e  |ref - exact| %.3e  ratio %.3f  |y| %.3e" % (kind, m, what, elib, eref, elib / max(eref, 1e-300), ynorm))
        assert np.isfinite(elib) and elib <= BOUND * eref + FLOOR * EPS * ynorm, (kind, m, what, elib, eref, ynorm)


def check_case_shape(out, kind, m):
    """the case is what its name says"""
    (si, _), (ai, _) = out["pivots"]
    last = 64 * ((m - 1) // 64)
    if kind == "dense":
        assert si.size == 0 and ai.size == 0
    elif kind == "skip_last":
        assert np.any(si >= last), si
    else:
        assert np.any(ai >= last), (si, ai)      # a pivot of the last block was ADDED to: the column probe ran, the block took the general path


def check_paths_agree(backend, kind, m):
    a, b = cached_run(backend, kind, m, True), cached_run(backend, kind, m, False)
    assert "k_ldl_front" in a["kernels"] and "k_ldl_panel" not in a["kernels"] and "k_ldl_front" not in b["kernels"]
    assert ("k_sinv_follow" in a["kernels"]) == (backend == "emu") and "k_sinv_follow" not in b["kernels"]
    assert not ({"k_sprep", "k_sinv128"} & a["kernels"])          # the inverse was built behind the factor, by the follower
    assert np.array_equal(a["lpr"], b["lpr"]) and np.array_equal(a["d"], b["d"])
    assert all(np.array_equal(x, y) for p, q in zip(a["pivots"], b["pivots"]) for x, y in zip(p, q))
    assert relerr(a["y"], b["y"]) < 1e-12


# ------------------------------------------------------------------ emulator, phase by phase
@pytest.mark.parametrize("kind,m", CASES, ids=IDS)
def test_follower_sweeps_against_extended_precision_emu(refmex, kind, m):
    out = cached_run("emu", kind, m)
    check_case_shape(out, kind, m)
    check_accuracy(refmex, out, kind, m)


@pytest.mark.parametrize("kind,m", CASES, ids=IDS)
def test_follower_and_panel_path_agree_emu(kind, m):
    check_paths_agree("emu", kind, m)


# ------------------------------------------------------------------ emulator, one process per workgroup: the polls are live
@pytest.fixture()
def concurrent_emu():
    helpers.use_emu()
    from hipemu import build_emu
    lib = ctypes.CDLL(build_emu.build())
    yield lib                                    # (the test switches the mode on: its phased reference run comes first)
    lib._Z18emu_set_concurrenti(0)
    lib._Z15emu_set_reversei(0)
    lib._Z22emu_set_reverse_blocksi(0)


@pytest.mark.parametrize("reverse,last_first", [(0, 0), (1, 0), (0, 1)])
@pytest.mark.parametrize("kind,m", [("dense", 154), ("skip_last", 154), ("probe_last", 330)])
def test_follower_as_concurrent_workgroups(refmex, concurrent_emu, kind, m, reverse, last_first):
    """reverse: the work-items of every workgroup scheduled in descending order; last_first: the processes forked from the last workgroup
    down (the followers are up before the workgroups they wait for).  The bits of the phased run."""
    want = cached_run("emu", kind, m)
    concurrent_emu._Z18emu_set_concurrenti(1)
    concurrent_emu._Z15emu_set_reversei(reverse)
    concurrent_emu._Z22emu_set_reverse_blocksi(last_first)
    out = factor_and_sweep(kind, m)
    concurrent_emu._Z18emu_set_concurrenti(0)
    assert "k_sinv_follow" in out["kernels"]
    assert np.array_equal(out["lpr"], want["lpr"]) and np.array_equal(out["d"], want["d"])
    for k in ("fw", "bw"):
        assert all(np.array_equal(a, b) for a, b in zip(out[k], want[k])), k
    assert np.array_equal(out["y"], want["y"])
    check_accuracy(refmex, out, kind, m)


# ------------------------------------------------------------------ the device
@pytest.mark.gpu
@pytest.mark.parametrize("kind,m", CASES, ids=IDS)
def test_follower_sweeps_against_extended_precision_gpu(refmex, kind, m):
    out = cached_run("hip", kind, m)
    check_case_shape(out, kind, m)
    check_accuracy(refmex, out, kind, m)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,m", CASES, ids=IDS)
def test_follower_and_panel_path_agree_gpu(kind, m):
    check_paths_agree("hip", kind, m)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [154, 666])
def test_follower_is_deterministic_across_repeats_gpu(m):
    """A tile read before it was complete shows as a difference between repeats."""
    from sedumi_amd import problem
    from sedumi_amd.plan import Plan
    helpers.use_hip()
    X, pars, rhss = make_case("dense", m)
    plan = Plan(0)
    plan.set_chol(problem.dense_symbolic(m), X)
    plan.upload("rhs", rhss[0])
    ref = None
    for rep in range(20):
        plan.upload("ada", X.data); plan.blkchol(pars, False); plan.ldlsolve()
        y = plan.download("y")
        if ref is None:
            ref = y
            assert np.all(np.isfinite(y)) and relerr(X @ y, rhss[0]) < 1e-10
        assert np.array_equal(y, ref), rep
    plan.close()
