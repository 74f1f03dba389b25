"""What each cached getada gateway's device plan is keyed on (sedumi_amd/csrc/sdm_mexcache.hip), through the mexFunction shims on the emulated
build of the C ABI (tests/test_mexcache_keys_gpu.py: on libsedumi_hip.so): one input at a time is replaced by a changed copy, and exactly
the plans built from it are rebuilt."""
import numpy as np
import pytest
import scipy.sparse as sp

from helpers import TOL, ref_scaling, relerr
from test_mexshims import mexcache_stats, shimlib, shimmex  # noqa: F401  (the fixtures: the emulated library and the shims built on it)


def _unit_by_reference(host, a):
    """One iteration unit through `host`'s gateways, every array handed to the next gateway BY REFERENCE (call_mx), with every argument
    named in `a` so that a test can change exactly one of them.  Returns numpy copies of (ADA', absd, L.L, L.d)."""
    mx = {k: host.to_mx(v) for k, v in a.items()}
    outs = []
    try:
        outs += host.call_mx("getada1", 1, mx["ADA"], mx["A"], mx["Ajc2"], mx["lqperm"], mx["d"], mx["qblkstart"])[1]
        outs += host.call_mx("getada2", 1, outs[0], mx["DAt"], mx["Aord"], mx["K"])[1]
        outs += host.call_mx("getada3", 2, outs[1], mx["A"], mx["Ajc1"], mx["Aord"], mx["ud"], mx["K"])[1]
        outs += host.call_mx("blkchol", 4, mx["L"], outs[2], mx["pars"], outs[3])[1]
        return tuple(host.from_mx(outs[i]) for i in (2, 3, 4, 5))
    finally:
        host.free(*outs, *mx.values())


def _drop_one_entry(Q):
    """Q without its last stored entry: another pattern (a subset: every product stays inside ADA's)"""
    Q = sp.csc_matrix(Q).copy()
    Q.data[-1] = 0.0
    Q.eliminate_zeros()
    return Q


@pytest.mark.parametrize("level", [0, 2])
def test_each_key_component_rebuilds_exactly_the_slots_keyed_on_it(glue, refmex, shimmex, shimlib, level):
    """The getada gateways keep one device plan each, rebuilt only when what it was built from changes (sdm_mexcache.hip):
    getada1 -- ADA / At patterns, the Lorentz block starts, Ajc2, the values of At;  getada2 -- ADA / DAt.q patterns;
    getada3 -- ADA / At patterns, the PSD blocks, Ajc1, the values of At;  getada (global route) -- ADA / At / DAt.q patterns, the
    block starts, the values of At.  One input at a time is replaced by a changed copy: exactly the plans keyed on it are rebuilt
    (At uploaded again where it is part of the plan), the others reused, a changed lqperm / qperm rebuilds nothing, the factor's plan
    is never rebuilt -- and every unit gives what the reference's gateways give for the same inputs.  Presenting the unchanged
    inputs again rebuilds the same plans once more."""
    import ctypes
    from oracle import glue as gl
    from sedumi_amd import problem
    lib = ctypes.CDLL(shimlib)
    lib.sdm_mexcache_token_base.restype = ctypes.c_double

    def changed_values(A):
        A = sp.csc_matrix(A).copy()
        A.data[A.nnz // 2] *= 1.5
        return A

    def swapped(perm):
        perm = np.array(perm, dtype=np.float64)
        flat = perm.reshape(-1)
        flat[[0, -1]] = flat[[-1, 0]]
        return perm

    def deltas(s0, s1):
        return {k: s1[k] - s0[k] for k in ("ada_build", "ada_reuse", "at_upload", "chol_build")}

    P = problem.random_sdp()
    assert P.m == 30 and P.K["q"].size == 2 and P.K["s"].size == 3
    S = glue.setup(P.At, P.K)
    d, ud = ref_scaling(P, 2)
    DAt = glue.getDAtm(S, d)
    Ajc = sp.csc_matrix(S["A"]).indptr
    split = np.asarray(S["Ablkjc"])[:, 2].astype(np.float64)
    base = {"ADA": S["ADA"], "A": S["A"], "Ajc2": split, "Ajc1": split, "lqperm": S["Aord"]["lqperm"], "Aord": S["Aord"],
            "d": {"l": np.asarray(d["l"]).reshape(-1, 1), "det": np.asarray(d["det"]).reshape(-1, 1)}, "qblkstart": P.K["qblkstart"],
            "K": P.K, "DAt": DAt, "ud": ud.reshape(-1, 1), "L": S["L"], "pars": gl.default_pars_chol()}
    j2 = int(np.flatnonzero(split > Ajc[:-1])[0])                 # a column with an LP / Lorentz nonzero: getada1 is told to leave its last one out
    j1 = int(np.flatnonzero(split < Ajc[1:])[0])                  # a column with a PSD nonzero: getada3 is told to leave its first one out
    Ajc2, Ajc1 = split.copy(), split.copy()
    Ajc2[j2] -= 1; Ajc1[j1] += 1
    K2 = problem.make_K(int(P.K["l"]), P.K["q"].ravel()[::-1], P.K["s"].ravel())      # the Lorentz cones' orders the other way round
    assert not np.array_equal(K2["qblkstart"], P.K["qblkstart"]) and np.array_equal(K2["sblkstart"], P.K["sblkstart"])
    Aord2 = dict(S["Aord"]); Aord2["qperm"] = swapped(S["Aord"]["qperm"])
    # (changed inputs, plans rebuilt: ada_build; of those the ones that hold At: at_upload)
    cases = [({}, 0, 0),
             ({"Ajc2": Ajc2}, 1, 1),
             ({"Ajc1": Ajc1}, 1, 1),
             ({"A": changed_values(S["A"])}, 2, 2),
             ({"K": K2, "qblkstart": K2["qblkstart"]}, 1, 1),
             ({"DAt": dict(DAt, q=_drop_one_entry(DAt["q"]))}, 1, 0),
             ({"lqperm": swapped(S["Aord"]["lqperm"]), "Aord": Aord2}, 0, 0)]
    try:
        lib.sdm_mexcache_clear()
        lib.sdm_mexcache_set_lazy(level)
        _unit_by_reference(shimmex, base)                           # fills the cache
        for change, nbuild, nat in cases:
            for a in (dict(base, **change), base):                  # the changed copy, then the unchanged inputs again
                ref = _unit_by_reference(refmex, a)
                s0 = mexcache_stats(shimlib)
                A3, absd, LL, Ld = _unit_by_reference(shimmex, a)
                assert deltas(s0, mexcache_stats(shimlib)) == {"ada_build": nbuild, "ada_reuse": 3 - nbuild, "at_upload": nat, "chol_build": 0}, sorted(change)
                if level == 0:
                    assert relerr(A3, ref[0]) < TOL, sorted(change)
                else:
                    assert sp.csc_matrix(A3).nnz == 1 and sp.csc_matrix(A3)[0, 0] > lib.sdm_mexcache_token_base()
                assert relerr(absd, ref[1]) < TOL and relerr(LL, ref[2]) < TOL and relerr(Ld, ref[3]) < TOL, sorted(change)
        # the global route (getada.mex, problems without PSD blocks): one plan, keyed on all of it
        P0 = problem.random_sdp(m=30, lp=7, q=(4, 5, 3), s=(), seed=33)
        S0 = glue.setup(P0.At, P0.K)
        d0, ud0 = ref_scaling(P0, 6)
        DAt0 = glue.getDAtm(S0, d0)
        split0 = np.asarray(S0["Ablkjc"])[:, 2].astype(np.float64)
        K02 = problem.make_K(int(P0.K["l"]), P0.K["q"].ravel()[::-1], ())
        assert not np.array_equal(K02["qblkstart"], P0.K["qblkstart"])
        base0 = {"A": S0["A"], "K": P0.K, "DAt": DAt0}
        ds0 = {"l": np.asarray(d0["l"]).reshape(-1, 1), "det": np.asarray(d0["det"]).reshape(-1, 1)}
        first = True
        for change in ({}, {"A": changed_values(S0["A"])}, {"K": K02}, {"DAt": dict(DAt0, q=_drop_one_entry(DAt0["q"]))}):
            for a in (dict(base0, **change), base0):
                r1 = refmex.call("getada1", 1, S0["ADA"], a["A"], split0, S0["Aord"]["lqperm"], ds0, a["K"]["qblkstart"])
                r3, _ = refmex.call("getada3", 2, refmex.call("getada2", 1, r1, a["DAt"], S0["Aord"], a["K"]), a["A"], split0, S0["Aord"], ud0.reshape(-1, 1), a["K"])
                s0 = mexcache_stats(shimlib)
                shimmex.set_global("ADA_sedumi_", S0["ADA"])
                absd = shimmex.call("getada", 1, a["A"], a["K"], ds0, a["DAt"])
                nbuild = 1 if change or first else 0
                assert deltas(s0, mexcache_stats(shimlib)) == {"ada_build": nbuild, "ada_reuse": 1 - nbuild, "at_upload": nbuild, "chol_build": 0}, sorted(change)
                assert relerr(shimmex.get_global("ADA_sedumi_"), r3) < TOL and relerr(absd.ravel(), r3.diagonal()) < TOL, sorted(change)   # (absd = diag(ADA'), getada.m:40)
                first = False
    finally:
        shimmex.set_global("ADA_sedumi_", None)
        lib.sdm_mexcache_set_lazy(0)
        lib.sdm_mexcache_clear()
