"""Stage 1 of ADA' on the matrix cores (k_psd_stage1_mfma, sedumi_amd/csrc/sdm_ada.hip) at the shapes its paths divide on: chunks of
S1_KC = 32 slots, four slots per MFMA step, blocks padded to np = 32 / 48 / 80 / 96, the nonzeros of a task staged in LDS or not,
single-nonzero tasks beside dense ones in one launch.

  * getada3 against the compiled reference at the suite's tolerance (GPU), on inputs for which the reference itself is inside that
    tolerance of the numpy restatement (checked here, on the CPU side of the same test);
  * the same problems through the emulator build of the same source against the numpy restatement (CPU);
  * the footprint of the kernel from its code-object metadata: three workgroups per compute unit at control07's block order (CPU)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import ROOT, TOL, relerr, use_emu, use_hip

S1_KC, S1_MAXN, S1_NZ = 32, 96, 1536        # sedumi_amd/csrc/sdm_plan.h (checked below): they shape the test problems
EDGES = (1, 4, 5, S1_KC - 1, S1_KC, S1_KC + 1, 47, 48, 49, 2 * S1_KC, 2 * S1_KC + 1)


def _slots(rng, n, nslot, per):
    """Lower-triangle positions in `nslot` distinct columns of a block of order n, up to `per` rows in each."""
    pos = []
    for c in sorted(rng.choice(n, size=nslot, replace=False)):
        rows = c + rng.choice(n - c, size=min(per, n - c), replace=False)
        pos += [(int(r), int(c)) for r in sorted(rows)]
    return pos


def _one_slot(rng, n, nnz):
    c = int(rng.integers(0, n - nnz + 1))
    return [(int(r), c) for r in sorted(c + rng.choice(n - c, size=nnz, replace=False))]


def edge_problem(s=(70, 24, 96, 35), seed=0, big=True):
    """Constraints whose tasks sit at every edge of the kernel: in the blocks of order 70 (np = 80) and 96 (np = 96) nslot = 1, 4, 5, the
    chunk edges 31 .. 33, 47 .. 49, 64, 65 and n; in the block of order 24 one-slot tasks of 1 .. 5 nonzeros and nslot = 4, 5, 23, 24; in the
    block of order 35 a single nonzero per constraint, as control07 has; and (big) one task of 2000 nonzeros, more than the kernel ever
    stages in LDS."""
    from sedumi_amd import problem
    rng = np.random.default_rng(seed)
    lp = 3
    K = problem.make_K(lp + 1, [], list(s))
    start = K["sblkstart"].ravel().astype(np.int64) - 1
    per_block = []
    for k, n in enumerate(s):
        if n > 64:
            specs = [_slots(rng, n, ns, 3) for ns in EDGES + (n - 1, n) if ns <= n]
            if big and n == max(s):
                tri = [(r, c) for c in range(n) for r in range(c, n)]
                specs.append([tri[i] for i in sorted(rng.choice(len(tri), size=2000, replace=False))])
        elif n <= 32:
            specs = [_one_slot(rng, n, z) for z in (1, 2, 3, 4, 5, 1, 1)] + [_slots(rng, n, ns, 2) for ns in (4, 5, n - 1, n)]
        else:
            tri = [(r, c) for c in range(n) for r in range(c, n)]
            specs = [[tri[i]] for i in rng.choice(len(tri), size=16, replace=False)]
        per_block.append(specs)
    m = max(len(x) for x in per_block)
    rows, cols, vals = [], [], []
    for j in range(m):
        for r in range(1, lp + 1):
            rows.append(r); cols.append(j); vals.append(rng.standard_normal())
        for k, n in enumerate(s):
            for (r, c) in per_block[k][(j + 3 * k) % len(per_block[k])]:
                rows.append(start[k] + r + c * n); cols.append(j); vals.append(rng.standard_normal() * (1.0 if r == c else 2.0))
    At = sp.csc_matrix((vals, (rows, cols)), shape=(int(K["N"]), m))
    return problem.Problem(At, K, f"edge_problem(s={s})")


def _task_shapes(P):
    """(block, n, nslot, nnz) of every stage-1 task of P, as ada_build cuts them."""
    start = P.K["sblkstart"].ravel().astype(np.int64) - 1
    ns = P.K["s"].ravel().astype(np.int64)
    out = []
    for j in range(P.m):
        r = P.At.indices[P.At.indptr[j]:P.At.indptr[j + 1]]
        for k, n in enumerate(ns):
            q = r[(r >= start[k]) & (r < start[k] + n * n)] - start[k]
            if q.size:
                out.append((k, int(n), int(np.unique(q // n).size), int(q.size)))
    return out


def test_edge_problem_has_the_shapes_it_is_for():
    P = edge_problem()
    T = _task_shapes(P)
    for n in (70, 96):
        assert {ns for (_, nn, ns, _) in T if nn == n} >= set(EDGES) | {n}
    assert {z for (_, nn, ns, z) in T if nn == 24 and ns == 1} == {1, 2, 3, 4, 5}
    assert any(z > S1_NZ for (_, _, _, z) in T)                                  # never staged
    assert sum(1 for (_, nn, ns, z) in T if ns == 1 and z == 1) >= P.m           # single nonzeros beside the dense tasks of the same launch
    assert max(nn for (_, nn, _, _) in T) <= S1_MAXN


def _ada_via_plan(P, d, ud):
    """ADA' and absd of the resident plan (dense pattern)."""
    from sedumi_amd import problem
    from sedumi_amd.plan import Plan
    plan = Plan(0)
    plan.set_chol(problem.dense_symbolic(P.m), problem.dense_pattern(P.m))
    plan.set_ada(P.At, P.Ablkjc, P.K, sp.csc_matrix((0, P.m)))
    plan.upload("dl", d["l"]); plan.upload("ddet", d["det"]); plan.upload("udsqr", ud)
    plan.getada(); plan.sync()
    ada, absd = plan.download("ada"), plan.download("absd")
    plan.close()
    return ada, absd


def test_edge_problems_on_the_emulator():
    """The emulator build of the same source on the problems of the GPU tests -- chunk edges, np = 32 .. 96, a task that is never
    staged -- against the numpy restatement of getada1 -> getada2 -> getada3."""
    from oracle import restate
    from sedumi_amd import capi, problem
    use_emu()
    try:
        for P, seed in ((edge_problem(), 2), (edge_problem(s=(18, 35, 66), seed=3, big=False), 4)):
            d, ud = problem.spd_scaling(P.K, seed=seed)
            ada, absd = _ada_via_plan(P, d, ud)
            A_o, absd_o = restate.getada(P.At, P.K, d, sp.csc_matrix((0, P.m)), ud)
            assert relerr(ada.reshape(P.m, P.m), A_o) < TOL and relerr(absd, absd_o) < TOL
    finally:
        capi.use_library(None)


@pytest.mark.gpu
@pytest.mark.parametrize("s,seed", [((70, 24, 96, 35), 0), ((70, 35), 1), ((80, 32, 65), 2), ((96,), 3), ((16, 66), 4)])
def test_getada3_at_the_edges_against_the_reference(glue, s, seed):
    from oracle import glue as gl, restate
    from sedumi_amd import mex, problem
    use_hip()
    P = edge_problem(s=s, seed=seed)
    S = glue.setup(P.At, P.K)
    assert np.array_equal(S["Ablkjc"], P.Ablkjc)
    d, ud = problem.spd_scaling(P.K, seed=seed + 20)
    ref = glue.ref
    DAt = glue.getDAtm(S, d)
    ADA1 = ref.call("getada1", 1, S["ADA"], S["A"], S["Ablkjc"][:, 2], S["Aord"]["lqperm"], {"l": gl._col(d["l"]), "det": gl._col(d["det"])},
                    P.K["qblkstart"])
    ADA2 = ref.call("getada2", 1, ADA1, DAt, S["Aord"], P.K)
    ADA3, absd3 = ref.call("getada3", 2, ADA2, S["A"], S["Ablkjc"][:, 2], S["Aord"], gl._col(ud), P.K)
    # the reference itself is inside the tolerance on these inputs (against the numpy restatement of the three calls)
    A_o, absd_o = restate.getada(P.At, P.K, d, sp.csc_matrix((0, P.m)), ud)
    assert relerr(ADA3, A_o) < TOL and relerr(absd3.ravel(), absd_o) < TOL
    A3, absd = mex.getada3(ADA2, S["A"], S["Ablkjc"][:, 2], S["Aord"], ud, P.K)
    assert relerr(A3, ADA3) < TOL and relerr(absd, absd3) < TOL, (relerr(A3, ADA3), relerr(absd, absd3))


def _plan_constants(tmp_path):
    """S1_WAVES and the dynamic LDS of a launch at maxn = 70 with a largest task of 631 nonzeros, from sedumi_amd/csrc/sdm_plan.h itself (the
    constexpr helpers ada_psd launches with), compiled as the emulator build compiles the header."""
    import subprocess
    src = tmp_path / "s1.cpp"
    src.write_text('#include "sdm_plan.h"\n#include <cstdio>\nint main() { std::printf("%d %zu %d %d %d\\n", sdm::S1_WAVES, sdm::s1_mfma_lds(70, 631), '
                   'sdm::S1_KC, sdm::S1_NZ, sdm::S1_MAXN); }\n')
    exe = tmp_path / "s1"
    subprocess.check_call(["g++", "-std=c++17", "-DSDM_EMU", "-I", os.path.join(ROOT, "tests", "hipemu"), "-I", os.path.join(ROOT, "sedumi_amd", "csrc"),
                           "-o", str(exe), str(src)])
    return [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]


def test_constants_of_this_file_are_those_of_the_plan_header(tmp_path):
    assert _plan_constants(tmp_path)[2:] == [S1_KC, S1_NZ, S1_MAXN]


def test_three_tasks_fit_a_compute_unit_at_order_70(tmp_path):
    """From the code object of k_psd_stage1_mfma and the dynamic LDS ada_psd asks for at maxn = 70 with control07's largest task (631
    nonzeros; sdm::s1_mfma_lds of sdm_plan.h, which ada_psd launches with): three workgroups fit a compute unit's 163 840 bytes of LDS
    and its register file (512 vector registers per SIMD lane, allotted in blocks of 8; a workgroup's wavefronts are dealt over the four
    SIMDs).  A condition of the hardware, not a measurement."""
    import importlib.util
    from sedumi_amd import build
    spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "tools", "code_objects.py"))
    co = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(co)
    if not os.path.exists(co.READELF):
        pytest.skip("llvm-readelf not found")
    ks = {k: v for k, v in co.kernels(build.build()).items() if "k_psd_stage1_mfma" in k}
    assert len(ks) == 1, list(ks)
    (v,) = ks.values()
    waves, dyn = _plan_constants(tmp_path)[:2]
    lds = v["group_segment_fixed_size"] + dyn
    assert 3 * lds <= 163840, (v["group_segment_fixed_size"], dyn)
    regs = -(-(v["vgpr_count"] + v["agpr_count"]) // 8) * 8
    assert 3 * -(-waves // 4) * regs <= 512, v
    assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, v
