#!/usr/bin/env python
"""bench.py -- IPM iterations per second of the normal-equations hot path on MI355X.

One "step" = one IPM iteration unit (sedumi.m:450-473) on frozen, HBM-resident inputs:
    1 x (getada1 + getada2 + getada3)  ->  1 x blkchol  ->  4 x (fwblkslv, ./L.d, bwblkslv)   (single RHS each)
Workload at N=1: BASELINE.json configs[1], examples/control07.mat itself -- the hot-path inputs of the reference's
example (At after pretransfo, K, the scaling of the "rand" golden tag, rhs) travel as tests/golden/control07.npz
(generated from /root/reference by tests/golden/make_golden.py).  `--workload control07_like` is the synthetic
problem of the same shape; `nb`, `maxcut<n>`, `blockdiag` are the shapes of configs[2..4].  `--other-configs` (N=1)
also measures those other configs briefly in the same process and reports them under "other_configs".

N>1 (launched with torch.distributed.run, one rank per GPU): ONE unit per step, sharded the way the workload shards
(SURVEY.md 8e): single-supernode workloads form ADA' as column panels per rank + one RCCL all-gather (factor and
solves replicated -- they do not shard); the block-diagonal workload deals its independent subtrees to the ranks
(all-gather of the solution only).  `--shard replicas` runs independent units per rank instead (weak scaling).

Prints ONE compact JSON line (rank 0, < 4 KB, strict JSON: `compact_line`) with the fields the driver expects.  A plain run
sets up, warms up, times `--steps` units and prints the line; its `roofline` and `cpu_baseline` are null.  `--full` adds
everything else: `roofline` and `cpu_baseline` (the unmodified reference MEX, naive BLAS-1, one host core) and a handful of
scalar extras in the line, and -- per-kernel times, the phases, `pcie_inclusive`, `mex_inclusive` (the unit through the built
mexFunction shims: what an unmodified sedumi.m pays), `whole_solve_weighted`, with `--other-configs` also `cpu_baseline_blas`
(the reference linked to the host's OpenBLAS) and the other configs -- in `profiles/bench_detail_<tag>.json`, whose path the
line names.  `--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy (`dump_outputs`).

`python bench.py --gpus N` without a launcher (no WORLD_SIZE in the environment) re-executes itself under
`python -m torch.distributed.run --nproc-per-node N` on 127.0.0.1 and passes rank 0's line through.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PARS = {"canceltol": 1e-12, "maxu": 5e5, "abstol": 1e-20}          # checkpars.m:144-168
HBM_PEAK_GBS = 8000.0                                               # MI355X_MICROARCH.md: HBM3E 8 TB/s
FP64_MATRIX_PEAK_TFS = 78.6                                         # v_mfma_f64_16x16x4_f64: = the FP64 vector rate on CDNA4
NSOLVE = 4
CONFIG_NOTE = {"contro": "examples/control07.mat (BASELINE.json configs[1])", "nb": "examples/nb.mat (BASELINE.json configs[2]; no PSD blocks: the getada.m route)",
               "arch0": "examples/arch0.mat (BASELINE.json configs[0])", "nb_lik": "nb-shaped SOCP (BASELINE.json configs[2] shape)",
               "maxcut": "MAXCUT SDP, one dense PSD block (BASELINE.json configs[3])"}

LINE_LIMIT = 4096                                                   # the driver parses ONE line; keep it far below any capture limit
ROOF_KEYS = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us", "launches_per_step", "algorithmic_work_per_launch")
BASE_KEYS = ("value", "unit", "cores", "kind", "sample")
TOP_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")


def _tidy(x, maxlen=240):
    """Numbers to 6 significant digits, non-finite numbers to null (strict JSON), strings cut to maxlen."""
    if isinstance(x, (bool, type(None), int)):
        return x
    if isinstance(x, (float, np.floating, np.integer)):
        x = float(x)
        if x != x or x in (float("inf"), float("-inf")):
            return None
        return int(x) if x == int(x) and abs(x) < 1e15 else float("%.6g" % x)
    if isinstance(x, str):
        return x if len(x) <= maxlen else x[:maxlen - 3] + "..."
    if isinstance(x, dict):
        return {str(k): _tidy(v, maxlen) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_tidy(v, maxlen) for v in x]
    return _tidy(str(x), maxlen)


def compact_line(full, extras=None, detail=None):
    """THE line of the driver's contract from the full result dictionary: the contract's top-level fields, `config`
    {workload, parallelism}, `roofline` (ROOF_KEYS), `cpu_baseline` (BASE_KEYS), at most five scalar extras and the path
    of the detail file.  Strict JSON (no NaN / Infinity), shorter than LINE_LIMIT bytes whatever the strings hold."""
    extras = dict(list((extras or {}).items())[:5])
    for maxlen in (240, 160, 100, 60):
        line = {k: full.get(k) for k in TOP_KEYS}
        cfg = full.get("config") or {}
        line["config"] = {k: cfg.get(k) for k in ("workload", "parallelism")}
        roof, base = full.get("roofline"), full.get("cpu_baseline")
        line["roofline"] = {k: roof.get(k) for k in ROOF_KEYS} if isinstance(roof, dict) else None
        line["cpu_baseline"] = {k: base.get(k) for k in BASE_KEYS} if isinstance(base, dict) else None
        for k, v in extras.items():
            line[k] = v if isinstance(v, (int, float, bool, type(None), np.floating, np.integer)) else str(v)
        line["detail"] = detail
        text = json.dumps(_tidy(line, maxlen), allow_nan=False, separators=(", ", ": "))
        if len(text.encode()) < LINE_LIMIT:
            return text
    raise AssertionError("bench line does not fit %d bytes" % LINE_LIMIT)


def write_detail(full, tag):
    """Everything the run measured, as profiles/bench_detail_<tag>.json (strict JSON); returns the path relative to the
    repository (None when the directory cannot be written: the line is printed regardless)."""
    import re
    rel = os.path.join("profiles", "bench_detail_" + re.sub(r"[^A-Za-z0-9_.-]", "_", tag) + ".json")
    try:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, rel), "w") as f:
            json.dump(_tidy(full, 2000), f, allow_nan=False, indent=1)
            f.write("\n")
        return rel
    except Exception:
        return None


def emit(full, tag, extras=None, detail=True):
    print(compact_line(full, extras, write_detail(full, tag) if detail else None), flush=True)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, arrays, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: every non-empty array as <path>/<name>.npy in float64, at most `limit` bytes in all.  When the arrays are
    larger, the small ones are written whole and each larger one as a fixed sample of its entries (positions drawn with seed 0,
    kept in order), so that two runs with the same arguments write the same positions."""
    os.makedirs(path, exist_ok=True)
    arrays = {k: np.ascontiguousarray(np.asarray(v, dtype=np.float64).ravel()) for k, v in arrays.items()}
    arrays = {k: v for k, v in arrays.items() if v.size}
    budget = limit // 8
    for i, (name, a) in enumerate(sorted(arrays.items(), key=lambda kv: kv[1].size)):
        share = budget // (len(arrays) - i)
        if a.size > share:
            a = a[np.sort(np.random.default_rng(0).choice(a.size, share, replace=False))]
        budget -= a.size
        np.save(os.path.join(path, name + ".npy"), a)


def plan_outputs(plan):
    """What a caller of the unit receives from the resident plan: ADA' and absd (getada3), L.L on its pattern and L.d (blkchol),
    blkchol's Lskip / Ladd as one status per row (0 kept, 1 skipped, 2 added) and the pivot value of those rows (0 elsewhere), the
    solution y of the last solve.  Every array has a length fixed by the problem, whatever the pivots."""
    (si, sv), (ai, av) = plan.pivots()
    status, value = np.zeros(plan.m), np.zeros(plan.m)
    status[si], value[si] = 1.0, sv
    status[ai], value[ai] = 2.0, av
    return {"ada": plan.download("ada"), "absd": plan.download("absd"), "L": plan.download("lpr"), "d": plan.download("d"),
            "y": plan.download("y"), "pivot_status": status, "pivot_value": value}


def relaunch(args):
    """`python bench.py --gpus N` with no launcher around it: the same command under torch.distributed.run, one rank per
    GPU, rendezvous on 127.0.0.1; rank 0's line passes through on stdout."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def dry_run(args, rank, world):
    """--dry-run: the launcher / process-group / line plumbing only, on CPU (gloo): barrier, K empty steps, MAX over ranks.
    NOTHING is measured and the line says so (value null); what tests/test_bench_line.py runs at world size 1 and 2."""
    dist = None
    if world > 1:
        import torch
        import torch.distributed as dist
        dist.init_process_group(backend="gloo")
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pass
    elapsed = time.perf_counter() - t0
    if dist is not None:
        dist.barrier()
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0:
        full = {"metric": "DRY RUN (plumbing only, nothing measured)", "value": None, "unit": "IPM iters/s", "n_gpus": world, "steps": args.steps,
                "warmup": args.warmup, "ms_per_step": None, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
                "data": "none", "config": {"workload": args.workload, "parallelism": f"{world} rank(s), gloo"}, "roofline": None, "cpu_baseline": None}
        print(compact_line(full, {"dry_run": True}), flush=True)
    if dist is not None:
        dist.destroy_process_group()


def build_workload(name, seed):
    """(P, L, ADApattern, Qpattern, d, udsqr, rhs, qpr, data_note)"""
    import scipy.sparse as sp
    from sedumi_amd import mex, problem
    qpr = None
    gold = {"control07": ("control07", "rand"), "control07_init": ("control07", "init"), "arch0": ("arch0", "rand"), "arch0_init": ("arch0", "init"),
            "nb": ("nb", "rand"), "nb_init": ("nb", "init")}
    if name in gold:
        # the reference's own examples: hot-path inputs of examples/<name>.mat (At after pretransfo, K, a scaling, rhs) from
        # tests/golden/<name>.npz; tag "init" = the identity scaling of iteration 1 (sdinit.m:63-78), "rand" = an ill-conditioned one
        fname, tag = gold[name]
        z = np.load(os.path.join(ROOT, "tests", "golden", fname + ".npz"))
        At = sp.csc_matrix((z["At_data"], z["At_indices"], z["At_indptr"]), shape=tuple(z["At_shape"]))
        K = problem.make_K(int(z["K_l"]), z["K_q"].ravel(), z["K_s"].ravel())
        P = problem.Problem(At, K, fname + ".mat")
        assert np.array_equal(P.Ablkjc, z["Ablkjc"])
        d = {"l": z[f"{tag}_dl"], "det": z[f"{tag}_ddet"]}
        ud, rhs = z[f"{tag}_udsqr"], z["rhs"]
        note = f"examples/{fname}.mat inputs (tests/golden/{fname}.npz), scaling of the golden '{tag}' tag"
        L, ADA = problem.dense_symbolic(P.m), problem.dense_pattern(P.m)
        Q = sp.csc_matrix((z[f"{tag}_DAtq_data"], z[f"{tag}_DAtq_indices"], z[f"{tag}_DAtq_indptr"]), shape=tuple(z[f"{tag}_DAtq_shape"]))
        if Q.nnz:                                       # Lorentz cones: the DAt.q of getDAtm.m for this scaling, values in the order of its pattern
            Q.sort_indices()
            qpr = np.asarray(Q.data, dtype=np.float64)
        return P, L, ADA, Q, d, ud, rhs, qpr, note
    else:
        if name == "control07_like":
            P = problem.control_like(seed=seed)
        elif name.startswith("maxcut"):
            P = problem.maxcut(int(name[6:] or 4000))
        elif name == "nb_like":                         # BASELINE.json configs[2] shape: 793 Lorentz cones of dimension 3, m = 123
            P = problem.random_sdp(m=123, lp=4, q=(3,) * 793, s=(), dens=0.66, seed=31 + seed)
            P.name = "nb_like(m=123,q=793x3)"
        elif name.startswith("blockdiag"):
            parts = name.split(":")
            nblk, n, mper = (int(parts[1]), int(parts[2]), int(parts[3])) if len(parts) == 4 else (64, 200, 150)
            P = problem.blockdiag_sdp(nblk=nblk, n=n, mper=mper, nnz=20, seed=4)
        else:
            raise SystemExit("unknown workload " + name)
        d, ud = problem.spd_scaling(P.K, seed=seed + 5)
        rhs = np.random.default_rng(seed).standard_normal(P.m)
        note = "synthetic"
    if name.startswith("blockdiag"):
        ADA = problem.symb_ada(P)
        L = mex.symbchol(ADA)                           # our own ordmmd + symfct (bit-exact with the reference)
    else:
        L, ADA = problem.dense_symbolic(P.m), problem.dense_pattern(P.m)
    Q = problem.lorentz_pattern(P)
    if Q.nnz:                                           # Lorentz cones: DAt.q values in the order of the pattern (getDAtm.m's product)
        qpr = 0.1 * np.random.default_rng(3).standard_normal(Q.nnz)
    return P, L, ADA, Q, d, ud, rhs, qpr, note


def build_lpdense(seed=1, m=2000, n=20000, ndense=8):
    """SURVEY.md 8(d) config 3 variant: sparse LP (m=2000, N=20000, 1 % density) with 8 fully dense variables, the case
    that exercises the dense-column leg of the unit: + sparse fwblkslv + dpr1fact + 4 x (fwdpr1 + bwdpr1).  Symbolic
    side (sedumi.m:356-392, symbcholden.m:43-55) through this library's own ordmmd / symfct / symbfwblk / incorder /
    finsymbden."""
    import scipy.sparse as sp
    from sedumi_amd import mex, problem
    rng = np.random.default_rng(seed)
    P0 = problem.lp_dense_cols(m=m, n=n, dens=0.01, ndense=ndense, seed=seed)
    At = sp.csc_matrix(P0.At)
    rows_dense = 1 + np.arange(ndense)
    denseA = sp.csc_matrix(At[rows_dense, :].T)                       # m x ndense (sedumi.m:359)
    keep = np.ones(At.shape[0]); keep[rows_dense] = 0.0
    P = problem.Problem(sp.csc_matrix(sp.diags(keep) @ At), P0.K, f"lp_dense_cols(m={m},n={n},dense={ndense})")   # sedumi.m:360
    P.At.eliminate_zeros()
    P = problem.Problem(P.At, P0.K, P.name)
    dl = 10.0 ** rng.uniform(-1, 1, At.shape[0])
    ADA = sp.csc_matrix(P.At.T @ P.At); ADA.data[:] = 1.0; ADA.sort_indices()
    L = mex.symbchol(ADA)
    LADsym = mex.symbfwblk(L, denseA)
    perm, dz = mex.incorder(LADsym)
    sym = mex.finsymbden(LADsym, perm, dz, float(ndense + 1))
    return P, L, ADA, {"l": dl, "det": np.zeros(0)}, np.zeros(0), rng.standard_normal(m), sym, denseA, dl[rows_dense]


def bench_lpdense(args, device):
    """One GPU, the unit WITH the dense-column leg: getada (LP part), blkchol, deninfac (LAD = L \\ Ad for the 8 columns at
    once + dpr1fact), 4 x (fwblkslv, fwdpr1, ./Ld, bwdpr1, bwblkslv)."""
    from sedumi_amd import problem
    P, L, ADA, d, ud, rhs, sym, denseA, smult = build_lpdense()
    plan = make_plan(device, P, L, ADA, problem.lorentz_pattern(P), d, ud, rhs, None)
    plan.set_dense(sym)
    plan.upload("ad", np.asarray(denseA.todense()).ravel(order="F"))
    host = [False]

    def step():
        plan.getada()
        plan.blkchol(PARS, True)
        host[0] = plan.deninfac(smult, 500.0) or host[0]
        for _ in range(NSOLVE):
            plan.ldlsolve()
    el = time_steps(plan, step, args.steps, args.warmup)
    if args.dump_outputs:
        lden, dden = plan.lden()
        dump_outputs(args.dump_outputs, dict(plan_outputs(plan), dden=dden, **{"lden_" + k: v for k, v in lden.items()}))
    phases = None
    if args.full:
        ph = np.zeros(4)
        nprof = min(args.steps, 20)
        for _ in range(nprof):
            plan.timer_begin(0); plan.getada(); plan.timer_end(0)
            plan.timer_begin(1); plan.blkchol(PARS, True); plan.timer_end(1)
            t0 = time.perf_counter(); plan.deninfac(smult, 500.0); plan.sync(); ph[2] += 1e3 * (time.perf_counter() - t0)
            plan.timer_begin(3)
            for _ in range(NSOLVE):
                plan.ldlsolve()
            plan.timer_end(3)
            ph[[0, 1, 3]] += [plan.timer_ms(0), plan.timer_ms(1), plan.timer_ms(3)]
        ph /= nprof
        phases = {"ada_ms": ph[0], "factor_ms": ph[1], "deninfac_ms_host_timed": ph[2], "solves_ms": ph[3], "dpr1fact_on_host_fallback": bool(host[0])}
    emit({
        "metric": "IPM iters/sec (ADA' form+factor+solve)", "value": args.steps / el, "unit": "IPM iters/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": 1e3 * el / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"{P.name}: sparse LP with dense columns (SURVEY.md 8(d) config 3 variant), m={P.m}, nnz(L)={plan.nnzL}, "
                               f"nsuper={np.asarray(L['xsuper']).size - 1}; unit = getada, blkchol, deninfac (sparse fwblkslv x 8 + dpr1fact), "
                               f"{NSOLVE}x(fwblkslv, fwdpr1, ./Ld, bwdpr1, bwblkslv)", "parallelism": "single GPU"},
        "roofline": None, "cpu_baseline": None, "phases_ms_per_step": phases}, "lpdense_n1", detail=args.full)
    plan.close()


def make_plan(device, P, L, ADA, Q, d, ud, rhs, qpr, one_launch_fronts=True):
    from sedumi_amd.plan import Plan
    plan = Plan(device)
    if not one_launch_fronts:
        plan.set_one_launch_fronts(False)                # the launch-per-panel path (--shard blockcyclic exchanges the panels between its launches)
    plan.set_chol(L, ADA)
    plan.set_ada(P.At, P.Ablkjc, P.K, Q)
    plan.upload("dl", d["l"]); plan.upload("ddet", d["det"]); plan.upload("udsqr", ud); plan.upload("rhs", rhs)
    if qpr is not None:
        plan.upload("qpr", qpr)
    return plan


def cpu_baseline(P, d, ud, rhs, budget_s=12.0, blas=None, max_units=400):
    """The compiled reference MEX (oracle/_ref) timed on this host, one thread, on a bounded sample of the same
    workload: repeated iteration units until ~budget_s of CPU time is spent (at most max_units).  blas = (path, prefix, suffix): the
    reference's BLAS-1 calls bound to that host BLAS instead of the shim's naive loops.  Problems without PSD blocks (nb.mat) take
    getada.m's route in sedumi.m:446-448 -- MATLAB sparse products, not timeable here: getada1 + getada2 (the same sums as MEX calls)
    stand in for it and getada3 is not called."""
    kind = {"value": None, "unit": "IPM iters/s", "cores": 1, "kind": "reference"}
    try:
        from oracle import glue as gl, refmex
        if not refmex.available():
            return None
        G = gl.Glue()
        ref = G.ref
        if blas is not None and not ref.use_blas(blas):
            return dict(kind, sample="failed: could not bind " + blas[0])
        S = G.setup(P.At, P.K)
        K = P.K
        dd = {"l": d["l"], "det": d["det"], "q1": np.ones(K["q"].size),
              "q2": np.zeros(int(K["mainblks"].ravel()[2] - K["mainblks"].ravel()[1]))}
        DAt = G.getDAtm(S, dd)
        dstruct = {"l": np.asarray(dd["l"]).reshape(-1, 1), "det": np.asarray(dd["det"]).reshape(-1, 1)}
        units, tot = 0, 0.0
        stage = np.zeros(4)
        t_wall = time.perf_counter()
        while True:
            t1, ADA1 = ref.timed_call("getada1", 1, (S["ADA"], S["A"], S["Ablkjc"][:, 2], S["Aord"]["lqperm"], dstruct, K["qblkstart"]))
            t2, ADA2 = ref.timed_call("getada2", 1, (ADA1, DAt, S["Aord"], K))
            if np.asarray(K["s"]).size:
                t3, (ADA3, absd) = ref.timed_call("getada3", 2, (ADA2, S["A"], S["Ablkjc"][:, 2], S["Aord"], np.asarray(ud).reshape(-1, 1), K))
            else:
                t3, ADA3, absd = (0.0,), ADA2, np.asarray(ADA2.diagonal()).reshape(-1, 1)
            t4, (LL, Ld, _, _) = ref.timed_call("blkchol", 4, (S["L"], ADA3, dict(PARS), absd))
            L = dict(S["L"]); L["L"] = LL
            ts = 0.0
            for _ in range(NSOLVE):
                tf, p = ref.timed_call("fwblkslv", 1, (L, rhs.reshape(-1, 1)))
                tb, _y = ref.timed_call("bwblkslv", 1, (L, p / Ld))
                ts += tf[0] + tb[0]
            tot += t1[0] + t2[0] + t3[0] + t4[0] + ts
            stage += [t1[0] + t2[0], t3[0], t4[0], ts]
            units += 1
            if tot >= budget_s or time.perf_counter() - t_wall > 3 * budget_s or units >= max_units:
                break
        if blas is not None:
            ref.use_blas(None)
        what = "OpenBLAS BLAS-1 (" + os.path.basename(blas[0]) + ", 1 thread)" if blas else "naive BLAS-1"
        return dict(kind, value=units / tot,
                    sample=f"{units} iteration units of {P.name} through oracle/_ref (unmodified reference C, gcc -O2, {what}), "
                           f"MEX calls only ({tot:.1f} s CPU)",
                    stage_ms_per_unit={"getada1+2": 1e3 * stage[0] / units, "getada3": 1e3 * stage[1] / units,
                                       "blkchol": 1e3 * stage[2] / units, "solves": 1e3 * stage[3] / units})
    except Exception as e:  # the baseline must never break the bench line
        return dict(kind, sample=f"failed: {e}")


def unit_fn(plan):
    def step():
        plan.getada()
        plan.blkchol(PARS, True)
        for _ in range(NSOLVE):
            plan.ldlsolve()
    return step


def time_steps(plan, step, steps, warmup):
    for _ in range(warmup):
        step()
    plan.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    plan.sync()
    return time.perf_counter() - t0


def profile_unit(plan, P, ud, nprof):
    """Roofline leg: the same steps with HIP events on the plan's stream -- around every launch (per-kernel times)
    and, in a second pass, around the three phases of the unit (ADA', factor incl. the inverses for the solves, the
    four solves).  Returns (roofline dict, phases dict)."""
    m, nnzL = plan.m, plan.nnzL
    step = unit_fn(plan)
    plan.kprof(True)
    for _ in range(nprof):
        step()
    prof = plan.kprof_summary()
    plan.kprof(False)
    ph = np.zeros(3)
    for _ in range(nprof):
        plan.timer_begin(0); plan.getada(); plan.timer_end(0)
        plan.timer_begin(1); plan.blkchol(PARS, True); plan.timer_end(1)
        plan.timer_begin(2)
        for _ in range(NSOLVE):
            plan.ldlsolve()
        plan.timer_end(2)
        ph += [plan.timer_ms(0), plan.timer_ms(1), plan.timer_ms(2)]
    ph /= nprof
    # ALGORITHMIC work per launch of each hot kernel (SURVEY.md 8(d) per-unit figures divided
    # by the launches per unit).  bound "hbm": bytes, peak 8 TB/s; bound "mfma": FP64 flops, peak 78.6 TFLOP/s.
    lind = int(np.sum(np.diff(plan.L_pattern.indptr)[(np.asarray(plan_xsuper(plan)) - 1)[:-1]])) if hasattr(plan, "L_pattern") else m
    solve_bytes = 8.0 * nnzL + 8.0 * lind + 16.0 * m    # per triangular sweep: 8*nnz(L) + 8*len(lindx) + 16*m
    fac_flops = factor_flops(plan)
    # on the device the LAST workgroups of a k_ldl_front launch build the triangular inverses of the fronts' diagonal super-blocks for the
    # solves (n^3 / 3 flops per front of n columns): the launch's work is both -- recognised by no inverse kernel of its own in the profile
    xs_ = np.asarray(plan_xsuper(plan), dtype=np.float64)
    inv_flops = float(np.sum(np.diff(xs_) ** 3) / 3.0)
    inv_in_front_launch = "k_ldl_front" in prof and not any(k in prof for k in ("k_sprep", "k_sinv128", "k_sinv_follow", "k_stile"))
    front_flops = fac_flops                       # the factorisation's flops only; the inverse the launch also builds is reported beside it
    npanel = max(1, prof.get("k_ldl_panel", (1, 0))[0] // nprof)
    ada_bytes = 8.0 * (ud.size + P.At.nnz + plan.nnzADA)
    model = {
        "k_ldl_panel": ("mfma", fac_flops / npanel),                               # the panel launches carry the whole LDL'
        "k_ldl_front": ("mfma", front_flops / max(1, prof.get("k_ldl_front", (nprof, 0))[0] // nprof)),   # ... or ONE launch per level does
        "k_ldl_update": ("mfma", fac_flops / npanel),
        "k_psd_stage1_mfma": ("mfma", None), "k_psd_stage1": ("fp64_vector", None),  # flops filled below from the task list (the two-dot kernel has no MFMA in it)
        "k_psd_stage2": ("hbm", 8.0 * (P.At.nnz + plan.nnzADA)), "k_psd_stage2_ell": ("hbm", 8.0 * (P.At.nnz + plan.nnzADA)),
        "k_ada_spdot": ("hbm", 8.0 * (P.At.nnz + plan.nnzADA)),
        "k_psd_direct": ("hbm", 8.0 * (ud.size + 2.0 * plan.nnzADA)),                # D_k once, ADA' read and written
        "k_sfw_step": ("hbm", None), "k_sbw_step": ("hbm", None), "k_sfw_diag": ("hbm", None), "k_sbw_diag": ("hbm", None),
    }
    peaks = {"hbm": (HBM_PEAK_GBS, "GB/s", 1e9), "mfma": (FP64_MATRIX_PEAK_TFS, "TFLOP/s", 1e12),
             "fp64_vector": (FP64_MATRIX_PEAK_TFS, "TFLOP/s", 1e12)}                    # (the FP64 vector rate equals the matrix rate on CDNA4)
    # (k_sinv_follow -- the emulator's form of the workgroups that build the inverse behind the factor -- spends most of its time waiting for it:
    # its events overlap that kernel's, it is not a stage of its own)
    dom = max(((k, v) for k, v in prof.items() if k != "k_sinv_follow"), key=lambda kv: kv[1][1])[0] if prof else None
    roof = None
    if dom:
        calls, ms = prof[dom]
        avg_s = ms / calls * 1e-3
        key = dom.split("<")[0]
        bound, work = model.get(key, ("hbm", None))
        if work is None and key.startswith("k_psd_stage1"):
            work = stage1_flops(P) / max(1, calls // nprof)
        if work is None and key in ("k_sfw_step", "k_sbw_step", "k_sfw_diag", "k_sbw_diag"):
            work = solve_bytes / max(1, 2 * calls // (nprof * NSOLVE))       # a sweep = its diagonal-block and its step launches (about half the bytes each)
        if work is None:
            work = ada_bytes
        peak, unit, scale = peaks[bound]
        ach = work / avg_s / scale
        roof = {"kernel": dom, "bound": bound, "achieved": ach, "peak": peak, "unit": unit, "frac": ach / peak,
                "traffic": None, "avg_launch_us": avg_s * 1e6, "launches_per_step": calls / nprof,
                "algorithmic_work_per_launch": work,
                **({"work_is": "LDL' of the fronts, SURVEY.md 8(d) (%.4g flops)" % fac_flops,
                    "also_in_this_launch_not_counted": "the triangular inverses of the fronts' diagonal super-blocks for the solves (%.4g flops), built by the "
                                                       "last workgroups of the same launch" % inv_flops} if key == "k_ldl_front" and inv_in_front_launch else {}),
                "timing": "HIP events around every launch on the plan's stream (adds ~2 us per launch; kernels shorter than "
                          "~7 us read as ~7 us: see phases_ms_per_step for those)",
                "stage_ms_per_step": {k: v[1] / nprof for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])}}
        import glob
        # the committed PMC file of THIS workload (tools/profile_round.sh <tag>_<workload> <workload>), latest round
        import re
        key = re.sub(r"[^a-z0-9]", "", P.name.lower().split(".")[0].replace("(n=", "").replace("_sdp", ""))
        key = "blockdiag" if key.startswith("blockdiag") else key
        pmcs = sorted(f for f in glob.glob(os.path.join(ROOT, "profiles", "*pmc_traffic.json")) if key and ("_" + key + "_") in os.path.basename(f))
        if pmcs:
            try:
                roof["traffic_from_committed_profile"] = {"bytes_per_launch": json.load(open(pmcs[-1])).get(dom),
                                                          "source": "profiles/" + os.path.basename(pmcs[-1]) + " (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command on the "
                                                                    "committed build, tools/profile_round.sh; PMC passes cannot run inside the timed bench)"}
                roof["traffic"] = roof["traffic_from_committed_profile"]["bytes_per_launch"]
                if dom in ("k_ldl_front", "k_ldl_panel") and roof["traffic_from_committed_profile"]["bytes_per_launch"]:
                    # what the factor kernel has to move at least: every front read once and written once, per launch
                    nsup = int(np.asarray(plan_xsuper(plan)).size - 1)
                    fs = float(np.sum(plan.front_layout(nsup)["fsize"]))
                    alg = 16.0 * fs / max(roof["launches_per_step"], 1e-9)
                    roof["traffic_from_committed_profile"]["algorithmic_bytes_per_launch"] = alg
                    roof["traffic_from_committed_profile"]["traffic_over_algorithmic_bytes"] = roof["traffic_from_committed_profile"]["bytes_per_launch"] / alg
            except Exception:
                pass
    nlaunch = sum(v[0] for k, v in prof.items() if k.startswith("k_sfw") or k.startswith("k_sbw")) / max(1, nprof * NSOLVE)
    t_solve = ph[2] / NSOLVE * 1e-3
    nb, nbad, growth = plan.solve_stats()
    phases = {"ada_ms": ph[0], "factor_ms": ph[1], "solves_ms": ph[2],
              "solve": {"us_per_solve": 1e6 * t_solve, "launches_per_solve": nlaunch, "us_per_launch": 1e6 * t_solve / max(nlaunch, 1),
                        "algorithmic_bytes_per_solve": 2.0 * solve_bytes, "achieved_GBs": 2.0 * solve_bytes / t_solve / 1e9,
                        "frac_of_hbm_peak": 2.0 * solve_bytes / t_solve / 1e9 / HBM_PEAK_GBS,
                        "dependency_chain": f"{nlaunch:.0f} dependent launches per solve x measured {1e6 * t_solve / max(nlaunch, 1):.2f} us per launch "
                                            "(launch boundary + the launch's own streaming)",
                        "super_block_width": plan.solve_width(),
                        "super_blocks": nb, "blocks_beyond_growth_bound": nbad, "max_growth": growth},
              "factor": {"flops": fac_flops, "achieved_TFLOPs": fac_flops / (ph[1] * 1e-3) / 1e12,
                         "frac_of_fp64_matrix_peak": fac_flops / (ph[1] * 1e-3) / 1e12 / FP64_MATRIX_PEAK_TFS}}
    return roof, phases


def plan_xsuper(plan):
    return getattr(plan, "_xsuper", [1, plan.m + 1])


def factor_flops(plan):
    """sum over supernodes of n*m^2 - n^2*m + n^3/3 from the symbolic factor."""
    Ljc = np.asarray(plan.L_pattern.indptr, dtype=np.float64)
    xs = np.asarray(plan_xsuper(plan), dtype=np.int64) - 1
    tot = 0.0
    for a, b in zip(xs[:-1], xs[1:]):
        n = float(b - a); ms = float(Ljc[a + 1] - Ljc[a])
        tot += n * ms * ms - n * n * ms + n ** 3 / 3.0
    return tot


def stage1_flops(P):
    """FLOPs of ADA' stage 1 per unit, summed over the (constraint j, PSD block k) tasks that have nonzeros (DESIGN.md
    section 3): blocks of order n <= 96 (k_psd_stage1_mfma) 2 n^2 nslot (Z = Y D(cols,:) dense) + 2 nnz n (Y); larger and
    Hermitian blocks (k_psd_stage1) 2 nnz n + 4 |U_k| nslot (two dots per target of the block's union pattern U_k);
    nslot = distinct columns among the stored nonzeros of A_jk."""
    K = P.K
    s = K["s"].ravel().astype(np.int64)
    if not s.size:
        return 0.0
    import scipy.sparse as sp
    At = sp.csc_matrix(P.At)
    start = (K["blkstart"].ravel().astype(np.int64) - 1)[1 + K["q"].size:]            # first row of every PSD block, then N
    rsdpN = int(np.asarray(K.get("rsdpN", s.size)).ravel()[0])
    rows = At.indices
    cols = np.repeat(np.arange(At.shape[1]), np.diff(At.indptr))
    sel = rows >= start[0]
    rows, cols = rows[sel], cols[sel]
    blk = np.searchsorted(start, rows, side="right") - 1
    off = rows - start[blk]
    n = s[blk]
    colin = (off % (n * n)) // n                                                       # column inside the block (either plane)
    task = cols.astype(np.int64) * s.size + blk
    nnz_t = np.bincount(task, minlength=At.shape[1] * s.size).astype(np.float64)
    slot_key = np.unique(task * (int(s.max()) + 1) + colin)
    nslot_t = np.bincount(slot_key // (int(s.max()) + 1), minlength=At.shape[1] * s.size).astype(np.float64)
    ulen = np.bincount(blk[np.unique(blk * (2 * int(s.max()) ** 2 + 1) + off, return_index=True)[1]], minlength=s.size).astype(np.float64)
    tot = 0.0
    for k in range(s.size):
        nk, sl = float(s[k]), slice(k, None, s.size)
        if s[k] <= 96 and k < rsdpN and s.max() <= 96:
            tot += float(np.sum(2.0 * nk * nk * nslot_t[sl] + 2.0 * nnz_t[sl] * nk))
        else:
            tot += float(np.sum(2.0 * nnz_t[sl] * nk + 4.0 * ulen[k] * nslot_t[sl]))
    return tot


def solve_leg(name, device, nsolve=200):
    """Only the solves of a workload (one ADA' + factorisation, then `nsolve` fw + ./d + bw solves timed): what the row-dot kernels
    stream once the launch boundaries amortise (maxcut8000: 256 MB of factor per sweep)."""
    try:
        t0 = time.perf_counter()
        P, L, ADA, Q, d, ud, rhs, qpr, note = build_workload(name, 0)
        plan = make_plan(device, P, L, ADA, Q, d, ud, rhs, qpr)
        plan._xsuper = np.asarray(L["xsuper"]).ravel().astype(np.int64)
        plan.getada(); plan.blkchol(PARS, True)
        for _ in range(5):
            plan.ldlsolve()
        plan.sync()
        t1 = time.perf_counter()
        for _ in range(nsolve):
            plan.ldlsolve()
        plan.sync()
        t_solve = (time.perf_counter() - t1) / nsolve
        plan.kprof(True)
        for _ in range(10):
            plan.ldlsolve()
        prof = plan.kprof_summary()
        plan.kprof(False)
        m, nnzL = plan.m, plan.nnzL
        xs = np.asarray(plan_xsuper(plan))
        lind = int(np.sum(np.diff(plan.L_pattern.indptr)[(xs - 1)[:-1]]))
        bytes_solve = 2.0 * (8.0 * nnzL + 8.0 * lind + 16.0 * m)
        nb, nbad, growth = plan.solve_stats()
        out = {"workload": name + " (solve leg only)", "problem": P.name, "m": int(m), "nnzL": int(nnzL), "us_per_solve": 1e6 * t_solve,
               "algorithmic_bytes_per_solve": bytes_solve, "achieved_GBs": bytes_solve / t_solve / 1e9, "frac_of_hbm_peak": bytes_solve / t_solve / 1e9 / HBM_PEAK_GBS,
               "launches_per_solve": sum(v[0] for v in prof.values()) / 10.0, "super_block_width": plan.solve_width(), "super_blocks": nb,
               "kernel_us_with_events": {k: v[1] / v[0] * 1e3 for k, v in sorted(prof.items())}, "setup_s": time.perf_counter() - t0 - nsolve * t_solve}
        plan.close()
        return out
    except Exception as e:  # never break the bench line
        return {"workload": name + " (solve leg only)", "error": repr(e)}


def measure_config(name, device, steps, warmup, nprof, mex_units=0, growth_max=None, refine=1, cpu_units=0):
    """One of the other BASELINE configs, measured briefly in this process: ms/unit, dominant kernel, solve rate.  growth_max: the
    bound beyond which a super-block of the solves is no longer applied as its bare inverse (0 = every block is beyond it); refine:
    what happens to those blocks (sdm_plan_set_refinement: 1 = inverse + iterative refinement, the default; 0 = substitution).
    cpu_units: that many units of the reference MEX on this host beside it (cpu_baseline), and the speed-ups against it."""
    try:
        t0 = time.perf_counter()
        P, L, ADA, Q, d, ud, rhs, qpr, note = build_workload(name, 0)
        plan = make_plan(device, P, L, ADA, Q, d, ud, rhs, qpr)
        if growth_max is not None:
            plan.set_growth_max(growth_max)
            plan.set_refinement(refine)
        plan._xsuper = np.asarray(L["xsuper"]).ravel().astype(np.int64)
        step = unit_fn(plan)
        el = time_steps(plan, step, steps, warmup)
        roof, phases = profile_unit(plan, P, ud, nprof)
        mexleg = mexlazy = None
        if mex_units:
            plan.upload("rhs", rhs); plan.ldlsolve()
            yres = plan.download("y")
            mexleg = mex_inclusive(P, L, ADA, Q, d, ud, rhs, qpr, mex_units, yres)
            if name.startswith("maxcut") or name.startswith("blockdiag"):
                mexlazy = {"level_%d" % lv: mex_inclusive(P, L, ADA, Q, d, ud, rhs, qpr, mex_units, yres, lazy=lv) for lv in (0, 1)}
        out = {"workload": name, "problem": P.name, "m": int(P.m), "nnzL": int(plan.nnzL), "nsuper": int(plan._xsuper.size - 1),
               "ms_per_step": 1e3 * el / steps, "iters_per_s": steps / el, "steps": steps,
               "dominant_kernel": roof and {k: roof[k] for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "avg_launch_us", "launches_per_step")},
               "phases_ms_per_step": {k: phases[k] for k in ("ada_ms", "factor_ms", "solves_ms")},
               "solve": phases["solve"], "factor": phases["factor"], "setup_s": time.perf_counter() - t0 - el}
        if mexleg is not None:
            out["mex_inclusive"] = mexleg
        if mexlazy:
            out["mex_inclusive_lazy"] = mexlazy
        if cpu_units:
            t1 = time.perf_counter()
            base = cpu_baseline(P, d, ud, rhs, budget_s=8.0, max_units=cpu_units)
            out["cpu_baseline"] = base
            out["setup_s"] -= time.perf_counter() - t1
            if base and base.get("value"):
                out["speedup_vs_cpu_reference"] = out["iters_per_s"] / base["value"]
                if mexleg and mexleg.get("value"):
                    out["mex_inclusive_speedup_vs_cpu_reference"] = mexleg["value"] / base["value"]
                for k, v in (mexlazy or {}).items():
                    if v.get("value"):
                        out["mex_inclusive_lazy_" + k + "_speedup_vs_cpu_reference"] = v["value"] / base["value"]
        if growth_max is not None:
            out["workload"] = (f"{name} (solves with growth_max = {growth_max:g}: every super-block beyond the bound, as in the last iterations of a run; " +
                               ("inverse + two refinement steps against the factor)" if refine else "substituted by one workgroup: sdm_plan_set_refinement(0))"))
        plan.close()
        return out
    except Exception as e:  # never break the bench line
        return {"workload": name, "error": repr(e)}


def pcie_inclusive(plan, P, d, ud, rhs, steps):
    """The same unit with every MEX-boundary transfer of the tier-1 flow inside the timed region (host buffers in and
    out around each of the six calls, as the mexFunction shims with the cached plan do): never `value`."""
    m = plan.m
    nA, nL = plan.nnzADA, plan.nnzL

    def step():
        plan.upload("dl", d["l"]); plan.upload("ddet", d["det"]); plan.upload("udsqr", ud)
        plan.getada()
        ada = plan.download("ada", nA); absd = plan.download("absd", m)          # getada3 returns ADA, absd
        plan.upload("ada", ada); plan.upload("absd", absd)                         # blkchol(L, ADA, pars, absd)
        plan.blkchol(PARS, True)
        plan.download("lpr", nL); dd = plan.download("d", m)                       # [L.L, L.d, ...]
        for _ in range(NSOLVE):
            plan.upload("rhs", rhs); plan.fwsolve(); y = plan.download("y", m)     # fwblkslv
            plan.upload("rhs", y / np.where(dd > 0, dd, 1.0)); plan.bwsolve(); plan.download("y", m)   # ./L.d in MATLAB, bwblkslv
    for _ in range(2):
        step()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    el = time.perf_counter() - t0
    return {"value": steps / el, "unit": "IPM iters/s", "ms_per_step": 1e3 * el / steps, "steps": steps,
            "note": "host buffers cross PCIe around every one of the 6 + 2x4 MEX-equivalent calls (pageable numpy memory, "
                    f"synchronous copies): {8 * (3 * nA + 2 * nL) / 1e6:.1f} MB per unit"}


def mex_inclusive(P, L, ADA, Q, d, ud, rhs, qpr, units, y_resident=None, mex_dir=None, lazy=None):
    """The unit as an UNMODIFIED sedumi.m would run it: through the built mexFunction shims (sedumi_amd/lib/mex/<name>.so, the
    sources of sedumi_amd/mexshims compiled against the package's MEX host -- no MATLAB / Octave in this image), host mxArrays in
    and out of every one of the 4 + 2x4 gateway calls, outputs handed to the next gateway by reference as MATLAB does
    (sedumi_amd.mexhost.iteration_units).  Times only what happens inside mexFunction, like cpu_baseline does for the reference
    MEX.  The library's process-wide cache (sdm_mexcache.hip) keeps the analysis of At / K / the patterns and the value arrays that
    travel between gateways on the device.  lazy = None: the library's default (level 2 since round 6: getada1 / getada2 / getada3 hand a
    token to the next gateway, ADA' stays on the device; SEDUMI_HIP_LAZY=0 turns it off); 0 / 1 / 2: that level.  Never `value`."""
    try:
        import ctypes
        import scipy.sparse as sp
        from sedumi_amd import capi, mex, mexhost
        K = P.K
        if not np.asarray(K["s"]).size:
            return {"skipped": "no PSD blocks: sedumi.m:446 takes the getada.m route"}
        m = P.m
        At = sp.csc_matrix(P.At)
        # Aord of sedumi.m:363-378: constraints from sparse to dense (sortnnz: by nonzero count of the part), PSD part by incorder
        nlq = np.asarray(P.Ablkjc)[:, 2] - At.indptr[:-1]
        Aord = {"lqperm": (np.argsort(nlq, kind="stable") + 1.0).reshape(-1, 1)}
        Qm = sp.csc_matrix(Q)
        if Qm.nnz:
            Qm = sp.csc_matrix((np.asarray(qpr, dtype=np.float64), Qm.indices, Qm.indptr), shape=Qm.shape)
            Aord["qperm"] = (np.argsort(np.diff(Qm.indptr), kind="stable") + 1.0).reshape(-1, 1)
        else:
            Aord["qperm"] = np.arange(1, m + 1, dtype=np.float64).reshape(-1, 1)
        sperm, _dz = mex.incorder(At, np.asarray(P.Ablkjc)[:, 2], float(np.asarray(K["mainblks"]).ravel()[2]))
        Aord["sperm"] = np.asarray(sperm, dtype=np.float64).reshape(-1, 1)
        dstruct = {"l": np.asarray(d["l"], dtype=np.float64).reshape(-1, 1), "det": np.asarray(d["det"], dtype=np.float64).reshape(-1, 1)}
        lib = capi.lib()
        st = (ctypes.c_int64 * 16)()
        lib.sdm_mexcache_clear()
        lib.sdm_mexcache_set_lazy(-1 if lazy is None else int(lazy))   # (-1: as SEDUMI_HIP_LAZY says, unset = level 2; 0: every gateway returns the reference's arrays)
        level = int(lib.sdm_mexcache_lazy())
        host = mexhost.MexHost(mex_dir)
        try:
            times, y = mexhost.iteration_units(host, At, np.asarray(P.Ablkjc)[:, 2], Aord, K, dstruct, {"q": Qm}, ud, L, ADA, PARS, rhs, units + 1, NSOLVE)
        finally:
            lib.sdm_mexcache_set_lazy(-1)
        lib.sdm_mexcache_stats(st, ctypes.c_int64(16))
        lib.sdm_mexcache_clear()
        first, rest = times[0], times[1:]
        tot = np.array([sum(t.values()) for t in rest])
        stage = {k: 1e3 * float(np.mean([t[k] for t in rest])) for k in rest[0]}
        out = {"value": float(len(rest) / tot.sum()), "unit": "IPM iters/s", "ms_per_step": 1e3 * float(tot.mean()), "steps": len(rest),
               "first_unit_ms": 1e3 * sum(first.values()), "stage_ms_per_unit": stage,
               "cache_counters": {"ada_build": int(st[0]), "ada_reuse": int(st[1]), "ada_upload": int(st[2]), "ada_resident": int(st[3]), "chol_build": int(st[4]),
                                  "chol_reuse": int(st[5]), "x_upload": int(st[6]), "x_resident": int(st[7]), "solve_resident": int(st[8]),
                                  "solve_stateless": int(st[9])},
               "content_checks": {"host_words_checksummed_per_unit": float(st[11]) / len(times), "MB_per_unit": 8e-6 * float(st[11]) / len(times),
                                  "ms_per_unit": 1e-6 * float(st[13]) / len(times), "checksums_per_unit": float(st[14]) / len(times),
                                  "rule": "residency is decided by a checksum of every word of the host array (sdm_mexcache.hip): arrays up to 65536 words at every "
                                          "presentation, larger ones once per address and epoch (= between two blkchol calls)"},
               "lazy_level": level,
               "lazy": ("level %d%s: getada1 / getada2%s return a token, ADA' stays on the device (sdm_mexcache.hip)" % (level, " (the default)" if lazy is None else "", " / getada3" if level > 1 else "")
                        if level else "level 0 (SEDUMI_HIP_LAZY=0): every gateway returns the reference's arrays"),
               "note": "mexFunction shims (sedumi_amd/lib/mex) on the MEX host of the package; host mxArrays cross PCIe at every gateway: scaling "
                       "data and right-hand sides up, absd, L.L, L.d, pivot lists and solutions down (level 0: ADA' three times as well); the first unit "
                       "(analysis of At, the patterns and the symbolic factor, once per solve) is reported separately"}
        if y_resident is not None:
            out["rel_diff_vs_resident_tier"] = float(np.linalg.norm(y - y_resident) / max(np.linalg.norm(y_resident), 1e-300))
        return out
    except Exception as e:  # never break the bench line
        return {"error": repr(e)}


def whole_solve_leg(name="control07", with_reference=True):
    """--other-configs: a WHOLE interior-point solve of one of the reference's examples by the product's MATLAB-free driver (sedumi_amd.driver:
    sedumi.m's loop restated, the hot path on the resident plan, the cone algebra outside it on numpy / LAPACK) and -- the CPU baseline beside it --
    the same loop with the compiled reference as every MEX (tests/driver + oracle/_ref: the checker, timed like cpu_baseline).  Seconds and iterations."""
    try:
        z = np.load(os.path.join(ROOT, "tests", "golden", f"driver_{name}.npz"))
        import scipy.sparse as sp
        from sedumi_amd import problem
        from sedumi_amd.driver import loop as lp
        g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        At = sp.csc_matrix((g["At_data"], g["At_indices"], g["At_indptr"]), shape=tuple(g["At_shape"]))
        K = problem.make_K(int(g["K_l"]), g["K_q"].ravel(), g["K_s"].ravel())
        t0 = time.perf_counter()
        r = lp.Sedumi(At, z["b"], z["c"], K, internal=True).solve()
        out = {"workload": name + " (whole solve, sedumi_amd.driver)", "seconds": time.perf_counter() - t0, "iterations": int(r["iter"]), "cx": float(r["cx"]), "by": float(r["by"]),
               "stop": int(r["STOP"])}
        if with_reference:
            try:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                from driver import sedumi_loop as sl
                t0 = time.perf_counter()
                rr = sl.Sedumi(At, z["b"], z["c"], K, internal=True).solve()
                out["cpu_baseline"] = {"seconds": time.perf_counter() - t0, "iterations": int(rr["iter"]), "cx": float(rr["cx"]), "cores": 1, "kind": "reference",
                                       "sample": "the same loop with the compiled reference as every MEX (oracle/_ref), one whole solve"}
                out["speedup_vs_cpu_reference"] = out["cpu_baseline"]["seconds"] / out["seconds"]
            except Exception as e:
                out["cpu_baseline"] = {"error": repr(e)}
        return out
    except Exception as e:  # never break the bench line
        return {"workload": name + " (whole solve)", "error": repr(e)}


def bench_subtrees(args, rank, local_rank, world, torch, dist, coll_dev):
    """BASELINE.json configs[4]: block-diagonal SDP (default 64 PSD blocks of order 200, 150 constraints each).  The
    64 independent elimination-tree subtrees are dealt to the ranks (sedumi_amd.dist.SubtreeShardedSolver): ADA',
    factor and solves of a subtree never leave its rank; the only exchange is the all-gather of the solution
    segments after each solve.  Total work is fixed: strong scaling."""
    from sedumi_amd import dist as sd, problem
    parts = args.workload.split(":")
    nblk, n, mper = (int(parts[1]), int(parts[2]), int(parts[3])) if len(parts) == 4 else (64, 200, 150)
    P = problem.blockdiag_sdp(nblk=nblk, n=n, mper=mper, nnz=20, seed=4)
    d, ud = problem.spd_scaling(P.K, seed=5)
    rhs = np.random.default_rng(0).standard_normal(P.m)
    dev = coll_dev if dist is not None else torch.device("cpu")
    solver = sd.SubtreeShardedSolver(P, device_index=local_rank, device=dev, pars=PARS)
    solver.upload_scaling(d, ud, P)
    solver.upload_rhs(rhs)                             # inputs resident in HBM before the timed region

    last = [None]

    def step():
        solver.factor()
        for _ in range(NSOLVE):
            last[0] = solver.solve_resident()

    def sync():
        if solver.plan is not None:
            solver.plan.sync()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
    for _ in range(args.warmup):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    if solver.plan is not None:
        solver.plan.sync()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        dist.barrier()
        t = torch.tensor([elapsed], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0 and args.dump_outputs:
        y = np.zeros(P.m)                              # the gathered solution in the problem's order (SubtreeShardedSolver.solve)
        if last[0] is None:
            y[solver.cols] = solver.plan.download("y", solver.cols.size)
        else:
            host, seg = last[0].cpu().numpy(), solver.send.numel()
            for q, c in enumerate(solver.cols_of):
                if c is not None and c.size:
                    y[c] = host[q * seg:q * seg + c.size]
        dump_outputs(args.dump_outputs, {"y": y})
    if rank == 0:
        emit({
            "metric": "IPM iters/sec (ADA' form+factor+solve)", "value": args.steps / elapsed, "unit": "IPM iters/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"{P.name}: block-diagonal SDP (BASELINE.json configs[4]), m={P.m}, {nblk} independent subtrees; "
                                   f"unit = getada1+2+3, blkchol, {NSOLVE}x(fwblkslv,./d,bwblkslv)",
                       "parallelism": f"{world} rank(s): subtrees per rank {[int(c.size // mper) for c in solver.cols_of]}, all-gather of y only"},
            "roofline": None, "cpu_baseline": None}, f"blockdiag_n{world}", detail=args.full)
    if dist is not None:
        dist.destroy_process_group()


def bench_separator(args, rank, local_rank, world, torch, dist, coll_dev):
    """--workload grid[:n]: factor + solves of ONE connected elimination tree sharded by subtrees (sedumi_amd.dist.
    SeparatorShardedSolver, SURVEY.md 8e rows blkchol / fwblkslv / bwblkslv): the matrix is the 5-point operator of an n x n grid
    (m = n^2, made diagonally dominant), standing in for an ADA' whose pattern has real separators.  Unit = blkchol +
    4 x (fwblkslv, ./d, bwblkslv); the matrix values are resident on every rank (what the ADA' layers leave there)."""
    import scipy.sparse as sp
    from sedumi_amd import dist as sd
    parts = args.workload.split(":")
    n = int(parts[1]) if len(parts) > 1 else 160
    T = sp.diags([-1.0, -1.0], [1, -1], shape=(n, n))
    X = sp.csc_matrix(sp.kron(sp.eye(n), T) + sp.kron(T, sp.eye(n)) + 4.5 * sp.eye(n * n)); X.sort_indices()
    rhs = np.random.default_rng(0).standard_normal(n * n)
    dev = coll_dev if dist is not None else torch.device("cuda", local_rank)
    solver = sd.SeparatorShardedSolver(X, device_index=local_rank, device=dev)
    last = [None]

    def step():
        solver.factor(X.data, PARS)
        for _ in range(NSOLVE):
            last[0] = solver.solve(rhs)

    def sync():
        solver.plan.sync()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
    for _ in range(args.warmup):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    solver.plan.sync()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        dist.barrier()
        t = torch.tensor([elapsed], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"y": last[0].cpu().numpy()})
    if rank == 0:
        own = [int(np.sum((solver.owner == r) & ~solver.top)) for r in range(world)]
        emit({
            "metric": "IPM iters/sec (factor+solve of a matrix with separators)", "value": args.steps / elapsed, "unit": "IPM iters/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"grid {n}x{n}: m={n * n}, nnz(L)={solver.plan.nnzL}, nsuper={solver.nsuper}; unit = blkchol, {NSOLVE}x(fwblkslv,./d,bwblkslv); "
                                   "right-hand side uploaded per solve",
                       "parallelism": f"{world} rank(s): {int(solver.top.sum())} separator supernodes on rank 0, subtree supernodes per rank {own}; "
                                      "reduce of the subtree roots' fronts, reduce of their update vectors, broadcast of the separators' solution"},
            "roofline": None, "cpu_baseline": None}, f"grid_n{world}", detail=args.full)
    if dist is not None:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default="control07",
                    help="control07 (default: examples/control07.mat, BASELINE configs[1]) | control07_like (synthetic, same shape) | "
                         "control07_init / arch0[_init] / nb[_init] (the reference examples at the golden scalings) | nb_like (configs[2] shape) | lpdense (configs[2] dense-column variant) | maxcut<n> (configs[3]) | blockdiag[:nblk:n:mper] (configs[4]) | "
                         "grid[:n] (factor + solves of a matrix with separators, subtrees sharded over the ranks)")
    ap.add_argument("--shard", default="auto", choices=["auto", "replicas", "columns", "blocks", "blockcyclic"],
                    help="N>1, ONE unit per step: blocks = PSD blocks dealt to the ranks, partial ADA' + one RCCL all-reduce (auto when "
                         "the problem has at least N PSD blocks); columns = ADA' column panels per rank + RCCL all-gather (auto otherwise); "
                         "factor/solves replicated in both (one dense supernode does not shard); replicas = independent units per "
                         "rank (weak scaling, no collective); blockcyclic = columns for ADA' + ONE dense front factored block-column-cyclically "
                         "(sedumi_amd.dist.BlockCyclicFactor: a broadcast per 64-column panel), solves replicated")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: per-kernel roofline and phases, the PCIe- and MEX-inclusive tiers, "
                         "the iteration-weighted whole-solve figure, the CPU baseline of the reference; writes the detail file")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float64, at most 64 MB in all: a fixed "
                         "sample of the entries of the larger arrays beyond that)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--other-configs", action="store_true",
                    help="(implies --full) also measure the other BASELINE configs (both scalings of the reference examples, maxcut4000, blockdiag, the "
                         "maxcut8000 solve leg), the OpenBLAS-linked CPU baseline and the lazy MEX tiers: minutes, all of it into the detail file only")
    ap.add_argument("--no-other-configs", action="store_true", help="(accepted for older command lines; other configs are off unless --other-configs)")
    ap.add_argument("--graph", action="store_true", help="replay the step from a captured hipGraph (one launch per step)")
    ap.add_argument("--dry-run", action="store_true", help="launcher / process-group / line plumbing only, on CPU; nothing is measured")
    ap.add_argument("--tag", default=None, help="suffix of profiles/bench_detail_<workload>_n<N>[_<tag>].json")
    args = ap.parse_args()
    args.full = args.full or args.other_configs

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(relaunch(args))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.dry_run:
        return dry_run(args, rank, world)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (there is no CPU fallback)")
    # BENCH_SHARE_GPU=1 (smoke tests on a 1-GPU box only): all ranks use device 0 and the process group runs on gloo
    share = os.environ.get("BENCH_SHARE_GPU") == "1"
    if share:
        local_rank = 0
    dist = None
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist
        if share:
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
    coll_dev = torch.device("cpu") if share else torch.device("cuda", local_rank)

    if args.workload == "lpdense":
        return bench_lpdense(args, local_rank)
    if args.workload.startswith("blockdiag") and (world > 1 or args.shard != "auto"):
        return bench_subtrees(args, rank, local_rank, world, torch, dist, coll_dev)
    if args.workload.startswith("grid"):
        return bench_separator(args, rank, local_rank, world, torch, dist, coll_dev)
    P, L, ADA, Q, d, ud, rhs, qpr, data_note = build_workload(args.workload, seed=0 if (world == 1 or args.shard != "replicas") else rank)
    nblk = int(np.asarray(P.K["s"]).size)
    shard = "none" if world == 1 else args.shard
    if shard == "auto":                                 # the way the workload shards
        shard = "blocks" if nblk >= world else "columns"
    shard_cols = shard in ("columns", "blocks", "blockcyclic")         # ONE unit per step, strong scaling
    cs = bs = bc = None
    if shard == "blocks":
        from sedumi_amd import dist as sd
        bs = sd.BlockShardedAda(P, L, ADA, device_index=local_rank, device=coll_dev)
        bs.upload_scaling(d, ud, qpr)
        plan = bs.plan
        plan.upload("rhs", rhs)
    else:
        plan = make_plan(local_rank, P, L, ADA, Q, d, ud, rhs, qpr, one_launch_fronts=shard != "blockcyclic")
    plan._xsuper = np.asarray(L["xsuper"]).ravel().astype(np.int64)
    if shard in ("columns", "blockcyclic"):
        from sedumi_amd import dist as sd
        cs = sd.ColumnShardedAda(plan, device=coll_dev)
    if shard == "blockcyclic":
        bc = sd.BlockCyclicFactor(L, ADA, device_index=local_rank, device=coll_dev, plan=plan)

    def step():
        if cs is not None:
            cs.getada()
        elif bs is not None:
            bs.getada()
        else:
            plan.getada()
        if bc is not None:
            bc.factor_resident(PARS, True)
        else:
            plan.blkchol(PARS, True)
        for _ in range(NSOLVE):
            plan.ldlsolve()

    eager_step = step
    if args.graph and cs is None and bs is None:
        for _ in range(2):
            eager_step()                       # first-use work (function attributes, allocations) outside the capture
        plan.sync()
        gid = plan.graph_capture(eager_step)

        def step():                            # noqa: F811
            plan.graph_launch(gid)

    def barrier():
        plan.sync()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    plan.sync()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        dist.barrier()
        t = torch.tensor([elapsed], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, plan_outputs(plan))

    if not args.full:
        roof, phases = None, None
    elif bc is not None:                                 # (the per-kernel profile re-runs the unit on this plan alone: not with a front spread over ranks)
        roof, phases = None, {"factor": {"frac_of_fp64_matrix_peak": None}, "solve": {"frac_of_hbm_peak": None}}
    else:
        roof, phases = profile_unit(plan, P, ud, min(max(args.steps, 20), 50))

    if rank == 0:
        base = base_blas = pcie = mexleg = weighted = None
        others = []
        headline = args.workload == "control07" and world == 1
        if world == 1 and args.full:
            pcie = pcie_inclusive(plan, P, d, ud, rhs, min(args.steps, 20))
            plan.upload("rhs", rhs); plan.ldlsolve()
            mexleg = mex_inclusive(P, L, ADA, Q, d, ud, rhs, qpr, min(args.steps, 30), plan.download("y"))
            if headline:
                # a WHOLE solve of control07.mat (41 factorisations, profiles/r04_control07_whole_solve_growth_by_iteration.txt): the explicit inverse of
                # the solves' super-block stays within the growth bound for the first 35 iterations and is beyond it for the last 6 (inverse +
                # refinement): `value` is the first regime; this is the iteration-weighted figure from the two units measured in this run
                beyond = measure_config("control07", local_rank, 100, 5, 20, 0, growth_max=0.0)
                others.append(beyond)
                if "ms_per_step" in beyond:
                    n_in, n_out = 35, 6
                    ms_w = (n_in * 1e3 * elapsed / args.steps + n_out * beyond["ms_per_step"]) / (n_in + n_out)
                    weighted = {"value": 1e3 / ms_w, "unit": "IPM iters/s", "ms_per_step": ms_w, "iterations_within_growth_bound": n_in, "iterations_beyond": n_out,
                                "ms_per_step_within": 1e3 * elapsed / args.steps, "ms_per_step_beyond": beyond["ms_per_step"],
                                "source": "regimes per iteration from profiles/r04_control07_whole_solve_growth_by_iteration.txt (tools/driver_log.py on the GPU box)"}
            if not args.no_cpu_baseline:
                base = cpu_baseline(P, d, ud, rhs, budget_s=10.0)
            if args.other_configs:
                others.append({"workload": args.workload + " (mex_inclusive at lazy level 0: every gateway returns the reference's arrays)",
                               "mex_inclusive": mex_inclusive(P, L, ADA, Q, d, ud, rhs, qpr, min(args.steps, 30), None, lazy=0)})
                if not args.no_cpu_baseline:
                    try:
                        from oracle import refmex
                        ob = refmex.find_openblas()
                    except Exception:
                        ob = None
                    if ob:
                        base_blas = cpu_baseline(P, d, ud, rhs, budget_s=8.0, blas=ob)
                # the second scaling of the headline config (identity scaling of iteration 1 next to an ill-conditioned one),
                # the other reference examples at both scalings, then the synthetic configs[3], [4]
                nocpu = args.no_cpu_baseline
                for nm, st, wu, npf, mxu, cpu in (("control07_init", 100, 5, 20, 0, 0), ("arch0", 100, 5, 20, 5, 20), ("arch0_init", 100, 5, 20, 0, 0), ("nb", 100, 5, 20, 0, 20),
                                                  ("nb_init", 100, 5, 20, 0, 0), ("maxcut4000", 10, 2, 5, 2, 1), ("blockdiag", 20, 3, 10, 2, 3)):
                    if nm != args.workload:
                        others.append(measure_config(nm, local_rank, st, wu, npf, mxu, cpu_units=0 if nocpu else cpu))
                others.append(whole_solve_leg("control07", with_reference=not nocpu))
                others.append(solve_leg("maxcut4000", local_rank))
                others.append(solve_leg("maxcut8000", local_rank))
                if headline:
                    others.append(measure_config("control07", local_rank, 30, 3, 10, 0, growth_max=0.0, refine=0))
        mult = 1 if (shard_cols or world == 1) else world
        out = {
            "metric": "IPM iters/sec (ADA' form+factor+solve)", "value": mult * args.steps / elapsed, "unit": "IPM iters/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True, "scaling": "strong" if shard_cols else "weak", "vs_baseline": None, "dtype": "f64",
            "data": data_note,
            "config": {"workload": f"{P.name}: {CONFIG_NOTE.get(args.workload[:6], 'synthetic')}, m={P.m}, nnz(At)={P.At.nnz}, "
                                   f"nnz(ADA')={plan.nnzADA}, nnz(L)={plan.nnzL}; unit = getada1+2+3, blkchol, {NSOLVE}x(fwblkslv,./d,bwblkslv)",
                       "parallelism": ({"columns": "ADA' column panels per rank + RCCL all-gather, factor/solves replicated (they do not shard: one dense supernode)",
                                         "blocks": "PSD blocks dealt to the ranks, partial ADA' + RCCL all-reduce, factor/solves replicated",
                                         "blockcyclic": "ADA' column panels + all-gather; the ONE dense front factored block-column-cyclically (64-column panels, a broadcast per panel); solves replicated",
                                         "replicas": "replicas: independent units per rank, no collective"}[shard] if world > 1 else "single GPU")},
            "roofline": roof, "phases_ms_per_step": phases, "cpu_baseline": base, "cpu_baseline_blas": base_blas,
            "pcie_inclusive": pcie, "mex_inclusive": mexleg, "whole_solve_weighted": weighted, "other_configs": others,
        }
        if base and base.get("value") and mexleg and mexleg.get("value"):
            out["mex_inclusive_speedup_vs_cpu_reference"] = mexleg["value"] / base["value"]
        if base and base.get("value"):
            out["speedup_vs_cpu_reference"] = out["value"] / mult / base["value"]
        if base_blas and base_blas.get("value"):
            out["speedup_vs_cpu_reference_blas"] = out["value"] / mult / base_blas["value"]
        extras = {"speedup_vs_cpu_reference": out.get("speedup_vs_cpu_reference"),
                  "mex_inclusive_value": mexleg.get("value") if isinstance(mexleg, dict) else None,
                  "whole_solve_weighted_value": weighted and weighted["value"],
                  "factor_frac_of_fp64_matrix_peak": phases["factor"]["frac_of_fp64_matrix_peak"],
                  "solves_frac_of_hbm_peak": phases["solve"]["frac_of_hbm_peak"]} if args.full else None
        emit(out, f"{args.workload}_n{world}" + (f"_{args.tag}" if args.tag else ""), extras, detail=args.full)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
