"""SURVEY 8f N6 timing: qrK through the host-pointer C ABI (transfers and the final synchronise included), both frame kinds, next to the
compiled reference gateway on one core of the same host.  Run on the GPU box:
    python tests/tools/time_qrk.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tests/tools/time_qrk.py --kernels CASE     (per-kernel times: five calls, Householder kind, no reference)
Cases: control07 (70, 35), 64x200, 1000, herm130, 2000 (device only: the reference needs seconds per call)."""
import os, sys, time
import numpy as np
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from sedumi_amd import mex, problem
import psd_frames_exact as pfe

CASES = {"control07": dict(s=[70, 35]), "64x200": dict(s=[200] * 64), "1000": dict(s=[1000]), "herm130": dict(hs=[130]), "2000": dict(s=[2000])}


def inputs(kw, seed=1):
    K = problem.make_K(1, [], kw.get("s", []), hs=kw.get("hs", ()))
    rng = np.random.default_rng(seed)
    mats = [rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if herm else 0) for n, herm in pfe.block_list(K)]
    return K, pfe.pack_blocks(mats, K)


def median_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    if "--kernels" in sys.argv:
        K, x = inputs(CASES[sys.argv[sys.argv.index("--kernels") + 1]])
        for _ in range(5):
            mex.qrK(x, K, nlhs=2)
        return
    from oracle.refmex import RefMex, REF_DIR
    ref = RefMex(REF_DIR)
    out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n"); out.flush()
    say("case        reflectors  [q,r] Householder [ms]  q alone [ms]  [q,r] explicit Qb [ms]  reference [q,r] 1 core [ms]  ratio (Householder)  us per reflector of the longest block (whole call)")
    for name, kw in CASES.items():
        K, x = inputs(kw)
        nmax = max(n for n, _ in pfe.block_list(K))
        nref = sum(max(n - 1, 0) for n, _ in pfe.block_list(K))
        xc = x.reshape(-1, 1)
        t0 = median_ms(lambda: mex.qrK(x, K, nlhs=2), 20, 3)
        tq = median_ms(lambda: mex.qrK(x, K), 20, 3)
        t1 = median_ms(lambda: mex.qrK(x, K, nlhs=2, frame_kind=mex.FRAME_EXPLICIT), 20, 3)
        tr = median_ms(lambda: ref.call("qrK", 2, xc, K), 5 if x.size > 500000 else 20, 1) if name != "2000" else float("nan")
        say("%-11s %10d  %22.3f  %12.3f  %22.3f  %27.3f  %19.2f  %10.2f" % (name, nref, t0, tq, t1, tr, tr / t0, 1e3 * t0 / max(nmax - 1, 1)))
    if out:
        out.close()


if __name__ == "__main__":
    main()
