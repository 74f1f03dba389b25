"""SURVEY 8f N5 timing: psdframeit / psdinvjmul through the host-pointer C ABI (transfers, the frame expansion and the final synchronise
included) next to the compiled reference gateways on one core of the same host.  Run on the GPU box:
    python tests/tools/time_psd_frames.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tests/tools/time_psd_frames.py --kernels CASE     (per-kernel times: five calls, no reference)
Cases: control07 (70, 35), 64x200 (BASELINE configs[4]), 1000, herm130, maxcut2000 (device only: the reference needs ~15 s per call)."""
import os, sys, time
import numpy as np
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from sedumi_amd import mex, problem
from oracle.refmex import RefMex, REF_DIR
import psd_frames_exact as pfe

CASES = {"control07": dict(s=[70, 35]), "64x200": dict(s=[200] * 64), "1000": dict(s=[1000]), "herm130": dict(hs=[130]), "maxcut2000": dict(s=[2000])}
PEAK_TF = 78.6          # MI355X FP64 matrix peak, TF/s


def inputs(ref, kw, seed=1):
    K = problem.make_K(1, [], kw.get("s", []), hs=kw.get("hs", ()))
    rng = np.random.default_rng(seed)
    mats, ys = [], []
    for n, herm in pfe.block_list(K):
        mats.append(rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if herm else 0))
        Y = rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if herm else 0)
        ys.append(Y + Y.conj().T)
    x = pfe.pack_blocks(mats, K)
    t0 = time.perf_counter()
    frms = np.asarray(ref.call("qrK", 2, x.reshape(-1, 1), K)[0]).ravel()
    tq = time.perf_counter() - t0
    lab = 10.0 ** rng.uniform(-3, 3, sum(n for n, _ in pfe.block_list(K)))
    return K, frms, lab, pfe.pack_blocks(ys, K), tq


def median_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    ref = RefMex(REF_DIR)
    if "--kernels" in sys.argv:
        K, frms, lab, y, _ = inputs(ref, CASES[sys.argv[sys.argv.index("--kernels") + 1]])
        for _ in range(5):
            mex.psdframeit(lab, frms, K); mex.psdinvjmul(lab, frms, y, K)
        return
    out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n"); out.flush()
    say("case          op           device kind 0 [ms]  device kind 1 [ms]  reference 1 core [ms]  ratio (kind 0)  GEMM TF/s at kind-1 time (share of %.1f)" % PEAK_TF)
    for name, kw in CASES.items():
        K, frms, lab, y, tq = inputs(ref, kw)
        n3 = float(sum((4 if herm else 1) * n ** 3 for n, herm in pfe.block_list(K)))
        col = lambda v: np.asarray(v).reshape(-1, 1)
        with_ref = name != "maxcut2000"
        te = median_ms(lambda: mex.psdframe_explicit(frms, K), 20, 3)
        qb = mex.psdframe_explicit(frms, K).ravel()
        say("%-13s qrK (reference, once) %.1f ms ; psdframe_explicit %.3f ms = %.2f TF/s of its (4/3) n^3" % (name, 1e3 * tq, te, 4.0 / 3.0 * n3 / te / 1e9))
        for op, flops, dev, rf in (("psdframeit", 2 * n3, lambda f, k: mex.psdframeit(lab, f, K, frame_kind=k), lambda: ref.call("psdframeit", 1, col(lab), col(frms), K)),
                                   ("psdinvjmul", 8 * n3, lambda f, k: mex.psdinvjmul(lab, f, y, K, frame_kind=k), lambda: ref.call("psdinvjmul", 1, col(lab), col(frms), col(y), K))):
            t0 = median_ms(lambda: dev(frms, 0), 20, 3)
            t1 = median_ms(lambda: dev(qb, 1), 20, 3)
            tr = median_ms(rf, 5 if n3 > 1e8 else 20, 1) if with_ref else float("nan")
            tf = flops / t1 / 1e9
            say("%-13s %-12s %18.3f  %18.3f  %21.3f  %14.1f  %8.2f (%.1f%%, transfers included)" % (name, op, t0, t1, tr, tr / t0, tf, 100 * tf / PEAK_TF))
    if out:
        out.close()


if __name__ == "__main__":
    main()
