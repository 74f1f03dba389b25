"""SURVEY 8f N7 timing: urotorder, givensrot and sqrtinv through the host-pointer C ABI (transfers and the final synchronise included) next to the
compiled reference gateways on one core of the same host.  Run on the GPU box:
    python tests/tools/time_urot.py [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tests/tools/time_urot.py --kernels CASE     (per-kernel times: five calls of each, no reference)
Cases: control07 (70, 35), 64x200, 1000, herm130, 2000 (device only: the reference needs seconds per call).
Inputs: triu of standard normals (Hermitian: imaginary strict upper triangle), diagonal |.| + 0.5, maxu = 1.1 -- about 0.45 n^2 rotations per block;
givensrot takes the rotations urotorder produced and a full random x, sqrtinv the same x."""
import os, sys, time
import numpy as np
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from sedumi_amd import mex, problem
import psd_frames_exact as pfe
import urot_exact as ue

CASES = {"control07": dict(s=[70, 35]), "64x200": dict(s=[200] * 64), "1000": dict(s=[1000]), "herm130": dict(hs=[130]), "2000": dict(s=[2000])}
MAXU = 1.1


def inputs(kw, seed=1):
    K = problem.make_K(1, [], kw.get("s", []), hs=kw.get("hs", ()))
    rng = np.random.default_rng(seed)
    us, xs = [], []
    for n, herm in pfe.block_list(K):
        M = np.triu(rng.standard_normal((n, n)))
        if herm:
            M = M + 1j * np.triu(rng.standard_normal((n, n)), 1)
        M[np.diag_indices(n)] = np.abs(np.real(np.diagonal(M))) + 0.5
        us.append(M)
        xs.append(rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if herm else 0))
    slen = sum(n for n, _ in pfe.block_list(K))
    return K, pfe.pack_blocks(us, K), pfe.pack_blocks(xs, K), 10.0 ** rng.uniform(-3, 3, 1 + slen)


def median_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    if "--kernels" in sys.argv:
        K, u, x, v = inputs(CASES[sys.argv[sys.argv.index("--kernels") + 1]])
        for _ in range(5):
            _, _, gjc, g = mex.urotorder(u, K, MAXU)
            mex.givensrot(gjc, g, x, K)
            mex.sqrtinv(x, v, K)
        return
    from oracle.refmex import RefMex, REF_DIR
    ref = RefMex(REF_DIR)
    out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n"); out.flush()
    col = lambda a: np.asarray(a, dtype=np.float64).reshape(-1, 1)
    say("case        rotations | urotorder [ms]  reference [ms]  ratio | givensrot [ms]  reference [ms]  ratio | sqrtinv [ms]  reference [ms]  ratio | us per step of the longest block (urotorder, whole call)")
    for name, kw in CASES.items():
        K, u, x, v = inputs(kw)
        nmax = max(n for n, _ in pfe.block_list(K))
        _, _, gjc, g = mex.urotorder(u, K, MAXU)
        nrot = sum(int(b[1][-1]) for b in ue.split(np.zeros(gjc.size), gjc, g, K))
        reps = 5 if u.size > 500000 else 20
        tu = median_ms(lambda: mex.urotorder(u, K, MAXU), reps, 3 if reps == 20 else 1)       # (median of 20; of 5 from a million entries on)
        tg = median_ms(lambda: mex.givensrot(gjc, g, x, K), reps, 3 if reps == 20 else 1)
        ts = median_ms(lambda: mex.sqrtinv(x, v, K), 20, 3)
        if name != "2000":
            ru = median_ms(lambda: ref.call("urotorder", 4, col(u), K, MAXU), reps, 1)
            rg = median_ms(lambda: ref.call("givensrot", 1, col(gjc), col(g), col(x), K), reps, 1)
            rs = median_ms(lambda: ref.call("sqrtinv", 1, col(x), col(v), K), reps, 1)
        else:
            ru = rg = rs = float("nan")
        say("%-11s %9d | %14.3f  %14.3f  %5.2f | %14.3f  %14.3f  %5.2f | %12.3f  %14.3f  %5.2f | %8.2f" %
            (name, nrot, tu, ru, ru / tu, tg, rg, rg / tg, ts, rs, rs / ts, 1e3 * tu / max(nmax - 1, 1)))
    if out:
        out.close()


if __name__ == "__main__":
    main()
