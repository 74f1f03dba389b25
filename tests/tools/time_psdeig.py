"""SURVEY 8f N10 timing: psdeig (values only, and with eigenvectors) and minpsdeig through the host-pointer C ABI (transfers and the synchronise
after every sweep included) against the host code the driver runs without device_eig (Cone.psdeig, Cone.minpsdeig of sedumi_amd/driver/loop.py:
LAPACK's eigvalsh / eigh per block):
    psdeig values   host  /  sdm_psdeig(q = NULL)
    psdeig vectors  host  /  sdm_psdeig
    minpsdeig       host  /  sdm_minpsdeig
alternating the variants in one process, medians and quartiles of each, the sweeps made and the launches they took.  One case per invocation, ended
by its own alarm, nothing is tried twice.  Run on the GPU box:
    python tests/tools/time_psdeig.py CASE [--out FILE] [--limit SECONDS]
Cases: control07 (70, 35), 64x200 (64 blocks of order 200), 1000 (one block of order 1000).  The blocks are X = Q diag(lambda) Q' / 2 with lambda
drawn from [1, 2], formed in double."""
import os, signal, sys, time
import numpy as np
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from sedumi_amd import capi, mex
from sedumi_amd.driver import loop as lp
import psd_frames_exact as pfe
import psdeig_exact as pe

CASES = {"64x200": dict(s=[200] * 64), "control07": dict(s=[70, 35]), "1000": dict(s=[1000])}


def main():
    name = sys.argv[1]
    limit = int(sys.argv[sys.argv.index("--limit") + 1]) if "--limit" in sys.argv else 240
    signal.alarm(limit)                                              # a hang ends the process; nothing is started after it
    assert capi.backend() == "hip-gfx950" and capi.device_count() >= 1, "a timing needs the device"
    K = pe.make_K(CASES[name])
    rng = np.random.default_rng(1)
    xs = []
    for n, herm in pfe.block_list(K):
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        xs.append((Q * rng.uniform(1.0, 2.0, n)) @ Q.T / 2)
    x = pfe.pack_blocks(xs, K)
    cn = lp.Cone(None, K)                                            # (ref = None: no device_eig, the host code)
    variants = {
        "psdeig values host": lambda: cn.psdeig(x), "psdeig values device": lambda: mex.psdeig(x, K),
        "psdeig vectors host": lambda: cn.psdeig(x, want_q=True), "psdeig vectors device": lambda: mex.psdeig(x, K, nlhs=2),
        "minpsdeig host": lambda: cn.minpsdeig(x), "minpsdeig device": lambda: mex.minpsdeig(x, K),
    }
    lab, q, info = mex.psdeig(x, K, nlhs=3)
    sweeps = mex.psdeig_last_sweeps()
    same = np.array_equal(mex.psdeig(x, K), lab) and mex.minpsdeig(x, K)[0, 0] == lab.min()
    hl = cn.psdeig(x)
    close = float(np.max(np.abs(hl - lab.ravel())) / np.max(np.abs(hl)))
    ncb = [(n + 31) // 32 for n, _ in pfe.block_list(K)]
    steps = max(m + (m & 1) - 1 for m in ncb)
    reps, warm = (5, 1) if x.size > 500000 else (30, 5)
    for _ in range(warm):
        for f in variants.values():
            f()
    t = {k: [] for k in variants}
    for _ in range(reps):                                            # alternating: all see the same neighbours on the host and the device
        for k, f in variants.items():
            t0 = time.perf_counter(); f(); t[k].append(1e3 * (time.perf_counter() - t0))
    qt = lambda v, p: float(np.percentile(v, p))
    med = {k: qt(v, 50) for k, v in t.items()}
    line = ("%-10s lenud %9d  column blocks %d  steps per sweep %d  sweeps %d (one synchronise each)  launches at most %d = sweeps (3 steps + 1) + 6   info %d\n"
            % (name, x.size, max(ncb), steps, sweeps, sweeps * (3 * steps + 1) + 6, info))
    for k, v in t.items():
        line += "    %-24s median %9.3f ms (quartiles %9.3f .. %9.3f)\n" % (k, med[k], qt(v, 25), qt(v, 75))
    line += ("    host / device: psdeig values %5.2f   psdeig vectors %5.2f   minpsdeig %5.2f;   values-only and minimum bit-equal: %s;"
             "   max |lab - host lab| / max |lab| %.1e"
             % (med["psdeig values host"] / med["psdeig values device"], med["psdeig vectors host"] / med["psdeig vectors device"],
                med["minpsdeig host"] / med["minpsdeig device"], same, close))
    print(line, flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
            f.write(line + "\n")
    assert same and info == -1


if __name__ == "__main__":
    main()
