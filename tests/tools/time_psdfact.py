"""SURVEY 8f N9 timing: psdfactor, psdinvscale and the psdfactor + psdscale of trydif.m:62-63 through the host-pointer C ABI (transfers and
synchronises included) against the host code the driver runs without device_fact (Cone.psdfactor, Cone.psdinvscale, Cone.psdscale of
sedumi_amd/driver/loop.py: LAPACK's Cholesky, two triangular solves, two products per block):
    psdfactor    host  /  sdm_psdfactor
    psdinvscale  host  /  sdm_psdinvscale
    trydif       host psdfactor + psdscale  /  sdm_psdfactor + sdm_psdscale (two calls)  /  sdm_trydif_psd (one call)
alternating the variants in one process, medians and quartiles of each, and that the one call is bit-equal to the two.  One case per invocation,
ended by its own alarm, nothing is tried twice.  Run on the GPU box:
    python tests/tools/time_psdfact.py CASE [--out FILE] [--limit SECONDS]
Cases: 64x200 (64 blocks of order 200), control07 (70, 35), 1000 (one block of order 1000)."""
import os, signal, sys, time
import numpy as np
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from sedumi_amd import capi, mex
from sedumi_amd.driver import loop as lp
import psdfact_exact as pe

CASES = {"64x200": dict(s=[200] * 64), "control07": dict(s=[70, 35]), "1000": dict(s=[1000])}


def main():
    name = sys.argv[1]
    limit = int(sys.argv[sys.argv.index("--limit") + 1]) if "--limit" in sys.argv else 240
    signal.alarm(limit)                                              # a hang ends the process; nothing is started after it
    assert capi.backend() == "hip-gfx950" and capi.device_count() >= 1, "a timing needs the device"
    c = pe.make_case(CASES[name], "flat")
    K, x, z = c["K"], c["x"], c["z"]
    cn = lp.Cone(None, K)                                            # (ref = None: no device_fact, the host code)
    nt = (max(CASES[name]["s"]) + 63) // 64
    ux = mex.psdfactor(x, K).ravel()
    variants = {
        "psdfactor host": lambda: cn.psdfactor(x), "psdfactor device": lambda: mex.psdfactor(x, K, nlhs=2),
        "psdinvscale host": lambda: cn.psdinvscale(ux, z), "psdinvscale device": lambda: mex.psdinvscale(ux, z, K),
        "trydif host": lambda: cn.psdscale(cn.psdfactor(x)[0], z), "trydif two calls": lambda: mex.psdscale_u(mex.psdfactor(x, K), z, K),
        "trydif one call": lambda: mex.trydif_psd(x, z, K),
    }
    two, one = mex.psdscale_u(mex.psdfactor(x, K), z, K), mex.trydif_psd(x, z, K)
    same = np.array_equal(two, one[1]) and np.array_equal(mex.psdfactor(x, K), one[0])
    hu = cn.psdfactor(x)[0]
    close = float(np.max(np.abs(hu - ux)) / np.max(np.abs(hu)))
    reps, warm = (10, 2) if x.size > 500000 else (30, 5)
    for _ in range(warm):
        for f in variants.values():
            f()
    t = {k: [] for k in variants}
    for _ in range(reps):                                            # alternating: all see the same neighbours on the host and the device
        for k, f in variants.items():
            t0 = time.perf_counter(); f(); t[k].append(1e3 * (time.perf_counter() - t0))
    q = lambda v, p: float(np.percentile(v, p))
    med = {k: q(v, 50) for k, v in t.items()}
    line = "%-10s lenud %9d  nt %2d  launches psdfactor %d (<= 3 nt), psdinvscale %d (2 nt)\n" % (name, x.size, nt, 2 * nt - 1, 2 * nt)
    for k, v in t.items():
        line += "    %-20s median %9.3f ms (quartiles %9.3f .. %9.3f)\n" % (k, med[k], q(v, 25), q(v, 75))
    line += ("    host / device: psdfactor %5.2f   psdinvscale %5.2f   trydif (one call) %5.2f;   two calls / one call %5.2f;   one call bit-equal to the two: %s;"
             "   max |ux - host ux| / max |ux| %.1e"
             % (med["psdfactor host"] / med["psdfactor device"], med["psdinvscale host"] / med["psdinvscale device"],
                med["trydif host"] / med["trydif one call"], med["trydif two calls"] / med["trydif one call"], same, close))
    print(line, flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
            f.write(line + "\n")
    assert same


if __name__ == "__main__":
    main()
