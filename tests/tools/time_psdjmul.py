"""SURVEY 8f N11 timing: psdjmul and the two fused calls through the host-pointer C ABI (transfers and synchronises included):
    psdjmul   host code of the driver without device_jmul (Cone.psdjmul of sedumi_amd/driver/loop.py: a product per block)  /  sdm_psdjmul
    maxstep   sdm_psdinvscale + sdm_minpsdeig (two calls)  /  sdm_maxstep_psd (one call)
    wstruct   sdm_trydif_psd + sdm_psdeig, values only (two calls)  /  sdm_wstruct_psd (one call)
alternating the variants in one process, medians and quartiles of each, and that each one call is bit-equal to its two.  One case per invocation,
ended by its own alarm, nothing is tried twice.  Run on the GPU box:
    python tests/tools/time_psdjmul.py CASE [--out FILE] [--limit SECONDS]
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
    K, x, z, g = c["K"], c["x"], c["z"], c["g"]
    cn = lp.Cone(None, K)                                            # (ref = None: no device switch, the host code)
    nt = (max(CASES[name]["s"]) + 63) // 64
    ud = mex.psdfactor(x, K).ravel()
    variants = {
        "psdjmul host": lambda: cn.psdjmul(g, z), "psdjmul device": lambda: mex.psdjmul(g, z, K),
        "maxstep two calls": lambda: mex.minpsdeig(mex.psdinvscale(ud, g, K), K, nlhs=2), "maxstep one call": lambda: mex.maxstep_psd(ud, g, K, nlhs=2),
        "wstruct two calls": lambda: mex.psdeig(mex.trydif_psd(x, z, K)[1], K), "wstruct one call": lambda: mex.wstruct_psd(x, z, K),
    }
    m2, m1 = variants["maxstep two calls"](), variants["maxstep one call"]()
    sw_m = mex.psdeig_last_sweeps()
    t2, w1 = mex.trydif_psd(x, z, K), variants["wstruct one call"]()
    sw_w = mex.psdeig_last_sweeps()
    same = (np.array_equal(m2[0], m1[0]) and m2[1] == m1[1] and np.array_equal(t2[0], w1[0]) and np.array_equal(t2[1], w1[1])
            and np.array_equal(mex.psdeig(t2[1], K), w1[2]) and t2[2] is w1[3])
    hz, dz = cn.psdjmul(g, z), mex.psdjmul(g, z, K).ravel()
    close = float(np.max(np.abs(hz - dz)) / np.max(np.abs(hz)))
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
    line = "%-10s lenud %9d  nt %2d  psdjmul: 1 launch of %d tiles;  sweeps: maxstep %d, wstruct %d\n" % (
        name, x.size, nt, len(CASES[name]["s"]) * nt * (nt + 1) // 2, sw_m, sw_w)
    for k, v in t.items():
        line += "    %-20s median %9.3f ms (quartiles %9.3f .. %9.3f)\n" % (k, med[k], q(v, 25), q(v, 75))
    line += ("    psdjmul host / device %5.2f;   maxstep two calls / one call %5.2f;   wstruct two calls / one call %5.2f;   one call bit-equal to the two: %s;"
             "   max |z - host z| / max |z| %.1e"
             % (med["psdjmul host"] / med["psdjmul device"], med["maxstep two calls"] / med["maxstep one call"],
                med["wstruct two calls"] / med["wstruct one call"], same, close))
    print(line, flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
            f.write(line + "\n")
    assert same


if __name__ == "__main__":
    main()
