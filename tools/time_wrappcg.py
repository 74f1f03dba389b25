"""Time sdm_plan_wrappcg against the host-orchestrated wrapPcg of sedumi_amd.driver (one GPU command, warmed up).

  per call     every wrapPcg call of a control07 and an arch0 solve: Sedumi.wrapPcg (the host loop around the device operators) and
               plan.wrappcg on the same plan state and inputs, alternated, each once per call
  whole solve  control07 with PlanHot(device_pcg=False) and (device_pcg=True), alternated, --solves each

    python tools/time_wrappcg.py [--solves 5] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def per_call(name):
    import test_driver as td
    from sedumi_amd.driver import loop as lp
    host, dev, ks = [], [], []

    class Timed(lp.Sedumi):
        def wrapPcg(self, L, d, DAt, rb, rv, cgpars, y0):
            pl = self.hot.plan
            if self.cone.nq:
                pl.upload("qauxdet", d["auxdet"]); pl.upload("qauxtr", d["auxtr"])
            t0 = time.perf_counter()
            out = lp.Sedumi.wrapPcg(self, L, d, DAt, rb, rv, cgpars, y0)
            t1 = time.perf_counter()
            o = pl.wrappcg(rv, rb, y0, cgpars, bool(np.size(d["perm"])))
            t2 = time.perf_counter()
            host.append(t1 - t0); dev.append(t2 - t1); ks.append((out[2], o[2]))
            return out

    At, K, g = td.problem(name)
    Timed(At, g["b"], g["c"], K, hot=lp.PlanHot(), internal=True).solve()
    return np.array(host), np.array(dev), ks


def whole(name, device_pcg):
    import test_driver as td
    from sedumi_amd.driver import loop as lp
    At, K, g = td.problem(name)
    S = lp.Sedumi(At, g["b"], g["c"], K, hot=lp.PlanHot(device_pcg=device_pcg), internal=True)
    t0 = time.perf_counter()
    r = S.solve()
    return time.perf_counter() - t0, r["iter"]


def q(a):
    return "median %.3f ms  min %.3f  max %.3f  (n = %d)" % (1e3 * np.median(a), 1e3 * a.min(), 1e3 * a.max(), a.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import helpers
    helpers.use_hip()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    whole("nb", True)                                                      # warm-up: library load, code objects, first allocations
    for name in ("control07", "arch0"):
        h, d, ks = per_call(name)
        same = sum(1 for a_, b_ in ks if a_ == b_)
        say(f"per call {name}: {len(ks)} wrapPcg calls, CG steps host {sum(a_ for a_, _ in ks)} device {sum(b_ for _, b_ in ks)}, same k on {same}")
        say(f"  host loop   {q(h)}")
        say(f"  wrappcg     {q(d)}")
        say(f"  ratio of medians host / device {np.median(h) / np.median(d):.2f}; per CG step host {1e3 * h.sum() / max(1, sum(a_ for a_, _ in ks)):.3f} ms, "
            f"device {1e3 * d.sum() / max(1, sum(b_ for _, b_ in ks)):.3f} ms")
    off, on = [], []
    for i in range(a.solves):
        off.append(whole("control07", False)); on.append(whole("control07", True))
    say(f"whole solve control07, alternated: device_pcg off {q(np.array([t for t, _ in off]))} iterations {[it for _, it in off]}")
    say(f"whole solve control07, alternated: device_pcg on  {q(np.array([t for t, _ in on]))} iterations {[it for _, it in on]}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
