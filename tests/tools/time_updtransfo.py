"""SURVEY 8f N8 timing: the PSD chain of updtransfo.m:99-108 through the host-pointer C ABI (transfers and synchronises included), two ways:
    A  as the driver ran it before N8: triumtriu on the host (numpy, full products of the two triangles), urotorder / givensrot / sqrtinv / qrK as
       four calls of the library, triumtriu on the host again
    B  one sdm_updtransfo_psd (explicit frames, as the driver asks for them)
alternating A and B in one process, medians and the spread of each, and that B's outputs equal A's device steps fed with the library's triumtriu.
One case per invocation, ended by its own alarm, nothing is tried twice.  Run on the GPU box:
    python tests/tools/time_updtransfo.py CASE [--out FILE] [--limit SECONDS]
Cases: 64x200 (64 blocks of order 200), control07 (70, 35), 1000 (one block of order 1000)."""
import os, signal, sys, time
import numpy as np
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from sedumi_amd import capi, mex
import psd_frames_exact as pfe
import triu_exact as te

CASES = {"64x200": dict(s=[200] * 64), "control07": dict(s=[70, 35]), "1000": dict(s=[1000])}
MAXU = 1.1


def host_triumtriu(x, y, K):
    """ConePart.triumtriu of sedumi_amd/driver/loop.py"""
    out = []
    for X, Y in zip(pfe.split_blocks(x, K), pfe.split_blocks(y, K)):
        ZZ = np.triu(X) @ np.triu(Y)
        out.append(ZZ + np.triu(ZZ, 1).conj().T)
    return pfe.pack_blocks(out, K)


def chain_a(c, first=host_triumtriu, last=host_triumtriu):
    K = c["K"]
    du = first(c["ux"], c["u"], K)
    du, perm, gjc, g = mex.urotorder(du, K, MAXU, c["perm"])
    q = mex.givensrot(gjc, g, c["q"], K)
    vinv = mex.sqrtinv(q, c["vlab"], K)
    frs, r = mex.qrK(vinv, K, nlhs=2, frame_kind=mex.FRAME_EXPLICIT)
    return last(np.asarray(r).ravel(), np.asarray(du).ravel(), K), perm, frs


def chain_b(c):
    return mex.updtransfo_psd(c["ux"], c["u"], c["perm"], c["q"], c["vlab"], c["K"], maxu=MAXU, frame_kind=mex.FRAME_EXPLICIT)


def main():
    name = sys.argv[1]
    limit = int(sys.argv[sys.argv.index("--limit") + 1]) if "--limit" in sys.argv else 240
    signal.alarm(limit)                                              # a hang ends the process; nothing is started after it
    assert capi.backend() == "hip-gfx950" and capi.device_count() >= 1, "a timing needs the device"
    c = te.make_chain(CASES[name])
    want = chain_a(c, mex.triumtriu, mex.triumtriu)
    got = chain_b(c)
    same = all(np.array_equal(np.asarray(a).ravel(), np.asarray(b).ravel()) for a, b in zip(got, want))
    reps, warm = (10, 2) if c["ux"].size > 500000 else (30, 5)
    for _ in range(warm):
        chain_a(c); chain_b(c)
    ta, tb = [], []
    for _ in range(reps):                                            # alternating: both see the same neighbours on the host and the device
        t0 = time.perf_counter(); chain_a(c); t1 = time.perf_counter(); chain_b(c); t2 = time.perf_counter()
        ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t2 - t1))
    t0 = time.perf_counter(); host_triumtriu(c["ux"], c["u"], c["K"]); th = 1e3 * (time.perf_counter() - t0)
    tt = []
    for _ in range(5):
        t0 = time.perf_counter(); mex.triumtriu(c["ux"], c["u"], c["K"]); tt.append(1e3 * (time.perf_counter() - t0))
    q = lambda v, p: float(np.percentile(v, p))
    line = ("%-10s lenud %9d  A host triumtriu + 4 gateways: median %9.3f ms (quartiles %9.3f .. %9.3f)   B one call: median %9.3f ms (%9.3f .. %9.3f)   "
            "A / B %5.2f   one host triumtriu %8.3f ms   sdm_triumtriu call %8.3f ms   B bit-equal to the single calls: %s"
            % (name, c["ux"].size, q(ta, 50), q(ta, 25), q(ta, 75), q(tb, 50), q(tb, 25), q(tb, 75), q(ta, 50) / q(tb, 50), th, float(np.median(tt)), same))
    print(line, flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
            f.write(line + "\n")
    assert same


if __name__ == "__main__":
    main()
