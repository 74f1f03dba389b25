"""tools/kernel_digests.py [library] -- one line per gfx950 function of libsedumi_hip.so: sha256 of its machine code and, for kernels, the
resource numbers of the code object's metadata.  Two builds whose lines are equal run the same device code: what a change that only moves
source text has to show (`diff` of the two outputs).
The text that is hashed is llvm-objdump's disassembly of the function with the instruction encodings, without addresses: symbol order
inside a code object and absolute addresses do not enter.  Branches are pc-relative, so their encodings do not move with the function;
the one thing that does is the distance to a called function (s_getpc_b64 + s_add_u32 / s_addc_u32 with a literal): those two literals
are replaced by the name of the function at the address they add up to.  The padding between two functions is left out."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import code_objects as co  # noqa: E402

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size",
        "vgpr_spill_count", "sgpr_spill_count", "max_flat_workgroup_size", "wavefront_size")


def functions(obj):
    """{symbol: [(address, encoding words, text)]} of one code object (bytes)"""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(obj)
        f.flush()
        dis = subprocess.run([OBJDUMP, "-d", f.name], capture_output=True, text=True, check=True).stdout
    res, cur = {}, None
    for line in dis.split("\n"):
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", line)
        if m:
            cur = res.setdefault(m.group(2), [])
            continue
        m = re.match(r"^\s+(.*?)\s*// ([0-9A-F]+): ((?:[0-9A-F]{8} ?)+)", line)
        if m and cur is not None:
            cur.append((int(m.group(2), 16), m.group(3).split(), re.sub(r"\s+", " ", m.group(1))))
    return res


def normalised(fns):
    """per symbol the text to hash: `encoding  instruction` lines; the literals of a pc-relative address computation become the target's name"""
    start = {insns[0][0]: name for name, insns in fns.items() if insns}
    out = {}
    for name, insns in fns.items():
        lines = []
        for i, (addr, enc, text) in enumerate(insns):
            if text.startswith("s_getpc_b64") and i + 2 < len(insns) and insns[i + 1][2].startswith("s_add_u32") and insns[i + 2][2].startswith("s_addc_u32") \
                    and len(insns[i + 1][1]) == 2 and len(insns[i + 2][1]) == 2:
                lo, hi = int(insns[i + 1][1][1], 16), int(insns[i + 2][1][1], 16)
                rel = (hi << 32 | lo)
                rel -= (1 << 64) if rel >> 63 else 0
                target = insns[i + 1][0] + rel                      # s_getpc_b64 yields the address of the instruction behind it
                tname = start.get(target, "data+?")
                insns[i + 1] = (insns[i + 1][0], [insns[i + 1][1][0], "<lo>"], re.sub(r"0x[0-9a-f]+$", tname + "@lo", insns[i + 1][2]))
                insns[i + 2] = (insns[i + 2][0], [insns[i + 2][1][0], "<hi>"], re.sub(r"(0x[0-9a-f]+|-?\d+)$", tname + "@hi", insns[i + 2][2]))
            addr, enc, text = insns[i]
            lines.append(" ".join(enc) + "  " + re.sub(r"\s*<[^>]*>$", "", text))
        while lines and lines[-1].split("  ")[1] in ("s_nop 0", "s_code_end"):   # alignment padding in front of the next symbol
            lines.pop()
        out[name] = "\n".join(lines)
    return out


def digests(lib):
    meta = {}
    for obj in co.code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(obj)
            f.flush()
            notes = subprocess.run([co.READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
        for blk in re.split(r"\n\s*- \.agpr_count", "\n" + notes)[1:]:
            blk = "  - .agpr_count" + blk
            name = re.search(r"\.name:\s+(\S+)", blk)
            if name:
                meta[name.group(1)] = " ".join("%s=%s" % (k, (re.search(r"\.%s:\s+(\d+)" % k, blk) or [None, "-"])[1]) for k in META)
    rows = {}
    for obj in co.code_objects(lib):
        for name, text in normalised(functions(obj)).items():
            n = text.count("\n") + 1 if text else 0
            rows.setdefault(name, []).append("%s %6d insns  %s" % (hashlib.sha256(text.encode()).hexdigest()[:32], n, meta.get(name, "(device function)")))
    return rows


if __name__ == "__main__":
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(co.ROOT, "sedumi_amd", "lib", "libsedumi_hip.so")
    rows = digests(lib)
    for name, dn in sorted(zip(rows, co.demangle(list(rows))), key=lambda t: t[1]):
        for r in sorted(rows[name]):                              # (an inline function can be in several code objects)
            print("%-60s %s" % (dn.split("(")[0][-60:], r))
