#!/usr/bin/env python3
"""Per-kernel resource table of two builds, from the compiler's own report.

    make -C localization_amd/csrc CXXFLAGS="-O3 -fPIC -std=c++17 -Rpass-analysis=kernel-resource-usage" 2> build.log
    tools/dev/kernel_resources.py parent.log change.log [PARENT_CSRC CHANGE_CSRC] > profiles/edge_terms/kernel_resources.txt

One row per kernel instantiation: VGPRs, AGPRs, scratch bytes per lane, LDS bytes per block and occupancy must be EQUAL (a row that differs
is marked DIFF and the exit status is 1); SGPRs and spill counts are reported as parent -> change.  With the two build directories: per
translation unit, the instruction count of its gfx950 code object (llvm-objdump -d), and whether the disassembly is identical once symbol
names and addresses are removed.
"""
import glob
import os
import tempfile
import re
import subprocess
import sys

HELD = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
REPORTED = ("TotalSGPRs", "SGPRs Spill", "VGPRs Spill")


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = out.setdefault((line.split(":", 1)[0], val), {})
        elif cur is not None:
            cur[key] = val
    return out


def demangle(names):
    try:
        txt = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return [t.replace("locamd::(anonymous namespace)::", "").split("(")[0].replace("void ", "") for t in txt]
    except (OSError, subprocess.CalledProcessError):
        return list(names)


OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/llvm/bin/llvm-objdump")


def disassembly(obj, tmp):
    """the device code of a .hip.o: its instructions, symbol names and addresses removed"""
    work = os.path.join(tmp, os.path.basename(obj))
    with open(obj, "rb") as f, open(work, "wb") as g:
        g.write(f.read())
    subprocess.run([OBJDUMP, "--offloading", work], capture_output=True, check=True)   # (writes the code object next to its input)
    co = glob.glob(work + ".*gfx950")[0]
    txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    return [re.sub(r"<[^>]*>", "", l).split("//")[0].strip() for l in txt.splitlines() if re.match(r"\s+[a-z]\w+", l)]


def code_objects(parent_dir, change_dir):
    print("\ntranslation unit                     instructions parent -> change   disassembly")
    for obj in sorted(glob.glob(os.path.join(change_dir, "*.hip.o"))):
        with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
            a, b = disassembly(os.path.join(parent_dir, os.path.basename(obj)), ta), disassembly(obj, tb)
        print(f"{os.path.basename(obj)[:-2]:36s} {len(a):>12d} -> {len(b):<12d}    {'identical' if a == b else 'differs'}")


def main():
    parent, change = parse(sys.argv[1]), parse(sys.argv[2])
    keys = sorted(set(parent) | set(change))
    short = dict(zip(keys, demangle([k[1] for k in keys])))
    bad = 0
    print(f"{'file':34s} {'kernel':58s} " + " ".join(f"{h.split(' ')[0]:>8s}" for h in HELD) + "   " + "  ".join(f"{r:>12s}" for r in REPORTED))
    for k in keys:
        p, c = parent.get(k), change.get(k)
        if p is None or c is None:
            print(f"{k[0]:34s} {short[k]:58s} only in {'change' if p is None else 'parent'}   DIFF")
            bad += 1
            continue
        same = all(p.get(h) == c.get(h) for h in HELD)
        held = " ".join(f"{c.get(h, '?'):>8s}" if p.get(h) == c.get(h) else f"{p.get(h, '?') + '>' + c.get(h, '?'):>8s}" for h in HELD)
        rep = "  ".join(f"{p.get(r, '?') + ' -> ' + c.get(r, '?'):>12s}" for r in REPORTED)
        print(f"{k[0]:34s} {short[k]:58s} {held}   {rep}{'' if same else '   DIFF'}")
        bad += not same
    print(f"# {len(keys)} kernels, {bad} differ in a held column")
    if len(sys.argv) > 4:
        code_objects(sys.argv[3], sys.argv[4])
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
