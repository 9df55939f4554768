#!/usr/bin/env python3
"""Do the angiography and repeat registration kernels of the working tree compile to the code of another revision?

Compiles angiogram_inst.hip and repeat_register_inst.hip of octproz_amd/csrc to gfx950 assembly (the flags of
tests/test_angiogram.py::test_angio_kernels_need_no_scratch), once from `git archive REV` and once from the working tree, and compares
every kernel symbol:

  identical                  the instruction streams are equal (comments and the numbers of local labels stripped)
  same opcodes, reordered    the opcode multisets are equal, and so are NumVgprs, TotalNumSgprs, ScratchSize and LDSByteSize
  DIFFERENT                  neither

Only opcodes and the resource lines are read.  Needs no GPU.  Exit status 1 if the symbol sets differ or any kernel is DIFFERENT.

    python scripts/angio_kernel_diff.py --rev HEAD --out profiles/angio_refactor_kernel_diff.txt
"""
import argparse
import collections
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "octproz_amd/csrc"
FILES = ("angiogram_inst.hip", "repeat_register_inst.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "-Wno-pass-failed", "-Wno-unused-value", "-S", "--cuda-device-only"]
RESOURCES = ("NumVgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize")
EXPECTED = 7 * (3 + 6 + 6) * 2 + 2


def compile_kernels(hipcc, csrc, tmp, tag):
    """{symbol: (instruction stream, {resource: value})} of both instance files"""
    kernels = {}
    for f in FILES:
        out = os.path.join(tmp, "%s_%s.s" % (tag, f))
        subprocess.check_call([hipcc] + FLAGS + ["-o", out, f], cwd=csrc, stderr=subprocess.DEVNULL)
        text = open(out).read()
        for name in re.findall(r"^(_ZN3oct\w+_kernel\w+):", text, re.M):
            body = text[text.index("\n" + name + ":") + 1:]
            meta = {k: int(re.search(r"; %s: (\d+)" % k, body).group(1)) for k in RESOURCES}
            stream = []
            for line in body[:body.index(".Lfunc_end")].split("\n")[1:]:
                line = line.split(";")[0].strip()
                if not line or line.startswith(".") or line.endswith(":"):
                    continue
                stream.append(re.sub(r"\.LBB\d+_\d+", ".L", re.sub(r"\s+", " ", line)))
            kernels[name] = (stream, meta)
    return kernels


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rev", default="HEAD", help="the revision the working tree is compared with")
    ap.add_argument("--hipcc", default="/opt/rocm/bin/hipcc")
    ap.add_argument("--out", help="write the per-kernel table here as well")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.check_output(["git", "archive", args.rev, CSRC, "include"], cwd=ROOT)
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(os.path.join(tmp, "old"))
        old = compile_kernels(args.hipcc, os.path.join(tmp, "old", CSRC), tmp, "old")
        new = compile_kernels(args.hipcc, os.path.join(ROOT, CSRC), tmp, "new")
    lines, tally = [], collections.Counter()
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            verdict = "MISSING in the %s tree" % ("old" if name not in old else "new")
        else:
            (so, mo), (sn, mn) = old[name], new[name]
            ops = lambda s: collections.Counter(x.split(" ")[0] for x in s)
            if so == sn:
                verdict = "identical"
            elif ops(so) == ops(sn) and mo == mn:
                verdict = "same opcodes, reordered"
            else:
                verdict = "DIFFERENT (instructions %d -> %d; %s)" % (
                    len(so), len(sn), ", ".join("%s %d -> %d" % (k, mo[k], mn[k]) for k in RESOURCES if mo[k] != mn[k]) or "resources equal")
        tally[verdict.split(" (")[0]] += 1
        lines.append("%-28s %s" % (verdict, name))
    head = ["# scripts/angio_kernel_diff.py --rev %s: %d kernels in the old tree, %d in the new one (%d expected)" % (args.rev, len(old), len(new), EXPECTED)]
    head += ["# %4d %s" % (n, v) for v, n in sorted(tally.items())]
    text = "\n".join(head + lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        open(args.out, "w").write(text)
    ok = set(old) == set(new) and len(new) == EXPECTED and set(tally) <= {"identical", "same opcodes, reordered"}
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
