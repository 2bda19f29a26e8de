#!/usr/bin/env python3
"""Compare the device code of two `hipcc --cuda-device-only -S` outputs kernel by kernel.

    python scratch/isa_compare.py before.s after.s [--rename REGEX REPL] [--only REGEX] [--label TEXT]

For every kernel (a symbol with an .amdhsa_kernel descriptor) the lines between its label and its .Lfunc_end, and its .amdhsa_* block,
must be textually identical; .file / .ident / .loc directives are ignored, and so is the function ordinal in basic-block labels
(.LBB<function>_<block>: the function's position in the translation unit, which moves when other kernels are removed).  --rename rewrites symbol names in both files first (a removed
template parameter), --only restricts the kernels of `before` that are expected in `after`.  Prints one line per kernel; exit status 1
on any difference.
"""
import argparse
import re
import sys

SKIP = re.compile(r"^\s*\.(file|ident|loc|cfi_\w+)\b")
BLOCK = re.compile(r"BB\d+_(\d+)")
PAD = re.compile(r"\s+;")            # the comment column after a label depends on the label's length


def kernels(path, rename):
    text = open(path).read()
    if rename:
        text = re.sub(rename[0], rename[1], text)
    lines = text.split("\n")
    out = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        name = m.group(1)
        j = next(k for k in range(i, len(lines)) if lines[k].strip() == ".end_amdhsa_kernel")
        desc = [l.strip() for l in lines[i : j + 1]]
        b = next(k for k, l in enumerate(lines) if l.startswith(name + ":"))
        e = next(k for k in range(b, len(lines)) if lines[k].startswith(".Lfunc_end"))
        body = [PAD.sub(" ;", BLOCK.sub(r"BB_\1", l)) for l in lines[b:e] if not SKIP.match(l)]
        ninstr = sum(1 for l in body if re.match(r"\t[a-z]\w+", l) and not l.lstrip().startswith("."))
        info = {k: next((re.search(r"(\d+)", l.split(k)[1]).group(1) for l in lines[e : e + 40] if k in l), "?")
                for k in (" NumVgprs:", " NumAgprs:", " TotalNumSgprs:", " AccumOffset:", " ScratchSize:", " LDSByteSize:")}
        out[name] = (body, desc, ninstr, info)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--rename", nargs=2, metavar=("REGEX", "REPL"))
    ap.add_argument("--only", help="kernels of `before` expected in `after` (regex on the symbol)")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    A, B = kernels(a.before, a.rename), kernels(a.after, a.rename)
    if a.only:
        A = {k: v for k, v in A.items() if re.search(a.only, k)}
    bad = 0
    if a.label:
        print(a.label)
    print(f"kernels: before {len(A)}, after {len(B)}; only before: {sorted(set(A) - set(B))}; only after: {sorted(set(B) - set(A))}")
    bad += set(A) != set(B)
    for name in sorted(set(A) & set(B)):
        (ba, da, na, ia), (bb, db, nb, ib) = A[name], B[name]
        same = ba == bb and da == db
        bad += not same
        regs = " ".join(f"{k[1:-1]}={v}" for k, v in ib.items())
        verdict = "identical" if same else f"DIFFERENT (code {'same' if ba == bb else 'differs'}, descriptor {'same' if da == db else 'differs'}; before {na} instructions)"
        print(f"{name}  instructions={nb} {regs}  {verdict}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
