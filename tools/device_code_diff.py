#!/usr/bin/env python3
"""Compare the device code of two csrc trees kernel by kernel — the check behind "this refactor is a re-spelling". No GPU needed.

    python tools/device_code_diff.py PARENT_CSRC NEW_CSRC [--same-as NEW_UNIT=PARENT_UNIT]

Every *.hip of both trees is compiled to an assembly listing (`hipcc <make print-flags> -S --cuda-device-only`, as
tests/test_mfma_hazard_scan.py does). A listing is cut into one piece per function symbol: its instructions, its `.amdhsa_*` block and
its resource `.set` lines, plus its entry in the metadata (arguments, VGPRs, SGPRs, LDS, scratch). What says nothing about the code
is dropped: comment text, `.loc` / `.file` / `.ident`, the per-compilation `__hip_cuid_*` symbol, and the function's running number
in local labels (`.LBB3_7`, `.Lfunc_end3`). One line per kernel: identical, changed (with the first differing line), or only in one
tree. `--same-as train_blocks.hip=train.hip`: a unit that exists only in the new tree because it re-compiles another one (it #includes
it) is held against the PARENT's listing of that other unit. Exit status 1 unless everything is identical."""
import argparse
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

_DROP = re.compile(r"^\s*\.(loc|file|ident)\b|__hip_cuid_")
_LOCAL = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end|Ltmp)\d+")
_TYPE = re.compile(r"^\s*\.type\s+([^,\s]+),@function")
_END = re.compile(r"^\.Lfunc_end\d+:")
_ENTRY = re.compile(r"^  - \.")
_NAME = re.compile(r"^    \.name:\s+(\S+)")


def _clean(line):
    """A listing line without what does not describe the code; '' when nothing is left."""
    if _DROP.search(line):
        return ""
    if ";" in line and not re.match(r"\s*\.(asciz|ascii|string)\b", line):
        line = line[: line.index(";")]
    return _LOCAL.sub(lambda m: "." + m.group(1), " ".join(line.split()))


def split_listing(text):
    """{function symbol: cleaned lines of its code, descriptor, resource symbols and metadata entry}"""
    lines = text.splitlines()
    out, i = {}, 0
    while i < len(lines):
        m = _TYPE.match(lines[i])
        i += 1
        if not m:
            continue
        sym, body = m.group(1), []
        while i < len(lines) and not _END.match(lines[i]):  # the label, the code and (for a kernel) the .amdhsa_kernel block
            body.append(lines[i])
            i += 1
        while i < len(lines) and not _TYPE.match(lines[i]) and not lines[i].lstrip().startswith(".amdgpu_metadata"):
            if lines[i].lstrip().startswith(".set " + sym + "."):
                body.append(lines[i])
            i += 1
        out[sym] = [c for c in map(_clean, body) if c]
    if ".amdgpu_metadata" in text:
        entries, entry = [], None
        for line in text[text.index(".amdgpu_metadata") :].splitlines():
            if _ENTRY.match(line):  # an element of amdhsa.kernels
                entry = []
                entries.append(entry)
            elif not line.startswith(" "):  # amdhsa.target, amdhsa.version, the end of the block
                entry = None
            if entry is not None:
                entry.append(line)
        for entry in entries:
            name = next((_NAME.match(l).group(1) for l in entry if _NAME.match(l)), None)
            if name is not None:
                out.setdefault(name, []).extend("meta " + c for c in map(_clean, entry) if c)
    return out


def compare_listings(parent_text, new_text):
    """[(symbol, verdict, detail)], verdict one of 'identical', 'changed', 'only in parent', 'only in new'"""
    a, b = split_listing(parent_text), split_listing(new_text)
    rows = []
    for sym in sorted(set(a) | set(b)):
        if sym not in b:
            rows.append((sym, "only in parent", ""))
        elif sym not in a:
            rows.append((sym, "only in new", ""))
        elif a[sym] == b[sym]:
            rows.append((sym, "identical", ""))
        else:
            k = next((k for k, (x, y) in enumerate(zip(a[sym], b[sym])) if x != y), min(len(a[sym]), len(b[sym])))
            x = a[sym][k] if k < len(a[sym]) else "<end>"
            y = b[sym][k] if k < len(b[sym]) else "<end>"
            rows.append((sym, "changed", f"{x}  ->  {y}"))
    return rows


def _listings(csrc, outdir, jobs):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    flags = subprocess.run(["make", "-s", "-C", csrc, "print-flags"], capture_output=True, text=True, check=True).stdout.split()

    def dump(src):
        out = os.path.join(outdir, os.path.basename(src)[:-4] + ".s")
        subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", src, "-o", out], check=True, capture_output=True, cwd=csrc)
        return os.path.basename(src), open(out).read()

    with ThreadPoolExecutor(max_workers=jobs) as pool:
        return dict(pool.map(dump, sorted(glob.glob(os.path.join(csrc, "*.hip")))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent_csrc")
    ap.add_argument("new_csrc")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--same-as", action="append", default=[], metavar="NEW_UNIT=PARENT_UNIT")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        sides = []
        for name, csrc in (("parent", args.parent_csrc), ("new", args.new_csrc)):
            os.mkdir(os.path.join(tmp, name))
            sides.append(_listings(os.path.abspath(csrc), os.path.join(tmp, name), args.jobs))
    for new_unit, parent_unit in (pair.split("=", 1) for pair in args.same_as):
        sides[0][new_unit] = sides[0][parent_unit]
    counts = {}
    for unit in sorted(set(sides[0]) | set(sides[1])):
        for sym, verdict, detail in compare_listings(sides[0].get(unit, ""), sides[1].get(unit, "")):
            counts[verdict] = counts.get(verdict, 0) + 1
            print(f"{verdict:14s} {unit:20s} {sym}" + (f"\n{'':14s} {detail}" if detail else ""))
    print(", ".join(f"{n} {v}" for v, n in sorted(counts.items())))
    return 0 if set(counts) <= {"identical"} else 1


if __name__ == "__main__":
    sys.exit(main())
