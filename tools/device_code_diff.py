#!/usr/bin/env python3
"""Are the gfx950 instruction streams of two versions of csrc/*.hip the same?  (the check of a refactor; needs no GPU)

    tools/device_code_diff.py A B deep_kernel.hip long_kernel.hip [--flags=-DJEN1_DEEP_PROFILE] [--jobs 8] [--keep DIR]

A and B are source trees (a directory that holds include/ and jen-1-pytorch_amd/csrc/) or git revisions of this repository
(exported to a temporary directory).  Every listed file is compiled on both sides with the flags of jen1_amd/lib.py build() plus
--flags, as device-only assembly, and compared per function symbol:

    instr       the text between the symbol's label and its .Lfunc_end, comments stripped, the function's index taken out of the
                local labels (.LBB<n>_, .Lfunc_end<n>; .Ltmp<n> renumbered from 0 inside the function)
    descriptor  the .amdhsa_kernel block
    metadata    the symbol's entry of .amdgpu_metadata (arguments, VGPR / SGPR / AGPR counts, LDS, scratch, spills)

and, per file, everything else the assembler reads (device variables, sections), without the .file and .ident lines and the
__hip_cuid_* symbol of the compile unit, as a bag of lines: where the device variables stand among each other follows the hash in that
symbol's name.  The figures printed are side A's; a symbol that only one side has is listed with its own.  Exit status 0: same set of symbols and all of it identical.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("jen-1-pytorch_amd", "csrc")


def tree_of(arg, tmp):
    """a directory as it is; anything else is a git revision, exported under tmp"""
    if os.path.isdir(os.path.join(arg, CSRC)):
        return os.path.abspath(arg)
    r = subprocess.run(["git", "-C", REPO, "rev-parse", "--verify", "--quiet", arg + "^{commit}"], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"{arg}: neither a source tree (no {CSRC}/ in it) nor a revision of this repository")
    rev = r.stdout.strip()
    out = os.path.join(tmp, rev[:12])
    os.makedirs(out, exist_ok=True)
    tar = subprocess.run(["git", "-C", REPO, "archive", rev, "include", CSRC], capture_output=True, check=True).stdout
    subprocess.run(["tar", "-x", "-C", out], input=tar, check=True)
    return out


def assemble(tree, name, flags, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(tree, "include"), "-I" + os.path.join(tree, CSRC),
           *flags, "--cuda-device-only", "-S", os.path.join(tree, CSRC, name), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"hipcc failed on {name} of {tree}:\n{r.stderr}")
    with open(out) as f:
        return f.read().split("\n")


def strip(line):
    return line.split(";", 1)[0].rstrip()


def parse(lines):
    """-> {symbol: {"instr": [...], "desc": [...], "meta": [...]}}, the remaining lines"""
    syms, rest = {}, []
    functions = {m.group(1) for m in (re.match(r"\s*\.type\s+(\S+),@function", l) for l in lines) if m}
    i, n = 0, len(lines)
    while i < n:
        line = lines[i]
        label = line[:-1] if line.endswith(":") else line.split(":", 1)[0] if re.match(r"\S+:\s*;", line) else None
        if label in functions:
            body, tmps, desc = [], {}, None
            i += 1
            while i < n and not re.match(r"\.Lfunc_end\d+:", lines[i]):
                s = strip(lines[i])
                if s.strip().startswith(".amdhsa_kernel "):      # a kernel's descriptor sits between its last instruction and .Lfunc_end
                    desc = syms.setdefault(label, {})["desc"] = []
                if desc is not None:
                    desc.append(s)
                    if s.strip() == ".end_amdhsa_kernel":
                        desc = None
                elif s.strip():
                    s = re.sub(r"\.LBB\d+_", ".LBB_", s)
                    s = re.sub(r"\.Ltmp\d+", lambda m: ".Ltmp%d" % tmps.setdefault(m.group(0), len(tmps)), s)
                    body.append(s)
                i += 1
            syms.setdefault(label, {})["instr"] = body
        elif line.strip() == ".amdgpu_metadata":
            entry = None
            i += 1
            while lines[i].strip() != ".end_amdgpu_metadata":
                if lines[i].startswith("  - "):          # a new entry of amdhsa.kernels
                    entry = []
                elif not lines[i].startswith("    "):    # back at the top level of the document
                    entry = None
                    rest.append(lines[i])
                if entry is not None:
                    entry.append(lines[i])
                    m = re.match(r"\s+\.symbol:\s+'?([^'\s]+?)(\.kd)?'?$", lines[i])
                    if m:
                        syms.setdefault(m.group(1), {})["meta"] = entry
                i += 1
        elif not re.match(r"\s*\.(file|ident)\s", line) and "__hip_cuid_" not in line:
            s = strip(line)
            if s.strip():
                rest.append(re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", s))
        i += 1
    return syms, sorted(rest)


def figure(meta, key):
    for l in meta or []:
        m = re.match(r"\s+(?:- )?\." + key + r":\s+(\d+)", l)
        if m:
            return int(m.group(1))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("files", nargs="+", help="names under jen-1-pytorch_amd/csrc/")
    ap.add_argument("--flags", default="", help="added to the build's flags on both sides")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--keep", help="leave the assembly files in this directory")
    ap.add_argument("--quiet", action="store_true", help="one line per file instead of the per-symbol table")
    args = ap.parse_args()
    flags = args.flags.split()
    with tempfile.TemporaryDirectory() as tmp:
        out = args.keep or tmp
        os.makedirs(out, exist_ok=True)
        trees = [tree_of(args.a, tmp), tree_of(args.b, tmp)]
        tag = "".join(c if c.isalnum() else "_" for c in args.flags)
        jobs = [(t, f, os.path.join(out, f"{f}.{tag}.{'ab'[k]}.s")) for f in args.files for k, t in enumerate(trees)]
        with ThreadPoolExecutor(max_workers=args.jobs) as ex:
            texts = list(ex.map(lambda j: assemble(j[0], j[1], flags, j[2]), jobs))
    ok = True
    for k, f in enumerate(args.files):
        (sa, ra), (sb, rb) = parse(texts[2 * k]), parse(texts[2 * k + 1])
        print(f"{f}  {args.flags or '(default flags)'}: {len(texts[2 * k])} lines of assembly")
        same_set = sorted(sa) == sorted(sb)
        n_same = 0
        def figures(sym):
            m = sym.get("meta")
            return (f"{len(sym.get('instr', []))} lines, vgpr {figure(m, 'vgpr_count')} sgpr {figure(m, 'sgpr_count')} agpr {figure(m, 'agpr_count')} "
                    f"lds(static) {figure(m, 'group_segment_fixed_size')} scratch {figure(m, 'private_segment_fixed_size')} "
                    f"spills {figure(m, 'sgpr_spill_count')}+{figure(m, 'vgpr_spill_count')}")

        for s in sorted(set(sa) | set(sb)):
            if s not in sa or s not in sb:       # (a renamed instantiation: its own figures, to lay beside those of the symbol it replaces)
                print(f"  {s}\n      only in {'A' if s in sa else 'B'}   {figures(sa[s] if s in sa else sb[s])}")
                continue
            a, b = sa[s], sb[s]
            cmp = {part: ("-" if part not in a and part not in b else "same" if a.get(part) == b.get(part) else "DIFFERS") for part in ("instr", "desc", "meta")}
            n_same += "DIFFERS" not in cmp.values()
            if not args.quiet or "DIFFERS" in cmp.values():
                print(f"  {s}\n      instr={cmp['instr']} descriptor={cmp['desc']} metadata={cmp['meta']}   {figures(a)}")
        good = same_set and n_same == len(sa) and ra == rb
        ok &= good
        print(f"  => {'identical' if good else 'NOT identical'}: {len(sa)} symbols in A, {len(sb)} in B, {n_same} identical in all three; "
              f"rest of the file (device variables, sections) {'same' if ra == rb else 'DIFFERS'}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
