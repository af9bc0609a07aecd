#!/usr/bin/env python3
"""Code-generation diff of the kernel files of two source trees (CPU only: hipcc cross-compiles for gfx950).

    python tools/codegen_diff.py PARENT_CSRC BRANCH_CSRC [file.hip ...]

Compiles gemm.hip and conv_direct.hip (plus every file named) from both csrc directories with the Makefile's flags plus
-S --cuda-device-only -Rpass-analysis=kernel-resource-usage, and prints per kernel instance: VGPRs, AGPRs, both spill
counts, scratch, LDS, occupancy, the instruction count and the mnemonics whose counts differ.  A kernel instance is named
by its demangled signature.  Exit status 1 when anything differs, 0 when every instance is identical.  It is a diff tool:
it knows no instruction and judges none.  `--json FILE` also writes the branch's table; `--markdown` prints a table for a note.

`--sequence` also compares, per instance, the ORDERED list of mnemonics and reports "equal" or the position of the first
difference: counts can match while the schedule moved.  `--from REGEX --to REGEX` adds the same comparison for the window from
the first mnemonic matching FROM to the last matching TO (e.g. a K loop: --from s_barrier --to v_mfma); the patterns are the
caller's, the tool compares text.  A sequence that differs counts as a difference for the exit status; a window does not.
"""
import argparse
import collections
import concurrent.futures
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# csrc/Makefile: CXXFLAGS, and EXTRA of the attention files
CXXFLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffast-math", "-fno-finite-math-only", "-Wall",
            "-Wno-unused-function", "-Wno-unused-variable"]
ATTN_EXTRA = ["-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-honor-nans", "-fhonor-infinities"]
ATTN_FILES = ("attention.hip", "attention_pipe.hip", "attention_pipe128.hip", "attention_cross.hip")
DEFAULT_FILES = ("gemm.hip", "conv_direct.hip")
FIELDS = (("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("VGPRs Spill", "VGPR spill"), ("SGPRs Spill", "SGPR spill"),
          ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "LDS"), ("Occupancy [waves/SIMD]", "occupancy"))


def demangle(names):
    """mangled -> readable signature where a demangler is installed, else the mangled name itself"""
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not names or not tool:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
    plain = out.stdout.splitlines() if out.returncode == 0 else names
    return dict(zip(names, plain)) if len(plain) == len(names) else {n: n for n in names}


def compile_file(csrc, source, defines=()):
    """{kernel: {"res": {field: n}, "ops": Counter(mnemonic -> n), "seq": [mnemonic, ...]}} of one file."""
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "out.s")
        cmd = [HIPCC, *CXXFLAGS, *(ATTN_EXTRA if source in ATTN_FILES else []), *defines, "-S", "--cuda-device-only",
               "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, source), "-o", asm]
        out = subprocess.run(cmd, capture_output=True, text=True, cwd=csrc)
        if out.returncode != 0:
            sys.exit("%s\n%s: compile failed" % (out.stderr[-4000:], os.path.join(csrc, source)))
        res, name = {}, None
        for line in out.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                res[name] = {}
            m = re.search(r"remark:\s+([A-Za-z ]+(?: \[[^\]]+\])?): (\d+)", line)
            if m and name and m.group(1).strip() in dict(FIELDS):
                res[name][m.group(1).strip()] = int(m.group(2))
        ops, seq, cur = {}, {}, None
        with open(asm) as f:
            for line in f:
                m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
                if m:
                    cur = m.group(1) if m.group(1) in res else (cur if m.group(1).startswith(".L") else None)
                    if cur and cur not in ops:
                        ops[cur] = collections.Counter()
                        seq[cur] = []
                    continue
                if cur is None:
                    continue
                s = line.strip()
                if s.startswith(".end_amdhsa_kernel") or s.startswith(".Lfunc_end"):
                    cur = None if s.startswith(".Lfunc_end") else cur
                    continue
                if not s or s[0] in ".;/#":
                    continue
                ops[cur][s.split()[0]] += 1
                seq[cur].append(s.split()[0])
    names = demangle(list(res))
    return {names[k]: {"res": res[k], "ops": ops.get(k, collections.Counter()), "seq": seq.get(k, [])} for k in res}


def first_difference(p, b):
    """"equal", or where two mnemonic lists part"""
    if p == b:
        return "equal (%d)" % len(b)
    i = next((i for i, (x, y) in enumerate(zip(p, b)) if x != y), min(len(p), len(b)))
    return "differs at %d of %d / %d: %s / %s" % (i, len(p), len(b), p[i] if i < len(p) else "(end)", b[i] if i < len(b) else "(end)")


def window(seq, first, last):
    """seq from the first mnemonic matching `first` to the last matching `last`, both included; [] where either is missing"""
    lo = next((i for i, m in enumerate(seq) if re.search(first, m)), None)
    hi = next((i for i in range(len(seq) - 1, -1, -1) if re.search(last, seq[i])), None)
    return seq[lo:hi + 1] if lo is not None and hi is not None else []


def short(sig):
    """kernel<template arguments>, without namespace and parameter list"""
    s = re.sub(r"^void ", "", sig)
    s = re.sub(r"\(.*\)$", "", s)
    return s.replace("ltxmi::", "")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent_csrc")
    ap.add_argument("branch_csrc")
    ap.add_argument("files", nargs="*")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="extra -D for both trees")
    ap.add_argument("--json", help="write the branch's per-instance table here")
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--sequence", action="store_true", help="also compare the ordered mnemonic list of every instance")
    ap.add_argument("--from", dest="win_from", metavar="REGEX", help="with --to: also compare this window of the sequence")
    ap.add_argument("--to", dest="win_to", metavar="REGEX")
    a = ap.parse_args()
    if bool(a.win_from) != bool(a.win_to) or (a.win_from and not a.sequence):
        ap.error("--from and --to go together, with --sequence")
    extra_cols = (["sequence"] if a.sequence else []) + (["window"] if a.win_from else [])
    a.parent_csrc, a.branch_csrc = os.path.abspath(a.parent_csrc), os.path.abspath(a.branch_csrc)
    files = list(DEFAULT_FILES) + [f for f in a.files if f not in DEFAULT_FILES]
    defines = ["-D" + d for d in a.defines]
    differ, table = 0, {}
    for source in files:
        in_parent = os.path.exists(os.path.join(a.parent_csrc, source))
        in_branch = os.path.exists(os.path.join(a.branch_csrc, source))
        if not (in_parent and in_branch):
            print("== %s: only in the %s tree" % (source, "parent's" if in_parent else "branch's"))
            continue
        with concurrent.futures.ThreadPoolExecutor(2) as pool:         # the two trees side by side
            par, br = pool.map(lambda d: compile_file(d, source, defines), (a.parent_csrc, a.branch_csrc))
        table[source] = {short(k): dict(v["res"], instructions=sum(v["ops"].values())) for k, v in br.items()}
        n_par, n_br = sum(sum(v["ops"].values()) for v in par.values()), sum(sum(v["ops"].values()) for v in br.values())
        print("== %s: %d / %d kernel instances, %d / %d instructions (parent / branch)" % (source, len(par), len(br), n_par, n_br))
        if a.markdown:
            print("| instance | " + " | ".join(t for _, t in FIELDS) + " | instructions | differs |" + "".join(" %s |" % c for c in extra_cols))
            print("|---|" + "---|" * (len(FIELDS) + 2 + len(extra_cols)))
        bad_here = 0
        for k in sorted(set(par) | set(br)):
            if k not in par or k not in br:
                print("  %s: only in the %s" % (short(k), "parent" if k in par else "branch"))
                bad_here += 1
                continue
            p, b = par[k], br[k]
            cols = []
            for f, _ in FIELDS:
                pv, bv = p["res"].get(f), b["res"].get(f)
                cols.append(str(bv) if pv == bv else "%s -> %s" % (pv, bv))
            pi, bi = sum(p["ops"].values()), sum(b["ops"].values())
            cols.append(str(bi) if pi == bi else "%d -> %d" % (pi, bi))
            ops = ["%s %d -> %d" % (o, p["ops"][o], b["ops"][o]) for o in sorted(set(p["ops"]) | set(b["ops"]))
                   if p["ops"][o] != b["ops"][o]]
            same = p["res"] == b["res"] and not ops
            extra = []
            if a.sequence:
                extra.append(first_difference(p["seq"], b["seq"]))
                same = same and p["seq"] == b["seq"]
            if a.win_from:
                extra.append(first_difference(window(p["seq"], a.win_from, a.win_to), window(b["seq"], a.win_from, a.win_to)))
            bad_here += not same
            if a.markdown:
                print("| `%s` | %s | %s |%s" % (short(k), " | ".join(cols), "no" if same else ", ".join(ops) or ("resources" if p["res"] != b["res"] else "order"),
                                                "".join(" %s |" % e for e in extra)))
            else:
                print("  %-100s %s" % (short(k), "  ".join("%s %s" % (t, c) for (_, t), c in zip(list(FIELDS) + [("", "instr")], cols))))
                if ops:
                    print("      mnemonic counts that differ: " + ", ".join(ops))
                for c, e in zip(extra_cols, extra):
                    print("      %s: %s" % (c, e))
        print("   %s" % ("identical" if not bad_here else "%d instance(s) DIFFER" % bad_here))
        differ += bad_here
    if a.json:
        with open(a.json, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
