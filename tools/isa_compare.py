#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two source trees, kernel symbol by kernel symbol.

    tools/isa_compare.py OLD_TREE NEW_TREE [--work DIR] [--jobs N] [--pattern REGEX]

Every translation unit of ccsd_amd/csrc/ is compiled with `hipcc -S --cuda-device-only` in both trees (no GPU needed; a
unit whose assembly in DIR is newer than the tree's sources is not compiled again).  Per symbol it prints
  identical     the function text, its .amdhsa_kernel descriptor and the resource comments behind it are byte-identical
  same opcodes  equal line count and opcode multiset, and unchanged descriptor / register / scratch / LDS / occupancy lines
  different     anything else (also: present in one tree only)
followed by the resource lines of the NEW tree's symbol and, where one of them moved, `[old -> new]` per moved figure.  It compares text;
it knows nothing about particular instructions.  Not part of the comparison: the number behind a compiler-local label's name -- every
`.L<name><n>` (`.LBB<f>_<n>` and `.Lfunc_end<f>`, where <f> is the ordinal of the function inside its unit, but also `.Ltmp<n>`, `.LJTI<f>_<n>`
and any other such label: their numbering is erased alike, while their positions and the code between them still count) and `BB<f>_<n>` in
comments --, the column at which a comment starts, and the `.globl` / `.protected` / `.p2align` lines ahead of a function, which name that
function and not the one before it.  So a kernel added in the middle of a unit leaves the functions behind it `identical` where their code is.
A unit that only one of the trees has lists its symbols as present in that tree only.
Exit status 1 when any symbol is `different`.
"""
import argparse
import collections
import os
import re
import subprocess
import sys

UNITS = ["ccsd_hip", "ccsd_r2", "ccsd_r2b", "ccsd_r2c", "ccsd_r2d", "ccsd_xa", "ccsd_lg", "ccsd_lgw"]
CSRC = os.path.join("ccsd_amd", "csrc")
STATS = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy", "codeLenInByte")


def compile_all(trees, work, jobs):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    todo = []
    for tag, tree in trees.items():
        os.makedirs(os.path.join(work, tag), exist_ok=True)
        src_dir = os.path.join(tree, CSRC)
        newest = max(os.path.getmtime(os.path.join(d, f)) for d in (src_dir, os.path.join(tree, "include")) for f in os.listdir(d))
        for u in UNITS:
            if not os.path.exists(os.path.join(tree, CSRC, u + ".hip")):      # (a unit only one of the trees has: its symbols are in one tree only)
                continue
            out = os.path.join(work, tag, u + ".s")
            if not os.path.exists(out) or os.path.getmtime(out) < newest:
                # relative source path, cwd = the tree: nothing in the assembly depends on where the tree lies
                todo.append((tree, out, [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                                         "-o", out + ".tmp", os.path.join(CSRC, u + ".hip")]))
    running, failed = [], False
    while todo or running:
        while todo and len(running) < jobs:
            tree, out, cmd = todo.pop(0)
            running.append((out, subprocess.Popen(cmd, cwd=tree, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)))
        out, proc = running.pop(0)
        err = proc.communicate()[1]
        if proc.returncode != 0:
            sys.stderr.write(f"hipcc failed for {out}:\n{err.decode()[-4000:]}\n")
            failed = True
        else:
            os.replace(out + ".tmp", out)
    if failed:
        sys.exit(2)


def split_symbols(path):
    """-> ({symbol: {"body": [...], "desc": [...], "stats": {...}}}, [every line that belongs to no symbol])"""
    syms, rest = collections.OrderedDict(), []
    if not os.path.exists(path):
        return syms, rest
    cur, part = None, None            # part: "body" up to the symbol's .Lfunc_end, "desc" inside its .amdhsa_kernel block, "tail" behind (resource comments)
    for line in open(path):
        line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", line.rstrip("\n"))      # (a hash of the unit's path and contents)
        # compiler-local labels (.LBB<f>_<n>, .Lfunc_end<f>, BB<f>_<n> in comments) carry the ordinal <f> of their function in the unit: a
        # kernel added ahead of a function renumbers them without changing a byte of its code
        line = re.sub(r"(\.L[A-Za-z_]+|\bBB)\d+(?=_\d|:|-|\s|$)", r"\1", line)
        line = re.sub(r"\s+;", " ;", line)            # (the comment column moves with the label's width)
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            # (the .protected / .globl / .p2align lines ahead of it name this function, not the one before)
            prev = cur["desc"] if cur is not None else rest
            while prev and re.match(r"\s*\.(protected|globl|weak|p2align|section\s+\.text)", prev[-1]):
                prev.pop()
            cur, part = syms.setdefault(m.group(1), {"body": [], "desc": [], "stats": {}}), "body"
            continue
        if cur is None:
            rest.append(line)
            continue
        m = re.match(r"; (\w+)(?::| =) (\d+)", line)
        if m and m.group(1) in STATS:
            cur["stats"][m.group(1)] = int(m.group(2))
            cur["desc"].append(line)
        elif part == "desc" or re.match(r"\s*\.amdhsa_kernel\s", line):      # (sits inside the function, ahead of its .Lfunc_end)
            cur["desc"].append(line)
            part = "body" if ".end_amdhsa_kernel" in line else "desc"
        elif part == "body":
            cur["body"].append(line)
            if re.match(r"\.Lfunc_end\d*:", line):
                part = "tail"
        elif re.match(r"\s*\.(amdgpu_metadata|ident|addrsig)|\s*\.section\s+\S*\.note|\s*\.type\s", line):
            cur = None                 # (behind the last function, or a variable: no symbol's text)
            rest.append(line)
        else:
            cur["desc"].append(line)   # the resource comment block behind the function counts with its descriptor
    return syms, rest


def opcodes(body):
    ops = collections.Counter()
    for line in body:
        s = line.strip()
        if s and s[0] not in ".;" and not s.split()[0].endswith(":"):
            ops[s.split()[0]] += 1
    return ops


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--work", default="build/isa_compare")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--pattern", default=".")
    a = ap.parse_args()
    compile_all({"old": os.path.abspath(a.old), "new": os.path.abspath(a.new)}, a.work, max(1, min(a.jobs, 16)))
    totals = collections.Counter()
    for u in UNITS:
        old, old_rest = split_symbols(os.path.join(a.work, "old", u + ".s"))
        new, new_rest = split_symbols(os.path.join(a.work, "new", u + ".s"))
        for name in list(new) + [n for n in old if n not in new]:
            o, n = old.get(name), new.get(name)
            if o is None or n is None:
                verdict = "different (only in %s)" % ("new" if o is None else "old")
            elif o["body"] == n["body"] and o["desc"] == n["desc"]:
                verdict = "identical"
            elif (len(o["body"]) == len(n["body"]) and opcodes(o["body"]) == opcodes(n["body"]) and o["desc"] == n["desc"]
                  and all(o["stats"].get(k) == n["stats"].get(k) for k in STATS)):
                moved = sum(x != y for x, y in zip(o["body"], n["body"]))
                verdict = f"same opcodes ({moved} of {len(n['body'])} lines differ in place)"
            else:
                verdict = "different"
            totals[verdict.split(" (")[0]] += 1
            if re.search(a.pattern, name):
                s = (n or o)["stats"]
                moved = ", ".join(f"{k} {o['stats'].get(k)} -> {s.get(k)}" for k in STATS if o and n and o["stats"].get(k) != s.get(k))
                print(f"{u:9s} {verdict:14s} lines {len((n or o)['body']):6d} vgpr {s.get('NumVgprs', -1):3d} agpr {s.get('NumAgprs', -1):3d} "
                      f"sgpr {s.get('TotalNumSgprs', -1):3d} scratch {s.get('ScratchSize', -1):4d} lds {s.get('LDSByteSize', -1):6d} "
                      f"occ {s.get('Occupancy', -1)} bytes {s.get('codeLenInByte', -1):6d}  {name}" + (f"  [{moved}]" if moved else ""))
        same = old_rest == new_rest
        totals["identical" if same else "different"] += 1
        print(f"{u:9s} {'identical' if same else 'different':14s} <everything outside the functions: metadata, kernel arguments, variables>")
    print("total: " + ", ".join(f"{totals[k]} {k}" for k in ("identical", "same opcodes", "different")))
    return 1 if totals["different"] else 0


if __name__ == "__main__":
    sys.exit(main())
