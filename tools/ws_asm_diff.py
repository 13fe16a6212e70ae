#!/usr/bin/env python3
"""Is the machine code of the weights-stationary kernels still the same?

    hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 \\
          --cuda-device-only -S -I include -I point-gnn_amd/csrc \\
          point-gnn_amd/csrc/gnn.hip -o X.s          (before and after a change)
    tools/ws_asm_diff.py [--all] A.s B.s [kernel-name-substring]

For every *ws*kernel* symbol -- with --all: for every kernel of the two files,
the check of a change that must leave the whole device side alone -- `same`
when the instruction streams and the kernel descriptors agree after
renumbering labels, otherwise the register / scratch / LDS / kernarg figures
and instruction counts of both sides (and, for the kernels that match the
substring, a unified diff).  Kernels are paired by demangled name; the two
split-precision edge kernels are also found under the names they had as
separate kernels.  The last line counts the kernels compared; exit status 1
when any differs.  Needs c++filt."""
import re
import subprocess
import sys
import difflib

RENAME = [
    # the aggregation policy (ws_sum.h) defaults to the max the kernels had
    (r", pgnn::WsMax>", r">"),
    (r"edge_ws_bf16x3_kernel<(\d+), (\d+)>", r"edge_ws_split_kernel<pgnn::Bf16x3, \1, \2>"),
    (r"edge_ws_f16x2_kernel<(\d+), (\d+)>", r"edge_ws_split_kernel<pgnn::F16x2, \1, \2>"),
]
COUNT = ["v_mfma", "ds_read", "global_load", "v_pk_"]
META = (r"\.amdhsa_(next_free_vgpr|next_free_sgpr|accum_offset|"
        r"group_segment_fixed_size|private_segment_fixed_size|kernarg_size)\s+(\S+)")
ARGS = [x for x in sys.argv[1:] if x != "--all"]
ALL = "--all" in sys.argv[1:]


def kernels(path):
    out, name, body = {}, None, []
    meta = {}
    for line in open(path):
        s = line.strip()
        if name is None:
            m = re.match(r"^(_Z\w+):", line)
            if m and "kernel" in m.group(1) and (ALL or "ws_" in m.group(1)):
                name, body = m.group(1), []
            m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
            if m:
                cur = m.group(1)
                meta[cur] = {}
            m = re.match(META, s)
            if m and meta:
                meta[cur][m.group(1)] = m.group(2)
            continue
        if s.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        if not s or s.startswith(";"):
            continue
        if s.startswith(".amdhsa_") or s.startswith(".end_amdhsa") or s.startswith(".section") or s == ".text":
            m = re.match(META, s)
            if m:
                meta.setdefault(name, {})[m.group(1)] = m.group(2)
            continue
        s = re.sub(r"\s*;.*$", "", s)
        body.append(s)
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names),
                         capture_output=True, text=True).stdout.split("\n")
    res = {}
    for n, d in zip(names, dem):
        d = re.sub(r"^void ", "", d).replace("(anonymous namespace)", "{anon}")
        d = re.sub(r"\(.*$", "", d)
        for a, b in RENAME:
            d = re.sub(a, b, d)
        labels = {}
        b2 = []
        for s in out[n]:
            s = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s)
            s = s.replace(n, "SELF")
            b2.append(s)
        # renumber labels in order of first appearance
        def ren(m):
            return labels.setdefault(m.group(0), ".L%d" % len(labels))
        b2 = [re.sub(r"\.LBB_\d+", ren, s) for s in b2]
        res[d] = (b2, meta.get(n, {}))
    return res


def counts(body):
    c = {k: sum(1 for s in body if s.startswith(k)) for k in COUNT}
    c["all"] = sum(1 for s in body if not s.endswith(":"))
    return c


a, b = kernels(ARGS[0]), kernels(ARGS[1])
show = len(ARGS) > 2
bad = 0
for k in sorted(set(a) | set(b)):
    if k not in a or k not in b:
        print("ONLY in", "A" if k in a else "B", k)
        bad += 1
        continue
    same = a[k][0] == b[k][0] and a[k][1] == b[k][1]
    print("%-9s %s" % ("same" if same else "DIFFERENT", k))
    if not same:
        bad += 1
        print("   A", a[k][1], counts(a[k][0]))
        print("   B", b[k][1], counts(b[k][0]))
        if show and ARGS[2] in k:
            for l in difflib.unified_diff(a[k][0], b[k][0], lineterm="", n=2):
                print("     ", l)
print("%d kernels compared, %d differ" % (len(set(a) | set(b)), bad))
sys.exit(1 if bad else 0)
