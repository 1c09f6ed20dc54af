#!/usr/bin/env python3
"""Instruction counts of grad_kernel's tile loops, from the compiler alone (no GPU): compiles deep_rl_amd/csrc/mi_update.hip to gfx950 assembly with the Makefile's
FLAGS and prints, per instantiation (grad_kernel_f32, grad_kernel_bx) and role (actor, critic), every loop of at least --min instructions by class: MFMA by shape,
transcendental VALU, other VALU by mnemonic, DS by width, VMEM, SALU, s_waitcnt.  A loop is the text between a backward branch and its target label; the role is
read off the loop itself (only the actor's loss takes a logarithm).  `tiles` = 4x4x1 MFMAs / 16 (the dW1 chain of one tile): an unrolled loop shows its counts per
iteration and per tile.  The script counts classes and nothing else.

usage: tools/grad_loop_isa.py [--src DIR] [--min 300] [--keep FILE.s] [--json]     (DIR: a csrc directory, default the tree's own; e.g. one of another checkout)"""
import argparse
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")


def makefile_flags(csrc):
    mk = open(os.path.join(csrc, "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*\?=\s*(.*)$" % name, mk, re.M).group(1).strip()   # noqa: E731
    return var("HIPCC"), var("FLAGS").replace("$(ARCH)", var("ARCH")).split()


def compile_asm(csrc, out):
    hipcc, flags = makefile_flags(csrc)
    subprocess.run([hipcc] + flags + ["-Wno-unused-command-line-argument", "--cuda-device-only", "-S", "-o", out, os.path.join(csrc, "mi_update.hip")], check=True)


def classify(op):
    if "mfma" in op:
        return "MFMA", re.sub(r"^v_mfma_f32_", "", op)
    if op.startswith("v_"):
        name = re.sub(r"_e32|_e64|_dpp|_sdwa", "", op)
        return ("transcendental", name) if op.startswith(TRANS) else ("VALU", name)
    if op.startswith("ds_"):
        return "DS", op
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "VMEM", op
    if op.startswith("s_waitcnt"):
        return "s_waitcnt", op
    if op.startswith("s_"):
        return "SALU", op
    return "other", op


def loops(asm, kernel, minlen):
    m = re.search(r"^(_Z\w*%s\w*):" % re.escape(kernel), asm, re.M)
    body = asm[m.end():]
    body = body[:re.search(r"^\.Lfunc_end\d+:", body, re.M).start()]
    lines = [l.strip() for l in body.split("\n")]
    labels = {}
    for n, l in enumerate(lines):
        lab = re.match(r"^(\.LBB\d+_\d+):", l)
        if lab:
            labels[lab.group(1)] = n
    out = []
    for n, l in enumerate(lines):
        b = re.match(r"s_c?branch\w* (\.LBB\d+_\d+)", l)
        if not (b and b.group(1) in labels and labels[b.group(1)] < n):
            continue
        seg = [x.split()[0] for x in lines[labels[b.group(1)]:n + 1] if x and not x.startswith((".", ";"))]
        if len(seg) < minlen:
            continue
        c = collections.Counter(classify(op) for op in seg)
        out.append(dict(label=b.group(1), instructions=len(seg), counts=c))
    return out


def report(asm, minlen):
    res = {}
    for kernel in ("grad_kernel_f32", "grad_kernel_bx"):
        for lp in loops(asm, kernel, minlen):
            c = lp["counts"]
            cls = collections.Counter()
            for (k, _), v in c.items():
                cls[k] += v
            tiles = sum(v for (k, name), v in c.items() if k == "MFMA" and name.startswith("4x4x1")) / 16.0
            if tiles == 0:      # a loop of the prologue (block_grad_norm), not a tile loop
                continue
            role = "actor" if any(name.startswith("v_log_") for (k, name) in c) else "critic"
            r = dict(kernel=kernel, role=role, label=lp["label"], instructions=lp["instructions"], tiles=tiles, classes=dict(cls),
                     detail={k: {name: v for (kk, name), v in sorted(c.items(), key=lambda kv: -kv[1]) if kk == k} for k in cls})
            # a loop with inner control flow has several backward branches: the outermost (longest) span per loop is the loop
            key = (kernel, role, tiles)
            if key not in res or res[key]["instructions"] < r["instructions"]:
                res[key] = r
    return list(res.values())


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(here, "..", "deep_rl_amd", "csrc"))
    ap.add_argument("--min", type=int, default=300)
    ap.add_argument("--keep")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = a.keep or os.path.join(tmp, "mi_update.s")
        compile_asm(a.src, path)
        res = report(open(path).read(), a.min)
    if a.json:
        json.dump(res, sys.stdout, indent=1)
        print()
        return
    order = ("MFMA", "transcendental", "VALU", "DS", "VMEM", "SALU", "s_waitcnt", "other")
    for r in res:
        t = r["tiles"] or 1.0
        print("%s %s loop %s: %d instructions, %g tile(s) per iteration" % (r["kernel"], r["role"], r["label"], r["instructions"], r["tiles"]))
        for k in order:
            if k not in r["classes"]:
                continue
            n = r["classes"][k]
            print("  %-15s %5d  (%.1f per tile)" % (k, n, n / t))
            if k in ("MFMA", "transcendental", "VALU", "DS", "VMEM"):
                for name, v in r["detail"][k].items():
                    print("      %-36s %4d" % (name, v))
        if "VALU" in r["classes"]:
            allv = r["classes"]["VALU"] + r["classes"].get("transcendental", 0)
            print("  %-15s %5d  (%.1f per tile)" % ("VALU + transc.", allv, allv / t))


if __name__ == "__main__":
    main()
