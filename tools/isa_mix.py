#!/usr/bin/env python3
"""Static VALU instruction mix of the compositing backward's hot loop (for bench.py's calibrated `roofline.valu_frac`).

Cross-compiles d3ga_amd/csrc/raster_composite_scan.hip to gfx950 assembly (no GPU needed), takes the group loop of
composite_bwd_tile_kernel<false, 512, false, 1, false, false> (the headline's) -- a depth-2 loop over the four block lines (the
first child loop, recognised by its DPP scans) counted four times, the rest of the depth-1 loop (with the lines unrolled: all
of them) once, each insert loop once per attempt, divided by the groups per trip (the loop may run two) -- and classes every
VALU instruction by the issue-cost classes tools/micro/valu_issue.hip measures:
plain (2-operand / fma), dpp, transcendental, packed, and other VOP3 (cndmask / cmp with an SGPR pair, med3, bfi ...).
Writes profiles/r07_composite_bwd_mix.json (one per round; bench.py reads the newest).

    python tools/isa_mix.py [KERNEL_PREFIX] [--src FILE.hip] [--out FILE.json]
"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "d3ga_amd", "csrc", "raster_composite_scan.hip")


def classify(op, line):
    if not op.startswith("v_"):
        return None
    if "_dpp" in op or "row_shr" in line or "quad_perm" in line or "row_ror" in line:
        return "dpp"
    if re.match(r"v_(exp|log|rcp|rsq|sqrt|sin|cos)_", op):
        return "trans"
    if op.startswith("v_pk_"):
        return "packed"
    if re.match(r"v_(cndmask_b32_e64|cmp\w*_e64|med3|bfi|mad_u64|lshl_add|add3|perm|readlane|writelane|readfirstlane)", op):
        return "vop3_other"
    return "plain"


def main():
    args = sys.argv[1:]
    opt = {}
    for k in ("--src", "--out"):
        if k in args:
            i = args.index(k)
            opt[k] = args[i + 1]
            del args[i:i + 2]
    src = opt.get("--src", SRC)
    asm = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-fno-gpu-rdc",
                          "-fno-slp-vectorize", "-I", os.path.dirname(SRC), "-S", "--cuda-device-only", src, "-o", "-"],
                         capture_output=True, text=True, check=True).stdout
    lines = asm.split("\n")
    # default: the instantiation the headline runs, composite_bwd_tile_kernel<false, 512, false, 1, false, false>
    kname = args[0] if args else "_ZN4d3ga25composite_bwd_tile_kernelILb0ELi512ELb0ELi1ELb0ELb0E"
    start = next(i for i, l in enumerate(lines) if l.startswith(kname))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    body = lines[start:end]
    # Basic blocks and their loops from the compiler's annotations: a block header line (".LBB<f>_<n>:" or "; %bb.<n>:")
    # says "in Loop: Header=BB<f>_<h> Depth=d" or, for a loop header, "This [Inner ]Loop Header: Depth=d" (its own line may
    # follow), with "Parent Loop BB<f>_<p>" lines naming the enclosing loops.
    blocks, cur = [], None
    for l in body:
        m = re.match(r"^(?:\.LBB(\d+_\d+):|; %bb\.(\d+):)", l)
        if m:
            cur = {"name": "BB" + m.group(1) if m.group(1) else None, "loop": None, "depth": 0, "parents": [], "lines": []}
            blocks.append(cur)
        if cur is None:
            continue
        h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d)", l)
        if h:
            cur["loop"], cur["depth"] = h.group(1), int(h.group(2))
        h = re.search(r"This (?:Inner )?Loop Header: Depth=(\d)", l)
        if h:
            cur["loop"], cur["depth"] = cur["name"], int(h.group(1))
        h = re.search(r"Parent Loop (BB\d+_\d+) Depth=\d", l)
        if h:
            cur["parents"].append(h.group(1))
        cur["lines"].append(l)
    parent = {b["name"]: b["parents"][-1] if b["parents"] else None for b in blocks if b["loop"] == b["name"] and b["name"]}
    def chain(loop):
        out = []
        while loop:
            out.append(loop)
            loop = parent.get(loop)
        return out[::-1]                                     # outermost first
    loops = {}
    for bl in blocks:
        if bl["loop"]:
            loops.setdefault(bl["loop"], []).extend(bl["lines"])
    # the group loop = the first depth-1 loop that has child loops (the kernel has small depth-1 loops in front of it)
    group = next(b["name"] for b in blocks if b["loop"] == b["name"] and b["depth"] == 1 and b["name"] in parent.values())
    children = [b["name"] for b in blocks if b["loop"] == b["name"] and parent.get(b["name"]) == group]
    # the four-line pixel loop, if the lines are not unrolled: the first child loop, the one with the DPP scans
    pixel = children[0] if children and any("row_shr" in x for x in loops[children[0]]) else None
    counts = {"plain": 0, "dpp": 0, "trans": 0, "packed": 0, "vop3_other": 0}
    other = {"lds": 0, "vmem": 0, "salu": 0}
    for bl in blocks:
        ch = chain(bl["loop"]) if bl["loop"] else []
        if not ch or ch[0] != group or len(ch) >= 3:
            continue                                         # outside the group loop, or the rare displaced-record publish
        w = 4 if (len(ch) == 2 and ch[1] == pixel) else 1    # the insert loop: once per attempt
        for l in bl["lines"]:
            t = l.strip()
            if not t or t.startswith(";") or t.startswith(".") or t.endswith(":") or re.match(r"^\S+:\s*;", t):
                continue
            op = t.split()[0]
            c = classify(op, t)
            if c:
                counts[c] += w
            elif op.startswith("ds_"):
                other["lds"] += w
            elif op.startswith("global_"):
                other["vmem"] += w
            elif op.startswith("s_"):
                other["salu"] += w
    # groups per trip of the group loop (one insert loop each: the loop may be unrolled by two)
    per_trip = max(1, sum(1 for c in children if c != pixel))
    counts = {k: round(v / per_trip, 1) for k, v in counts.items()}
    other = {k: round(v / per_trip, 1) for k, v in other.items()}
    vgpr = re.search(r"\.name:\s+" + re.escape(body[0].split(":")[0]) + r"\n(?:(?!\.name:).)*?\.vgpr_count:\s+(\d+)", asm, re.S)
    out = {"kernel": body[0].split(":")[0], "unit": "instructions per 16-entry group (four block lines, one insert attempt)", "counts": counts,
           "non_valu": other, "vgpr_count": int(vgpr.group(1)) if vgpr else None,
           "note": "vop3_other is priced at the v_cndmask_b32_e64 / v_cmp_*_e64 / v_med3 / v_bfi rate measured by "
           "tools/micro/valu_issue.hip (1.9 ns vs 1.2 ns for v_fma_f32 at 8 waves/SIMD)", "vop3_other_cycles": 3.8}
    try:      # calibrated issue cycles per group (the costs bench.py's valu_issue_model uses)
        cal = {(r["kind"], r["waves_per_simd"]): r["cycles_per_wave_inst_per_simd"]
               for r in json.load(open(os.path.join(ROOT, "profiles", "r02_valu_issue_pmc.json")))}
        cost = {"plain": cal[("v_fma_f32", 8)], "dpp": cal[("v_add_f32_dpp", 8)], "trans": cal[("v_exp_f32", 8)],
                "packed": cal[("v_pk_fma_f32", 8)], "vop3_other": out["vop3_other_cycles"]}
        out["issue_cycles_per_group"] = round(sum(counts[k] * cost[k] for k in counts), 1)
    except (OSError, KeyError, ValueError):
        pass
    json.dump(out, open(opt.get("--out", os.path.join(ROOT, "profiles", "r07_composite_bwd_mix.json")), "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    sys.exit(main())
