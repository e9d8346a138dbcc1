#!/usr/bin/env python3
"""Static instruction mix of the compositing forward (composite_fwd_q_kernel), the forward's sibling of isa_mix.py.

Cross-compiles d3ga_amd/csrc/raster_composite.hip to gfx950 assembly with build.py's flags (no GPU needed) and reports, for
every instantiation of composite_fwd_q_kernel, two regions:
  blend : the innermost loop that holds the v_exp_f32 pair (one iteration = two list positions x 64 pixels);
  batch : the rest of the loop around it (stage two, emission, fill / stage one, the next batch's gathers), every
          instruction counted once (the stage-one loop inside it too: one chunk);
and for each: VALU instructions by the issue classes tools/micro/valu_issue.hip measures (isa_mix.classify) with the
calibrated cycles of profiles/r02_valu_issue_pmc.json, the SALU count, and the LDS instructions by opcode with their
LDS-array cycles (the table below: one cycle per lane group of the instruction; stores additionally by their issue cost, which
the transfer of address and data sets).  Per kernel it also keeps the register counts, scratch, LDS bytes and occupancy the
compiler prints.

    python tools/isa_mix_fwd.py [--src FILE.hip] [--parent-src FILE.hip] [--out FILE.json] [--all]

Writes profiles/r08_composite_fwd_mix.json: the headline instantiation <false, false, true, false, false> in full ("new", and
"parent" when --parent-src names the parent commit's raster_composite.hip; its composite_common.h is taken from beside it),
and one summary line per instantiation.  tests/test_fwd_isa_host.py asserts on what analyse() returns.
"""
import importlib.util
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "d3ga_amd", "csrc")
SRC = os.path.join(CSRC, "raster_composite.hip")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_mix import classify  # noqa: E402  (the VALU issue classes are the backward tool's)

HEADLINE = (False, False, True, False, False)            # DUAL, DEPTH, L1V, PVB, WIN
# LDS-array cycles per wave-instruction (lane groups serviced one per cycle) and, for stores, the issue cycles (address + data
# transfer): the LDS table of the MI355X notes.  Reads cost their LDS-array cycles.
LDS_ARRAY = {"ds_read_u8": 2, "ds_read_i8": 2, "ds_read_u16": 2, "ds_read_i16": 2, "ds_read_u16_d16": 2, "ds_read_u16_d16_hi": 2,
             "ds_read_b32": 2, "ds_read_b64": 2, "ds_read_b96": 8, "ds_read_b128": 4, "ds_read2_b32": 4, "ds_read2_b64": 8,
             "ds_read2st64_b32": 4, "ds_read2st64_b64": 8,
             "ds_write_b8": 2, "ds_write_b16": 2, "ds_write_b32": 2, "ds_write_b64": 4, "ds_write_b96": 8, "ds_write_b128": 8,
             "ds_write2_b32": 4, "ds_write2_b64": 8, "ds_write2st64_b32": 4, "ds_write2st64_b64": 8}
LDS_STORE_ISSUE = {"ds_write_b8": 4, "ds_write_b16": 4, "ds_write_b32": 4, "ds_write_b64": 6, "ds_write_b96": 10, "ds_write_b128": 13,
                   "ds_write2_b32": 6, "ds_write2_b64": 13, "ds_write2st64_b32": 6, "ds_write2st64_b64": 13}
VOP3_OTHER_CYCLES = 3.8                                  # v_cndmask_b32_e64 / v_cmp_*_e64 / v_med3 / v_bfi (isa_mix.py)


def build_flags():
    """FLAGS + the per-source extras of d3ga_amd/csrc/build.py (read from it: one definition)."""
    spec = importlib.util.spec_from_file_location("_d3ga_build", os.path.join(CSRC, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.FLAGS) + list(mod.EXTRA.get("raster_composite.hip", []))


def compile_asm(src=SRC, hipcc=None):
    hipcc = hipcc or os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    inc = ["-I", os.path.dirname(os.path.abspath(src)), "-I", CSRC]      # a parent source brings its own composite_common.h
    return subprocess.run([hipcc] + build_flags() + inc + ["-S", "--cuda-device-only", src, "-o", "-"],
                          capture_output=True, text=True, check=True).stdout


def _cost_table():
    cal = {(r["kind"], r["waves_per_simd"]): r["cycles_per_wave_inst_per_simd"]
           for r in json.load(open(os.path.join(ROOT, "profiles", "r02_valu_issue_pmc.json")))}
    return {"plain": cal[("v_fma_f32", 8)], "dpp": cal[("v_add_f32_dpp", 8)], "trans": cal[("v_exp_f32", 8)],
            "packed": cal[("v_pk_fma_f32", 8)], "vop3_other": VOP3_OTHER_CYCLES}


def _instructions(lines):
    for l in lines:
        t = l.strip()
        if not t or t.startswith(";") or t.startswith(".") or t.endswith(":") or re.match(r"^\S+:\s*;", t):
            continue
        yield t.split()[0], t


def _region(lines, cost):
    valu = {"plain": 0, "dpp": 0, "trans": 0, "packed": 0, "vop3_other": 0}
    lds, salu, vmem, waits = {}, 0, 0, 0
    for op, t in _instructions(lines):
        c = classify(op, t)
        if c:
            valu[c] += 1
        elif op.startswith("ds_"):
            lds[op] = lds.get(op, 0) + 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            vmem += 1
        elif op == "s_waitcnt":
            waits += 1
        elif op.startswith("s_"):
            salu += 1
    unknown = sorted(op for op in lds if op not in LDS_ARRAY)
    out = {"valu": valu, "valu_total": sum(valu.values()), "salu": salu, "vmem": vmem, "s_waitcnt": waits, "lds": lds,
           "lds_insts": sum(lds.values()),
           "lds_array_cycles": sum(n * LDS_ARRAY.get(op, 0) for op, n in lds.items()),
           "lds_store_issue_cycles": sum(n * LDS_STORE_ISSUE[op] for op, n in lds.items() if op in LDS_STORE_ISSUE)}
    if unknown:
        out["lds_unpriced"] = unknown
    if cost:
        out["valu_issue_cycles"] = round(sum(valu[k] * cost[k] for k in valu), 1)
    return out


def split_kernels(asm):
    """{(DUAL, DEPTH, L1V, PVB, WIN): {"name", "body" (lines), "meta"}} for every composite_fwd_q_kernel in the assembly."""
    lines = asm.split("\n")
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_ZN4d3ga22composite_fwd_q_kernelI((?:Lb[01]E)+)E\S*):", l)
        if not m:
            continue
        end = next(j for j in range(i, len(lines)) if "s_endpgm" in lines[j])
        fend = next(j for j in range(end, len(lines)) if lines[j].startswith(".Lfunc_end"))
        tail = "\n".join(lines[fend:fend + 60])              # the compiler's resource comments behind the function
        meta = {}
        for key, pat in (("vgprs", r"; NumVgprs: (\d+)"), ("agprs", r"; NumAgprs: (\d+)"), ("sgprs", r"; NumSgprs: (\d+)"),
                         ("scratch", r"; ScratchSize: (\d+)"), ("occupancy", r"; Occupancy: (\d+)"), ("lds_bytes", r"; LDSByteSize: (\d+)")):
            f = re.search(pat, tail)
            meta[key] = int(f.group(1)) if f else None
        flags = tuple(b == "1" for b in re.findall(r"Lb([01])E", m.group(2)))
        out[flags] = {"name": m.group(1), "body": lines[i:end + 1], "meta": meta}
    return out


def loops_of(body):
    """Basic blocks with the compiler's loop annotations (as isa_mix.py reads them): blocks, parent-of-loop, lines-of-loop."""
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
    parent = {b["name"]: (b["parents"][-1] if b["parents"] else None) for b in blocks if b["loop"] == b["name"] and b["name"]}
    return blocks, parent


def analyse_kernel(k, cost=None):
    blocks, parent = loops_of(k["body"])

    def chain(loop):
        out = []
        while loop:
            out.append(loop)
            loop = parent.get(loop)
        return out[::-1]                                     # outermost first
    own = {}
    for b in blocks:
        if b["loop"]:
            own.setdefault(b["loop"], []).extend(b["lines"])
    inner = [h for h in own if h not in parent.values()]     # loops without child loops
    blend = [h for h in inner if sum(1 for op, _ in _instructions(own[h]) if op.startswith("v_exp_f32")) >= 2]
    if len(blend) != 1:
        raise RuntimeError("%s: %d candidate blend loops" % (k["name"], len(blend)))
    blend = blend[0]
    batch = chain(blend)[0]
    rest = [l for b in blocks if b["loop"] and chain(b["loop"])[0] == batch and b["loop"] != blend for l in b["lines"]]
    return {"kernel": k["name"], "meta": k["meta"], "blend": _region(own[blend], cost), "batch": _region(rest, cost),
            "whole_kernel": _region(k["body"], cost)}


def analyse(src=SRC, asm=None):
    """{flags: analysis} for every instantiation of composite_fwd_q_kernel in `src` (or in the given assembly text)."""
    try:
        cost = _cost_table()
    except (OSError, KeyError, ValueError):
        cost = None
    ks = split_kernels(asm if asm is not None else compile_asm(src))
    return {f: analyse_kernel(k, cost) for f, k in ks.items()}


def _summary(res):
    rows = []
    for f in sorted(res):
        a = res[f]
        rows.append({"DUAL,DEPTH,L1V,PVB,WIN": "".join("1" if b else "0" for b in f), "vgprs": a["meta"]["vgprs"], "scratch": a["meta"]["scratch"],
                     "occupancy": a["meta"]["occupancy"], "lds_bytes": a["meta"]["lds_bytes"], "blend_valu": a["blend"]["valu_total"],
                     "blend_valu_issue_cycles": a["blend"].get("valu_issue_cycles"), "blend_salu": a["blend"]["salu"],
                     "blend_lds": a["blend"]["lds"], "blend_lds_array_cycles": a["blend"]["lds_array_cycles"]})
    return rows


def main():
    args = sys.argv[1:]
    opt = {}
    for k in ("--src", "--parent-src", "--out"):
        if k in args:
            i = args.index(k)
            opt[k] = args[i + 1]
            del args[i:i + 2]
    new = analyse(opt.get("--src", SRC))
    out = {"unit": "instructions per blend-loop iteration (two list positions x 64 pixels) / per trip of the batch loop outside it (one stage-one chunk)",
           "lds_array_cycles_table": LDS_ARRAY, "lds_store_issue_cycles_table": LDS_STORE_ISSUE, "vop3_other_cycles": VOP3_OTHER_CYCLES,
           "headline": "composite_fwd_q_kernel<false, false, true, false, false>", "new": new[HEADLINE], "instantiations": _summary(new)}
    if "--parent-src" in opt:
        par = analyse(opt["--parent-src"])
        out["parent"] = par[HEADLINE]
        out["parent_instantiations"] = _summary(par)
    json.dump(out, open(opt.get("--out", os.path.join(ROOT, "profiles", "r08_composite_fwd_mix.json")), "w"), indent=1)
    show = {k: out[k] for k in ("parent", "new") if k in out}
    print(json.dumps({k: {r: v[r] for r in ("meta", "blend", "batch")} for k, v in show.items()}))
    if "--all" in args:
        for r in out["instantiations"]:
            print(json.dumps(r))


if __name__ == "__main__":
    sys.exit(main())
