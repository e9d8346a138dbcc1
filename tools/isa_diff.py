"""Compare the kernels of two `hipcc --save-temps` builds: for every kernel of the OLD assembly, is its instruction text (labels and
comments stripped) and its register count the same in the NEW one?  Kernels only in the new build are listed apart.  Kernels are
matched by demangled name with trailing `false` template arguments and a trailing `int4 const*` parameter (the windowed
variants' additions) removed, so that `k<a, b>(..)` of the old build meets `k<a, b, false>(.., int4 const*)` of the new one.

    python tools/isa_diff.py OLD.s NEW.s
"""
import re
import subprocess
import sys


def _key(names):
    dm = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    out = {}
    for n, d in zip(names, dm):
        k = d
        while True:
            k2 = re.sub(r", false>", ">", k)
            k2 = re.sub(r"^void (\S+)<false>\(", r"\1(", k2)
            k2 = re.sub(r", HIP_vector_type<int, 4u> const\*\)", ")", k2)
            if k2 == k:
                break
            k = k2
        out[n] = k
    return out


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\S+):[^\n]*$(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        lines = []
        for ln in body.splitlines():
            ln = ln.split(";")[0].strip()
            if not ln or ln.endswith(":") or ln.startswith("."):
                continue
            lines.append(re.sub(r"\.LBB\d+_\d+", "L", ln))
        out[name] = lines
    regs = {}
    for m in re.finditer(r"\.name:\s+(\S+)\s*\n(?:.*\n){0,12}?\s+\.sgpr_count:\s+(\d+)(?:.*\n){0,12}?\s+\.vgpr_count:\s+(\d+)", text):
        regs[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    return out, regs


def main(old, new):
    a, ra = kernels(old)
    b, rb = kernels(new)
    ka, kb = _key(list(a)), _key(list(b))
    a = {ka[n]: v for n, v in a.items()}
    ra = {ka[n]: v for n, v in ra.items() if n in ka}
    b = {kb[n]: v for n, v in b.items()}
    rb = {kb[n]: v for n, v in rb.items() if n in kb}
    same = diff = 0
    for name, body in a.items():
        if name not in b:
            print("MISSING in new:", name)
            diff += 1
        elif body != b[name] or ra.get(name) != rb.get(name):
            print("DIFFERS:", name, ra.get(name), rb.get(name))
            diff += 1
        else:
            same += 1
    added = sorted(set(b) - set(a))
    print(f"{same} kernels identical, {diff} differ; {len(added)} new kernels")
    for n in added:
        print("  new:", n, rb.get(n))
    return diff


if __name__ == "__main__":
    sys.exit(1 if main(sys.argv[1], sys.argv[2]) else 0)
