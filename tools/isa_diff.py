#!/usr/bin/env python3
"""Development aid for refactors: per-kernel comparison of gfx950 assembly listings (hipcc --cuda-device-only -S).
Usage: isa_diff.py OLD.s NEW.s [NEW2.s ...]   (the NEW listings are taken together: a file that was split)
Per kernel of OLD: whether the instruction stream is identical (block labels renumbered in order of appearance, comments dropped)
and the VGPR / scratch / LDS figures of both sides."""
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for name, meta in re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, flags=re.S):
        body = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)\n\s*s_endpgm", text, flags=re.S | re.M).group(1)
        labels, code = {}, []
        for ln in body.splitlines():
            ln = ln.split(";")[0].strip()
            if ln and not ln.startswith(".p2align"):
                code.append(re.sub(r"\.LBB\d+_\d+", lambda t: labels.setdefault(t.group(0), ".L%d" % len(labels)), ln))
        res = {k: int(re.search(r"\.amdhsa_" + k + r" (\d+)", meta).group(1))
               for k in ("next_free_vgpr", "private_segment_fixed_size", "group_segment_fixed_size")}
        out[name] = (code, res)
    return out


old = kernels(sys.argv[1])
new = {}
for p in sys.argv[2:]:
    new.update(kernels(p))
print("# kernel | stream | vgpr scratch lds (old -> new)")
for name in sorted(set(old) | set(new)):
    if name not in old or name not in new:
        side = old if name in old else new
        print(name, "| only in", "old" if name in old else "new", "|", " ".join("%d" % v for v in side[name][1].values()))
        continue
    (co, ro), (cn, rn) = old[name], new[name]
    same = "identical" if co == cn else "differs (%d -> %d instructions)" % (len(co), len(cn))
    fig = " ".join("%d" % ro[k] if ro[k] == rn[k] else "%d->%d" % (ro[k], rn[k]) for k in ro)
    print(name, "|", same, "|", fig)
