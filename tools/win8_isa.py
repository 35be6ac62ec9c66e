#!/usr/bin/env python3
"""What the compiler made of the chunk walk of every spmv_win8_kernel instance: VGPRs, scratch, and inside the walk's loop (the
backward-branch region of the kernel with the most stream loads) the vmcnt waits, the number of v_mov and the loads.  Reads the gfx950 assembly
that `hipcc --save-temps -c basic_iterative_solvers_amd/csrc/bis_spmv_win8.hip` leaves (no GPU needed).
    python tools/win8_isa.py bis_spmv_win8-hip-amdgcn-amd-amdhsa-gfx950.s [filter]"""
import re
import subprocess
import sys

path = sys.argv[1]
flt = sys.argv[2] if len(sys.argv) > 2 else ""
text = open(path).read()
# a function: "<sym>:" ... ".end_amdhsa_kernel" block follows with the register counts
funcs = re.split(r"\n\s*\.globl\s+", text)[1:]
rows = []
for f in funcs:
    sym = f.split("\n", 1)[0].split()[0]
    if "spmv_win8_kernel" not in sym:
        continue
    name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
    m = re.search(r"spmv_win8_kernel<(.*?)>\(", name)
    inst = m.group(1) if m else name
    if flt and flt not in inst:
        continue
    body = f.split(".end_amdhsa_kernel")[0]
    lines = body.split("\n")
    labels = {}
    for i, l in enumerate(lines):
        mm = re.match(r"^(\.LBB\d+_\d+):", l)
        if mm:
            labels[mm.group(1)] = i
    best = None  # the backward-branch region with the most non-temporal (stream) loads; ties: the shortest
    def key(span):
        return (sum(1 for l in lines[span[0]:span[1] + 1] if re.match(r"\s+global_load.*\bnt\b", l)), span[0] - span[1])
    for i, l in enumerate(lines):
        mm = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if mm and mm.group(1) in labels and labels[mm.group(1)] < i:
            span = (labels[mm.group(1)], i)
            if best is None or key(span) > key(best):
                best = span
    loop = lines[best[0]:best[1] + 1] if best else []
    waits = [re.search(r"vmcnt\((\d+)\)", l).group(1) for l in loop if "s_waitcnt" in l and "vmcnt" in l]
    movs = sum(1 for l in loop if re.match(r"\s+v_mov_b(32|64)(_e32|_e64)?\s+v", l) and re.search(r",\s*v\[?\d", l))
    loads = sum(1 for l in loop if re.match(r"\s+global_load", l))
    vg = re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", f)
    ag = re.search(r"\.amdhsa_accum_offset\s+(\d+)", f)
    sc = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", f)
    rows.append((inst, vg.group(1) if vg else "?", ag.group(1) if ag else "?", sc.group(1) if sc else "?",
                 len(loop), loads, ",".join(waits), movs))
print("instance <MODE, R, D, IMPL, VT, TWO> | next_free_vgpr | accum_offset | scratch | loop insns | loads | vmcnt waits in loop | v_mov of VGPRs in loop")
for r in sorted(rows):
    print(" | ".join(str(x) for x in r))
