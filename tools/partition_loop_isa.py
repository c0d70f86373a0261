#!/usr/bin/env python3
"""Instruction counts of the pair partition loop (seg2_nth_slots) of one kernel
in a gfx950 assembly listing, by class.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off \
        -mllvm -amdgpu-set-wave-priority -S --cuda-device-only \
        -Rpass-analysis=kernel-resource-usage -I hmc_amd/csrc \
        hmc_amd/csrc/estep_split.hip -o split.s 2> split.rpass
  python3 tools/partition_loop_isa.py split.s \
        _ZN3hmc12estep_valuesILb0ELi4ELb0ELb1ELi10EEEvNS_9ValueArgsE [--dump]

The loop is found from the compiler's own block annotations ("in Loop:
Header=..."): the loop of the first block that holds the median's f64
compares and at least six v_bcnt_u32_b32 (the stop ranks and K).  Every
instruction of its blocks counts, waits, nops and branches included; labels,
comments and directives do not.
"""
import re
import sys


def partition_loop(path, func):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(func + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    blocks, cur = [], None
    for l in lines[start:end]:
        m = re.match(r"^\.(LBB\d+_\d+):\s*(;.*)?$", l)
        if m:
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", l)
            cur = [m.group(1)[1:], h.group(1) if h else None, []]
            blocks.append(cur)
            continue
        if cur is None:
            continue
        if cur[1] is None and re.search(r"^\s*;\s+(Parent Loop|=>)", l):
            cur[1] = cur[0]  # a loop header: the annotation follows its label
        cur[2].append(l)
    hdr = next(h for _, h, ls in blocks
               if sum("v_bcnt_u32_b32" in s for s in ls) >= 6 and any("v_cmp_gt_f64" in s for s in ls))
    return [b for b in blocks if b[1] == hdr or b[0] == hdr]


def classify(blocks):
    cnt = dict(total=0, valu=0, salu=0, ds=0, s_nop=0, s_waitcnt=0, branch=0, saveexec=0, scratch=0, other=0)
    for _, _, ls in blocks:
        for s in ls:
            s = s.split(";")[0].strip()
            if not s or s.endswith(":") or s.startswith("."):
                continue
            op = s.split()[0]
            cnt["total"] += 1
            if op == "s_nop":
                cnt["s_nop"] += 1
            elif op == "s_waitcnt":
                cnt["s_waitcnt"] += 1
            elif op.startswith(("s_cbranch", "s_branch")):
                cnt["branch"] += 1
            elif op.startswith(("scratch_", "buffer_")):
                cnt["scratch"] += 1
            elif op.startswith("ds_"):
                cnt["ds"] += 1
            elif op.startswith("v_"):
                cnt["valu"] += 1
            elif op.startswith("s_"):
                cnt["salu"] += 1
                cnt["saveexec"] += "saveexec" in op
            else:
                cnt["other"] += 1
    return cnt


def main():
    path, func = sys.argv[1], sys.argv[2]
    blocks = partition_loop(path, func)
    print(func, [b[0] for b in blocks], classify(blocks))
    if "--dump" in sys.argv:
        for lab, _, ls in blocks:
            print("." + lab + ":")
            print("\n".join(l for l in ls if not l.strip().startswith(";")))


if __name__ == "__main__":
    main()
