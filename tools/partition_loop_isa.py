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


GROUPS = ("pop", "extend", "prologue", "heap test", "heap path", "tail", "chain end")


def step_body(path, func):
    """The basic blocks of phase B's step loop (the loop around the partition
    loop) outside the partition loop, in layout order, each with a group.

    The groups follow from landmarks of the listing, in layout order:
      pop        from the loop header to where its whole-wave skip lands (the
                 first conditional branch: no segment is idle)
      extend     from there to the last labelled block before v_ffbh_u32
                 (lg2_floor of the selection's depth budget; that block opens
                 with the exec restore of the extends)
      prologue   that block up to the partition loop
      heap test  behind the partition loop, through the block with the
                 whole-wave skip of the heap path
      heap path  from there to where that skip lands (std::__heap_select and
                 iter_swap on one lane: runs only when a segment spent its depth)
      tail       from there to where the tail's own whole-wave skip lands
      chain end  the rest (it holds the loop's only HBM stores)
    Each block is printed with its landmarks so the grouping can be checked."""
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(func + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    blocks, cur = [], None
    for l in lines[start:end]:
        m = re.match(r"^\.(LBB\d+_\d+):\s*(;.*)?$", l) or re.match(r"^; %bb\.(\d+):\s*(;.*)?$", l)
        if m:
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", l)
            name = m.group(1)[1:] if m.group(1).startswith("L") else "bb." + m.group(1)
            cur = dict(name=name, loop=h.group(1) if h else None, ins=[], hdr=False)
            blocks.append(cur)
            continue
        if cur is None:
            continue
        if re.search(r"^\s*;\s+(Parent Loop|=>)", l):
            cur["hdr"] = True
            cur["loop"] = cur["name"]
            continue
        s = l.split(";")[0].strip()
        if s and not s.endswith(":") and not s.startswith("."):
            cur["ins"].append(s)
    part = partition_loop(path, func)
    phdr = next(b[1] or b[0] for b in part)
    pnames = {b["name"] for b in blocks if b["loop"] == phdr} | {b[0] for b in part}
    # a header's own "in Loop" is not printed: the step loop is the loop of the
    # last block before the partition loop that is not part of it
    idx = {b["name"]: i for i, b in enumerate(blocks)}
    step = next(b["loop"] for b in reversed(blocks[:idx[phdr]]) if b["name"] not in pnames)
    first = idx[step]
    last = max(i for i, b in enumerate(blocks) if b["loop"] == step)
    body = blocks[first:last + 1]

    def has(b, *ops):
        return any(s.split()[0].startswith(ops) for s in b["ins"])

    def target(b):
        """Label the block's first conditional branch goes to."""
        t = next((s.split()[1] for s in b["ins"] if s.startswith("s_cbranch")), None)
        if t is None:
            raise SystemExit(f"{func}: block {b['name']} was expected to hold a whole-wave skip (s_cbranch_*) and has none: "
                             "the listing's layout changed, regroup by hand from --dump")
        return t.lstrip(".").lstrip("L")

    # every group but the first starts where a whole-wave skip lands
    extend_at = target(body[0])                       # no idle segment: past the pop
    ffbh = next((i for i, b in enumerate(body) if has(b, "v_ffbh")), None)
    if ffbh is None:
        raise SystemExit(f"{func}: no v_ffbh_u32 (the depth budget's lg2_floor) in the step loop {step}: "
                         "the prologue cannot be told from the extends")
    prologue_at = next(body[i]["name"] for i in range(ffbh, -1, -1) if body[i]["name"].startswith("BB"))
    out, state = [], "pop"
    after_part, tested, tail_at, end_at = False, False, None, None
    for i, b in enumerate(body):
        if b["name"] in pnames:
            after_part, state = True, "heap test"
            continue
        if not after_part:
            if b["name"] == extend_at:
                state = "extend"
            if b["name"] == prologue_at:
                state = "prologue"
        else:
            if b["name"] == tail_at:
                state, end_at = "tail", target(b)     # no window to sort: past the tail
            elif b["name"] == end_at:
                state = "chain end"
            elif state == "heap test" and tested:
                state = "heap path"
            if state == "heap test" and has(b, "v_cmp") and any(s.startswith("s_cbranch") for s in b["ins"]):
                tested, tail_at = True, target(b)     # no heap segment: past the heap path
        out.append((b, state))
    missing = [g for g in ("extend", "prologue", "heap test", "tail", "chain end") if g not in {g for _, g in out}]
    if missing:
        raise SystemExit(f"{func}: no block was grouped as {missing}: a skip of the step loop {step} does not land where "
                         "the grouping expects it")
    return out


def print_step_body(path, func):
    rows = step_body(path, func)
    keys = ("total", "valu", "salu", "ds", "vmem", "s_waitcnt", "s_nop", "branch", "scratch")
    print(func)
    print("%-10s %-9s " % ("group", "block") + " ".join("%6s" % k.replace("s_waitcnt", "wait").replace("s_nop", "nop")
                                                         for k in keys) + "  landmarks")
    sums = {g: dict.fromkeys(keys, 0) for g in GROUPS}
    for b, g in rows:
        c = classify([(b["name"], None, b["ins"])])
        c["vmem"] = c.pop("other")
        marks = sorted({s.split()[0] for s in b["ins"]
                        if s.split()[0].startswith(("global_", "flat_", "ds_add", "ds_write_b64", "v_mul_f64", "v_ffbh",
                                                    "v_cmp_gt_f64", "ds_bpermute", "scratch_"))})
        print("%-10s %-9s " % (g, b["name"]) + " ".join("%6d" % c[k] for k in keys) + "  " + " ".join(marks))
        for k in keys:
            sums[g][k] += c[k]
    print()
    for g in GROUPS:
        print("%-20s " % g + " ".join("%6d" % sums[g][k] for k in keys))
    once = [g for g in GROUPS if g != "heap path"]
    print("%-20s " % "all but heap path" + " ".join("%6d" % sum(sums[g][k] for g in once) for k in keys))
    print("%-20s " % "partition loop" + " ".join(
        "%6d" % {**classify(partition_loop(path, func)), "vmem": 0}.get(k, 0) for k in keys))


def main():
    path, func = sys.argv[1], sys.argv[2]
    if "--step-body" in sys.argv:
        print_step_body(path, func)
        return
    blocks = partition_loop(path, func)
    print(func, [b[0] for b in blocks], classify(blocks))
    if "--dump" in sys.argv:
        for lab, _, ls in blocks:
            print("." + lab + ":")
            print("\n".join(l for l in ls if not l.strip().startswith(";")))


if __name__ == "__main__":
    main()
