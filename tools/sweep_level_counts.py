#!/usr/bin/env python3
"""Static instruction counts of the tree sweeps of a fixed-layout step kernel, from the gfx950 assembly of smplsim_hip.hip
(hipcc <the flags of smplsim_amd/_lib.py> --cuda-device-only -S).

    python tools/sweep_level_counts.py KERNEL_SUBSTRING parent.s [change.s ...]

The kernel is cut at its wave barriers (the hand-offs of ss_wave_gpu.h sync()).  The sweep away from the root is the run of
segments that hold three 8-lane group sums each (9 DPP adds; 18 on the level of body 0): one segment per level.  Before it lie the
root block's two segments, and before those the sweep towards the root, two segments per level (part 1 | part 2); the leaf level's
part 1 shares its segment with the code before the solve and is left out, the root block's row gather closes the region, so the
region "towards the root" is part 2 of the leaf level, the other levels whole, and the root's rows.
Kinds: float (VALU float arithmetic without DPP), dpp, lds (ds_*), wait (s_waitcnt / s_nop), move (v_mov / v_cndmask),
scalar (s_* other than waits and exec-mask), exec (s_*_saveexec, writes of exec, s_cbranch_exec*), lane (v_readlane /
v_writelane: SGPR spills and reloads), vother (integer / compare / address VALU), mem (scratch / global)."""
import re
import sys

KINDS = ("float", "dpp", "lds", "wait", "move", "scalar", "exec", "lane", "vother", "mem")


def kernel_segments(path, sub):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and sub in l)
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".section"))
    segs, meta = [[]], {}
    for l in lines[start + 1:end]:
        if "wave barrier" in l:
            segs.append([])
            continue
        s = l.split(";")[0].strip()
        if s and not s.endswith(":") and not s.startswith("."):
            segs[-1].append(s)
    for l in lines[end:]:
        m = re.match(r"\s*;\s*(NumVgprs|NumSgprs|ScratchSize|Occupancy|codeLenInByte)\W+(\d+)", l)
        if m and m.group(1) not in meta:
            meta[m.group(1)] = int(m.group(2))
        if len(meta) == 5:
            break
    return segs, meta


def classify(i):
    op = i.split()[0]
    if "dpp" in i:
        return "dpp"
    if op.startswith("ds_"):
        return "lds"
    if op in ("s_waitcnt", "s_nop"):
        return "wait"
    if op.startswith("s_"):
        if "saveexec" in op or op.startswith("s_cbranch_exec") or re.match(r"s_\w+ exec\b", i):
            return "exec"
        return "scalar"
    if op.startswith(("v_mov", "v_cndmask", "v_accvgpr")):
        return "move"
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane"
    if re.search(r"_f32(_e32|_e64)?$", op) and not op.startswith("v_cmp"):
        return "float"
    if op.startswith(("scratch_", "global_", "buffer_", "flat_")):
        return "mem"
    return "vother"


def count(segs):
    c = {k: 0 for k in KINDS}
    for s in segs:
        for i in s:
            c[classify(i)] += 1
    return c


def fmt(c):
    return f"all {sum(c.values()):5d}  " + "  ".join(f"{k} {c[k]}" for k in KINDS)


def main():
    sub, paths = sys.argv[1], sys.argv[2:]
    for p in paths:
        segs, meta = kernel_segments(p, sub)
        ins = [i for s in segs for i in s]
        sums = [sum(i.startswith("v_add_f32_dpp") or (i.startswith("v_mov_b32_dpp")) for i in s) for s in segs]
        runs, k = [], 0
        while k < len(segs):
            j = k
            while j < len(segs) and sums[j] in (9, 18):
                j += 1
            if j - k >= 3:
                runs.append((k, j))
            k = max(j, k + 1)
        print(f"== {p}\n   kernel: {len(ins)} instructions  {meta}")
        print("   whole kernel: " + fmt(count(segs)))
        print(f"   v_readlane {sum(i.startswith('v_readlane') for i in ins)}  v_writelane {sum(i.startswith('v_writelane') for i in ins)}"
              f"  scratch_load {sum(i.startswith('scratch_load') for i in ins)}  scratch_store {sum(i.startswith('scratch_store') for i in ins)}")
        for a, b in runs:
            n = b - a
            up = segs[a - 2 - 2 * n:a - 2]
            print(f"   {n} levels; segment lengths towards the root {[len(s) for s in up]}, root {[len(s) for s in segs[a - 2:a]]}, away {[len(s) for s in segs[a:b]]}")
            print("   towards the root: " + fmt(count(up)))
            print("   away from the root: " + fmt(count(segs[a:b])))


if __name__ == "__main__":
    main()
