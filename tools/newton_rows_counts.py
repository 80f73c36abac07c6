#!/usr/bin/env python3
"""Static instruction counts of the code around the articulated-body solve of a Newton iteration, from the gfx950 assembly of a step
translation unit (hipcc <the flags of smplsim_amd/_lib.py> --cuda-device-only -S).

    python tools/newton_rows_counts.py KERNEL_SUBSTRING parent.s [change.s ...]

The kernel is cut at its wave barriers as tools/sweep_level_counts.py does, and the solve is found the same way (the run of segments
with three 8-lane group sums each is the sweep away from the root).  Around it:
  prepare   the segment that ends at newton_prepare's hand-off (contact forces and K_b, joint part of the right-hand side); it begins
            at the hand-off before it, so it also holds the few instructions between the loop's back edge and newton_prepare
  finish    the segment behind the last level of the sweep away from the root, up to newton_finish's hand-off: eval_rows, the sums
            of delta . gradient, the line search, the update.  (The rare non-finite exit's own hand-off is laid out elsewhere.)
  tail      the segment behind that hand-off, up to the next one (the loop's back edge lies in it)
Kinds as in sweep_level_counts.py.  "waits before the first wave sum": s_waitcnt instructions that wait for LDS (lgkmcnt) in the
finish segment ahead of its first row_bcast DPP add, that is the LDS round trips in front of the first wave-wide sum."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sweep_level_counts import count, fmt, kernel_segments  # noqa: E402


def solve_run(segs):
    sums = [sum(i.startswith(("v_add_f32_dpp", "v_mov_b32_dpp")) for i in s) for s in segs]
    best, k = None, 0
    while k < len(segs):
        j = k
        while j < len(segs) and sums[j] in (9, 18):
            j += 1
        if j - k >= 3 and (best is None or j - k > best[1] - best[0]):
            best = (k, j)
        k = max(j, k + 1)
    return best


def waits_before_first_sum(seg):
    n = 0
    for i in seg:
        if "row_bcast" in i:
            break
        n += i.startswith("s_waitcnt") and "lgkmcnt" in i
    return n


def main():
    sub, paths = sys.argv[1], sys.argv[2:]
    for p in paths:
        segs, meta = kernel_segments(p, sub)
        a, b = solve_run(segs)
        n = b - a
        prepare, finish, tail = segs[a - 2 - 2 * n - 1], segs[b], segs[b + 1]
        print(f"== {p}\n   kernel: {sum(len(s) for s in segs)} instructions  {meta}")
        for name, seg in (("prepare", prepare), ("finish", finish), ("tail", tail)):
            print(f"   {name:8s}" + fmt(count([seg])))
        br = sum(bool(re.match(r"s_cbranch", i)) for i in finish)
        print(f"   finish: branches {br}  s_waitcnt {sum(i.startswith('s_waitcnt') for i in finish)}"
              f"  of them lgkmcnt(0) {sum(i.startswith('s_waitcnt') and 'lgkmcnt(0)' in i for i in finish)}"
              f"  waits before the first wave sum {waits_before_first_sum(finish)}"
              f"  scratch {sum(i.startswith('scratch_') for i in prepare + finish + tail)}")


if __name__ == "__main__":
    main()
