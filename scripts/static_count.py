#!/usr/bin/env python3
"""Static instruction counts of one kernel in a gfx950 assembly file.

  python scripts/static_count.py file.s KERNEL_SUBSTRING

The assembly is that of `hipcc -S --cuda-device-only` with build.py's flags.
Prints the kernel's VALU / SALU / branch / vector-memory / LDS / scalar-load
instructions and its basic blocks: every block, cold ones included, so a
difference between two builds is one of code size, not of executed
instructions (those are the SQ_INSTS_* counters of scripts/gpu_mem.sh).
"""
import re
import sys
from collections import Counter


def klass(op):
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith(("s_waitcnt", "s_nop", "s_endpgm", "s_setprio", "s_sleep", "s_barrier", "s_code_end")):
        return "other"
    if op.startswith("s_"):
        return "smem" if op.startswith(("s_load", "s_buffer_load")) else "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("v_"):
        return "valu"
    return "other"


def main():
    path, kern = sys.argv[1], sys.argv[2]
    inside, total, blocks = False, Counter(), 1
    for line in open(path, errors="replace"):
        s = line.strip()
        if not inside:
            inside = bool(re.match(r"^\S+:", line)) and kern in line
            continue
        if s.startswith(".Lfunc_end"):
            break
        if re.match(r"^\.LBB\d+_\d+:", s):
            blocks += 1
        elif s and not s.startswith((".", ";")):
            total[klass(s.split()[0])] += 1
    print(f"{kern}: " + " ".join(f"{k} {total[k]}" for k in ("valu", "salu", "branch", "vmem", "lds", "smem"))
          + f" blocks {blocks}")


if __name__ == "__main__":
    main()
