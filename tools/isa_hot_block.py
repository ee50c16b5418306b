#!/usr/bin/env python3
"""tools/isa_hot_block.py -- basic blocks of one kernel in a gfx950 assembly listing, and the instruction mix of a chosen path
through them, with the kernel's register, scratch and occupancy figures.  The bucket accumulation's loop is a handful of blocks
(load and sign, the first half of the mixed addition up to the U2 == X1 test, the rest, the loop tail); their sum is the
per-addition instruction count.  A block is named by its label; the pieces a branch cuts it into get a ' each.

    hipcc <the Makefile's flags> --cuda-device-only -S -o msm.s mpc-jellyfish_amd/csrc/msm.hip
    python tools/isa_hot_block.py msm.s 'msm_accumulate_split_kernelINS_4EcFzINS_6BlsFqZEEELb0'                  # the block table
    python tools/isa_hot_block.py msm.s '<kernel>' ".LBB22_19,.LBB22_19',.LBB22_22"                               # mix of a path
"""
import collections
import re
import sys


def main():
    path, key = sys.argv[1], sys.argv[2]
    want = sys.argv[3].split(",") if len(sys.argv) > 3 else None
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if key in l and re.match(r"^_Z\w+:", l))
    name = lines[start].split(":")[0]
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    blocks, cur, lab = [], [], "entry"
    for l in lines[start + 1:end]:
        s = l.strip()
        if not s or s.startswith(";"):
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            blocks.append((lab, cur))
            cur, lab = [], m.group(1)
            continue
        if s.startswith("."):
            continue
        cur.append(s)
        if s.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
            blocks.append((lab, cur))
            cur, lab = [], lab + "'"
    blocks.append((lab, cur))
    print("kernel %s" % name)
    for l in lines[end:end + 60]:                                  # the compiler's summary comments after the code
        m = re.match(r"^; (NumVgprs|NumAgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize|codeLenInByte)\s*[:=]\s*(\S+)", l)
        if m:
            print("  %-16s %s" % (m.group(1), m.group(2)))
    if want is None:
        print("  %-16s %6s %6s %6s  %s" % ("block", "insts", "VALU", "MADs", "ends with"))
        for lab, c in blocks:
            if c:
                print("  %-16s %6d %6d %6d  %s" % (lab, len(c), sum(x.startswith("v_") for x in c), sum(x.startswith("v_mad_") for x in c), c[-1][:48]))
        return
    d = dict(blocks)
    mix = collections.Counter()
    for lab in want:
        mix.update(x.split()[0] for x in d[lab])
    valu = sum(n for op, n in mix.items() if op.startswith("v_"))
    print("  path %s" % " ".join(want))
    print("  %d instructions, %d of them VALU" % (sum(mix.values()), valu))
    for op, n in mix.most_common():
        print("    %-24s %5d" % (op, n))


if __name__ == "__main__":
    main()
