#!/usr/bin/env python3
"""Static counts on the interior-keypoint path of describe_kernel's keypoint loop.

    hipcc --offload-arch=gfx950 <the flags of __graft_entry__.HIPCC_FLAGS without -shared -fPIC>
          --offload-device-only -S -o a.s orbslam_mapsave_amd/csrc/orbfe_lib.hip
    tools/describe_isa_count.py a.s [b.s ...]

For every matrix-core instantiation: the keypoint loop (the backward branch that spans the most
MFMAs), its instructions minus the basic blocks of the byte-gather window loads (those holding
global_load_ubyte) and minus the x86 rounding fix-up (one tie test per window: the second,
fix-up pass behind it; a tie test per tile: the blocks holding v_bfe_u32), and the static VALU
count outside the loop (profiles/describe_issue/README.md)."""
import re
import sys
from collections import Counter


def kernel(lines, sym):
    start = [i for i, l in enumerate(lines) if l.startswith(sym + ":")][0]
    out = []
    for l in lines[start:]:
        if ".amdhsa_kernel" in l:
            break
        t = l.split(";")[0].strip()
        if t and (not t.startswith(".") or t.startswith(".LBB")):
            out.append(t)
    return out


def analyse(path, g, x):
    lines = open(path).read().split("\n")
    sym = f"_ZN5orbfe15describe_kernelILi{g}ELb{x}ELi2EEEvNS_8DescArgsE"
    ins = kernel(lines, sym)
    lab = {t[:-1]: i for i, t in enumerate(ins) if t.endswith(":")}
    # keypoint loop = backward branch span with most MFMAs
    loops = []
    for i, t in enumerate(ins):
        m = re.match(r"s_c?branch\S*\s+(\.LBB\d+_\d+)", t)
        if m and lab.get(m.group(1), 1 << 30) <= i:
            loops.append((lab[m.group(1)], i))
    a, b = max(loops, key=lambda r: sum(1 for t in ins[r[0]:r[1]] if t.startswith("v_mfma")))
    # basic blocks
    blocks, cur = [], []
    for i in range(a, b + 1):
        t = ins[i]
        if t.endswith(":"):
            if cur:
                blocks.append(cur)
            cur = []
            continue
        cur.append(i)
        if re.match(r"s_c?branch", t):
            blocks.append(cur)
            cur = []
    if cur:
        blocks.append(cur)
    drop = set()
    for blk in blocks:
        if any(ins[i].startswith("global_load_ubyte") for i in blk):
            drop.update(blk)
    # result: one tie test per window, then a branch over the fix-up pass
    ties = [i for i in range(a, b + 1) if ins[i].startswith("v_cmp_eq_u16")]
    if len(ties) == 1:
        j = ties[0]
        while not ins[j].startswith("s_cbranch_vccz"):
            j += 1
        tgt = lab[re.match(r"s_cbranch_vccz\s+(\S+)", ins[j]).group(1)]
        drop.update(range(j + 1, tgt))
    else:
        for blk in blocks:
            if any(ins[i].startswith("v_bfe_u32") for i in blk):
                drop.update(blk)
    c = Counter()
    for i in range(a, b + 1):
        t = ins[i]
        if i in drop or t.endswith(":"):
            continue
        op = t.split()[0]
        if op.startswith("v_mfma"):
            c["MFMA"] += 1
        elif op.startswith("v_"):
            c["VALU"] += 1
            if op.startswith("v_mov"):
                c["moves"] += 1
            if op.startswith("v_cmp"):
                c["compares"] += 1
        elif op == "s_nop":
            c["s_nop"] += 1
        elif re.match(r"s_c?branch", op):
            c["branches"] += 1
        elif op.startswith("s_waitcnt"):
            pass
        elif op.startswith("s_"):
            c["SALU"] += 1
    outside = Counter()
    for i, t in enumerate(ins):
        if a <= i <= b or t.endswith(":"):
            continue
        op = t.split()[0]
        if op.startswith("v_") and not op.startswith("v_mfma"):
            outside["VALU"] += 1
    nl = sum(1 for t in ins[a:b + 1] if t == "s_nop" or t.startswith("s_nop"))
    return c, outside["VALU"], nl


if __name__ == "__main__":
    for path in sys.argv[1:]:
        for g, x in ((8, 1), (2, 1), (16, 1), (8, 0), (2, 0)):
            c, out, nl = analyse(path, g, x)
            print(f"{path:12s} <{g},{'true' if x else 'false'},2> interior: VALU {c['VALU']} MFMA {c['MFMA']} moves {c['moves']} "
                  f"compares {c['compares']} s_nop {c['s_nop']} branches {c['branches']} SALU {c['SALU']} | loop s_nop total {nl} | outside-loop VALU (static) {out}")
