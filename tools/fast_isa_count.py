#!/usr/bin/env python3
"""Static instruction counts of fast_kernel's basic blocks.

    hipcc --offload-arch=gfx950 <the flags of __graft_entry__.HIPCC_FLAGS without -shared -fPIC>
          --offload-device-only -S -o a.s orbslam_mapsave_amd/csrc/orbfe_lib.hip
    tools/fast_isa_count.py [-v] a.s [b.s ...]

For both instantiations (<48>: the compile-time ROI pitch, <0>: the runtime pitch): VALU, DS
(LDS), SALU and global-memory instructions of the whole kernel and of its parts, a part being
the basic blocks that hold its marker instruction (profiles/fast_issue/README.md):

    prologue   everything before the loop over the two thresholds (cell and level loads, ROI
               staging, score-plane zeroing, lane layout)
    sweep      the pre-test (v_lerp_u8) and the list writes behind it (v_mbcnt)
    score      the arcs of fast_S (v_pk_minimum3_f16); one block per copy of the score loop
    nms        the 3x3 neighbour maximum of fast_emit (v_max3); one block per copy
    flush      the other blocks inside the sweep loop: the overflow flush without its scoring
    rest       the compaction pass of fast_emit, key stores, loop heads, the epilogue

-v lists every basic block.  The kernel descriptor's registers, LDS and scratch are printed with
the totals."""
import re
import sys
from collections import Counter

PARTS = ("prologue", "sweep", "score", "nms", "flush", "rest")


def kernel(lines, sym):
    start = [i for i, l in enumerate(lines) if l.startswith(sym + ":")][0]
    out, desc = [], {}
    for l in lines[start:]:
        if ".amdhsa_kernel" in l:
            break
        t = l.split(";")[0].strip()
        if t and (not t.startswith(".") or t.startswith(".LBB")):
            out.append(t)
    on = False
    for l in lines[start:]:
        if l.strip().startswith(".amdhsa_kernel"):
            on = sym in l
        elif on and ".end_amdhsa_kernel" in l:
            break
        elif on:
            m = re.match(r"\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|group_segment_fixed_size|"
                         r"private_segment_fixed_size)\s+(\S+)", l)
            if m:
                desc[m.group(1)] = m.group(2)
    return out, desc


def classify(op):
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "DS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    if op.startswith("s_waitcnt") or op == "s_nop" or op.startswith("s_endpgm"):
        return None
    if op.startswith(("s_load", "s_buffer_load")):
        return "SMEM"
    if op.startswith("s_"):
        return "SALU"
    return None


def blocks_of(ins):
    blocks, cur, name = [], [], "entry"
    for t in ins:
        if t.endswith(":"):
            if cur:
                blocks.append((name, cur))
            cur, name = [], t[:-1]
            continue
        cur.append(t)
        if re.match(r"s_c?branch", t):
            blocks.append((name, cur))
            cur, name = [], name + "+"
    if cur:
        blocks.append((name, cur))
    return blocks


def analyse(path, kp, verbose):
    lines = open(path).read().split("\n")
    sym = f"_ZN5orbfe11fast_kernelILi{kp}EEEvNS_8FastArgsE"
    ins, desc = kernel(lines, sym)
    blocks = blocks_of(ins)
    # the loops (backward branches) that hold the pre-test: the smallest is the sweep loop,
    # the largest the loop over the two thresholds
    lab = {name: i for i, (name, _) in enumerate(blocks)}
    lerp = next(i for i, (_, b) in enumerate(blocks) if any(t.startswith("v_lerp_u8") for t in b))
    spans = []
    for i, (_, b) in enumerate(blocks):
        m = re.match(r"s_c?branch\S*\s+(\.LBB\d+_\d+)", b[-1])
        if m and lab.get(m.group(1), 1 << 30) <= lerp <= i:
            spans.append((lab[m.group(1)], i))
    sweep_loop = min(spans, key=lambda r: r[1] - r[0])
    pass_head = min(r[0] for r in spans)
    parts = {p: Counter() for p in PARTS}
    total = Counter()
    rows = []
    for i, (name, b) in enumerate(blocks):
        ops = [t.split()[0] for t in b]
        c = Counter(k for k in map(classify, ops) if k)
        if any(o.startswith(("v_lerp_u8", "v_mbcnt")) for o in ops):
            part = "sweep"
        elif any(o.startswith("v_pk_minimum3") for o in ops):
            part = "score"
        elif any(o.startswith("v_max3") for o in ops):
            part = "nms"
        elif i < pass_head:
            part = "prologue"
        elif sweep_loop[0] <= i <= sweep_loop[1]:
            part = "flush"
        else:
            part = "rest"
        parts[part] += c
        parts[part]["blocks"] += 1
        total += c
        rows.append((name.replace(sym, "entry"), part, c))
    print(f"{path} fast_kernel<{kp}>: VALU {total['VALU']} DS {total['DS']} SALU {total['SALU']} "
          f"VMEM {total['VMEM']} | vgpr {desc.get('next_free_vgpr')} lds {desc.get('group_segment_fixed_size')} "
          f"(+ dynamic) scratch {desc.get('private_segment_fixed_size')}")
    for p in PARTS:
        c = parts[p]
        print(f"    {p:9s} blocks {c['blocks']:3d}  VALU {c['VALU']:4d}  DS {c['DS']:3d}  SALU {c['SALU']:4d}  VMEM {c['VMEM']:3d}")
    if verbose:
        for name, part, c in rows:
            print(f"        {name:14s} {part:9s} VALU {c['VALU']:3d} DS {c['DS']:3d} SALU {c['SALU']:3d} VMEM {c['VMEM']:3d}")


if __name__ == "__main__":
    args = sys.argv[1:]
    verbose = "-v" in args
    for path in (a for a in args if a != "-v"):
        for kp in (48, 0):
            analyse(path, kp, verbose)
