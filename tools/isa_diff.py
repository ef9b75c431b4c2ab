#!/usr/bin/env python3
"""Compare two device-only assembly files of liborbfe's translation unit, kernel by kernel.

    hipcc --offload-arch=gfx950 <the flags of __graft_entry__.HIPCC_FLAGS without -shared -fPIC>
          --offload-device-only -S -o a.s orbslam_mapsave_amd/csrc/orbfe_lib.hip
    tools/isa_diff.py a.s b.s

A refactor that moves launch sites changes the order in which the templates are instantiated,
and with it the order of the kernels in the file and the function index k of the local labels
(.LBB<k>_<n>, .Lfunc_end<k>).  So the comparison is per kernel symbol, with that index and the
assembler comments removed: for every kernel, its instruction stream (from its label
to its .amdhsa_kernel block) and that block (registers, LDS, scratch, kernarg size) must be the
same text.  Prints the kernels that differ
and exits 1 if there are any or if the two sets of symbols differ.
"""
import hashlib
import re
import sys

LOCAL = re.compile(r"(\.LBB|\.LJTI|\.Lfunc_end|\.Lfunc_begin|\bBB)\d+")


def kernels(path):
    """{symbol: (instruction text, .amdhsa block text)}"""
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))]
    want = set(names)
    out = {n: ["", ""] for n in names}
    i = 0
    while i < len(lines):
        l = lines[i]
        m = re.match(r"(\S+):\s*(;.*)?$", l)
        if m and m.group(1) in want and not out[m.group(1)][0]:
            j = i + 1
            while ".amdhsa_kernel" not in lines[j]:
                j += 1
            # comments (loop notes, padded to a column that moves with k's digits) are not code
            out[m.group(1)][0] = "\n".join(LOCAL.sub(r"\1", x.split(";")[0].rstrip()) for x in lines[i:j])
            i = j - 1
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            j = i
            while ".end_amdhsa_kernel" not in lines[j]:
                j += 1
            out[m.group(1)][1] = "\n".join(lines[i:j + 1])
            i = j
        i += 1
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    for p in sys.argv[1:3]:
        print(f"{hashlib.sha256(open(p, 'rb').read()).hexdigest()}  {p}")
    print(f"kernels: {len(a)} / {len(b)}")
    only = sorted(set(a) ^ set(b))
    for n in only:
        print(f"only in {'first' if n in a else 'second'}: {n}")
    differ = []
    for n in sorted(set(a) & set(b)):
        what = [w for w, x, y in (("code", a[n][0], b[n][0]), ("amdhsa", a[n][1], b[n][1])) if x != y]
        if not a[n][0] or not a[n][1]:
            what.append("not found")
        if what:
            differ.append(n)
            print(f"differs ({', '.join(what)}): {n}")
    print(f"differing kernels: {len(differ)}")
    return 1 if only or differ else 0


if __name__ == "__main__":
    sys.exit(main())
