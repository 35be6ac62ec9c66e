#!/usr/bin/env python3
"""Compare the device code of two builds of one source file, kernel by kernel.
   hipcc <build.FLAGS> --offload-device-only -S csrc/FILE.hip -o before.s   (at the parent commit; likewise after.s at the head)
   python tools/isa_compare.py before.s after.s
(a file that was split, as bis_spmv_sell.hip into bis_spmv_sellwin.hip and bis_spmv_win8.hip: after.s = the parts' .s files, concatenated)
A kernel is the text between its `.type NAME,@function` line and its `.Lfunc_end` label; comments and the numbering of the
local labels are dropped, the kernel's own name is replaced.  Kernels are matched by mangled name; the value-type argument
`d` (double) that `spmv_win8_kernel` and `w8_fill_kernel` gained with the 4-byte stream is dropped from the head's names, so the
fp64 instances meet their parents.  Prints every kernel of `before` that is missing or differs and "N of M identical";
exit status 1 unless N == M."""
import re
import sys


def kernels(path):
    with open(path) as f:
        txt = f.read()
    return {m.group(1): m.group(2) for m in re.finditer(r"^\s*\.type\s+(\S+),@function\n(.*?)^\.Lfunc_end\d+:", txt, flags=re.S | re.M)}


def key(name):
    return re.sub(r"((?:win8_kernel|w8_fill_kernel)I\w+?)dEEv", r"\1EEv", name)


def norm(body, name):
    body = re.sub(r";.*", "", re.sub(r"\.L\w+", ".L", body.replace(name, "KERNEL")))
    return "\n".join(line.strip() for line in body.splitlines() if line.strip())


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    by_key = {key(n): n for n in b}
    same = 0
    for n in a:
        m = by_key.get(key(n))
        if m is None:
            print("MISSING", n)
        elif norm(a[n], n) != norm(b[m], m):
            print("DIFFERS", n)
        else:
            same += 1
    print(f"{same} of {len(a)} identical ({len(b)} kernels after)")
    return 0 if same == len(a) else 1


if __name__ == "__main__":
    sys.exit(main())
