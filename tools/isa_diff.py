#!/usr/bin/env python
"""Which kernels' gfx950 assembly differs between two builds of the engine: the check behind "no existing kernel changes".
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -disable-machine-licm --cuda-device-only -S -o a.s fast_gicp_amd/csrc/fvh_capi.hip   (in each tree)
    python tools/isa_diff.py a.s b.s
Compares every kernel's body as text. Basic-block labels carry the function's ordinal in the file (.LBB123_4, "Header=BB123_5") and
the padding before a label's comment follows its width: both are normalised, since a kernel added in front renumbers every later one.
(tools/count_isa.py gives the instruction mix of one kernel.) Exit status 1 when a kernel of the first file changed or disappeared."""
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.S | re.M):
        body = re.sub(r"BB\d+_", "BB_", m.group(2))
        body = re.sub(r"\.Ltmp\d+", ".Ltmp", body)
        out[m.group(1)] = re.sub(r"[ \t]+", " ", body)
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    added = sorted(k for k in b if k not in a)
    gone = sorted(k for k in a if k not in b)
    changed = sorted(k for k in a if k in b and a[k] != b[k])
    print("%d kernels in %s, %d in %s" % (len(a), sys.argv[1], len(b), sys.argv[2]))
    for what, names in (("added", added), ("removed", gone), ("changed", changed)):
        print("%s: %d" % (what, len(names)))
        for k in names:
            print("  " + k)
    return 1 if gone or changed else 0


if __name__ == "__main__":
    sys.exit(main())
