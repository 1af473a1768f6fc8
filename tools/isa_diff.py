#!/usr/bin/env python3
"""Per-kernel diff of two device assembly files.

    hipcc ... --offload-arch=gfx950 --cuda-device-only -S x.hip -o a.s   (twice)
    python tools/isa_diff.py a.s b.s

Splits each file per kernel symbol, drops comments and directives, normalises
the function-numbered local labels and compares the instruction streams of
the kernels both files have.  Prints
    identical N different M only-in-first [...] only-in-second [...]
and exits 1 if a common kernel differs.  It is a differ and looks at nothing
else.
"""

import re
import shutil
import subprocess
import sys

BEGIN = re.compile(r"^\s*\.type\s+(\S+),@function")
END = re.compile(r"^\.Lfunc_end\d+:")
LABEL = re.compile(r"\.L([A-Za-z_]*)\d+_(\d+)")      # .LBB<function>_<block>


def kernels(path):
    out, name = {}, None
    for line in open(path):
        m = BEGIN.match(line)
        if m:
            name, out[m.group(1)] = m.group(1), []
        elif END.match(line):
            name = None
        elif name is not None:
            text = line.split(";", 1)[0].strip()
            if text and (not text.startswith(".") or text.endswith(":")):
                out[name].append(LABEL.sub(r".L\1_\2", text))
    return out


def pretty(names):
    names = sorted(names)
    if names and shutil.which("c++filt"):
        res = subprocess.run(["c++filt"], input="\n".join(names), text=True,
                             capture_output=True).stdout.split("\n")
        names = [n.split("(")[0].replace("void ", "").replace(" ", "")
                 for n in res if n]
    return "[" + ", ".join(names) + "]"


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    a, b = kernels(argv[0]), kernels(argv[1])
    common = sorted(set(a) & set(b))
    differ = [k for k in common if a[k] != b[k]]
    print("identical", len(common) - len(differ), "different", len(differ),
          "only-in-first", pretty(set(a) - set(b)),
          "only-in-second", pretty(set(b) - set(a)))
    if differ:
        print("different:", pretty(differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
