#!/usr/bin/env python3
"""Per-kernel diff of two device assembly files.

    hipcc ... --offload-arch=gfx950 --cuda-device-only -S x.hip -o a.s   (twice)
    python tools/isa_diff.py a.s b.s
    python tools/isa_diff.py --templates a.s b.s

Splits each file per kernel symbol, drops comments and directives, normalises
the function-numbered local labels and compares the instruction streams of
the kernels both files have.  Prints
    identical N different M only-in-first [...] only-in-second [...]
and exits 1 if a common kernel differs.  It is a differ and looks at nothing
else.

--templates pairs kernels by demangled template name (ns::kernel<args>, the
parameter list cut off) instead of by symbol, and drops trailing ",false"
template arguments first: a commit that adds a defaulted-off compile-time
flag and trailing kernel arguments renames every symbol, and this pairs
kernel<64,false> of the old file with kernel<64,false,false> of the new.
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


def template_names(ks):
    """Re-key {symbol: lines} by demangled template name with the trailing
    ",false" arguments dropped."""
    syms = sorted(ks)
    res = subprocess.run(["c++filt"], input="\n".join(syms), text=True,
                         capture_output=True, check=True).stdout.split("\n")
    out = {}
    for sym, dem in zip(syms, res):
        name = dem.split("(")[0].replace("void ", "").replace(" ", "")
        while name.endswith(",false>"):
            name = name[:-len(",false>")] + ">"
        assert name not in out, name
        # the kernel's own entry label carries the symbol
        out[name] = [t for t in ks[sym] if t != sym + ":"]
    return out


def pretty(names):
    names = sorted(names)
    if names and not names[0].startswith("_Z"):
        return "[" + ", ".join(names) + "]"
    if names and shutil.which("c++filt"):
        res = subprocess.run(["c++filt"], input="\n".join(names), text=True,
                             capture_output=True).stdout.split("\n")
        names = [n.split("(")[0].replace("void ", "").replace(" ", "")
                 for n in res if n]
    return "[" + ", ".join(names) + "]"


def main(argv):
    by_template = argv[:1] == ["--templates"]
    argv = argv[1:] if by_template else argv
    if len(argv) != 2:
        sys.exit(__doc__)
    a, b = kernels(argv[0]), kernels(argv[1])
    if by_template:
        a, b = template_names(a), template_names(b)
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
