#!/usr/bin/env python3
"""compare_isa.py OLD.so NEW.so [-v] -- do two builds of libturborc_hip.so hold the same gfx950 kernels, instruction for instruction?

Disassembles both libraries (check_isa_hazards.disassemble), cuts the text into kernels and compares each kernel's instruction
stream with what depends on placement taken out: addresses, encodings and the numbers of branch labels.  Kernels are matched by
demangled name after the known renames of a refactor, given as --rename 'REGEX=REPLACEMENT' (any number of them, applied in order to
the OLD names).  Prints the kernels that differ, that exist on one side only, and the counts; exit status 1 if any.  -v adds a
unified diff of the first differing kernels (--only REGEX: of those whose name matches).  A review aid for pull requests that must not change generated code; not a test.
"""
import difflib
import os
import re
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_isa_hazards import disassemble

CXXFILT = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"


def kernels(lib):
    """{demangled name: [normalised instruction, ...]}"""
    out, cur = {}, None
    for line in disassemble(lib).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
        if m:
            name = m.group(1)
            cur = None if re.match(r"L\d+|\$|\.", name) else out.setdefault(name, [])     # a label inside a kernel goes on with it
            continue
        m = re.match(r"^\s+([a-z_0-9]+)\s*(.*?)\s*//", line)
        if m and cur is not None:
            ops = re.sub(r"<[^>]*>", "<L>", m.group(2))                                   # branch targets
            if m.group(1).startswith(("s_branch", "s_cbranch", "s_call", "s_getpc", "s_setpc")):
                ops = re.sub(r"\b\d+\b|0x[0-9a-f]+", "N", ops)
            cur.append((m.group(1) + " " + ops).strip())
    names = list(out)
    dem = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return {d: out[n] for n, d in zip(names, dem)}


def main():
    args, renames, verbose, only = [], [], False, None
    it = iter(sys.argv[1:])
    for a in it:
        if a == "-v":
            verbose = True
        elif a == "--only":
            only = re.compile(next(it))
        elif a == "--rename":
            pat, rep = next(it).split("=", 1)
            renames.append((re.compile(pat), rep))
        else:
            args.append(a)
    if len(args) != 2:
        sys.exit(__doc__)
    old, new = kernels(args[0]), kernels(args[1])
    renamed = {}
    for name, code in old.items():
        for pat, rep in renames:
            name = pat.sub(rep, name)
        renamed[name] = code
    differ = sorted(k for k in renamed if k in new and renamed[k] != new[k])
    gone, added = sorted(k for k in renamed if k not in new), sorted(k for k in new if k not in renamed)
    for k in differ:
        print("differs: %s (%d -> %d instructions)" % (k, len(renamed[k]), len(new[k])))
    for k in gone:
        print("only in %s: %s" % (args[0], k))
    for k in added:
        print("only in %s: %s" % (args[1], k))
    if verbose:
        for k in [k for k in differ if not only or only.search(k)][:4]:
            print("\n".join(list(difflib.unified_diff(renamed[k], new[k], "old " + k, "new " + k, lineterm="", n=2))[:80]))
    print("%d kernels in the old library, %d in the new: %d differ, %d only old, %d only new" % (len(old), len(new), len(differ), len(gone), len(added)))
    return 1 if differ or gone or added else 0


if __name__ == "__main__":
    sys.exit(main())
