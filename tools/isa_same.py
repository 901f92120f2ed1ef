#!/usr/bin/env python3
"""Do two sets of hipcc -S listings hold the same kernels?  (A move of kernels
between translation units must not change their code.)

    hipcc <the Makefile's FLAGS> --cuda-device-only -S -o old.s old/csrc/screen32.hip   (and new*.s)
    python tools/isa_same.py old.s -- new1.s new2.s ... [-r 'REGEX=>REPL' ...]

Compares, per kernel (matched by demangled name, after the -r rewrites), the
instruction text and the kernel descriptor (.amdhsa_*: registers, LDS, scratch).
Local labels are normalised first (.LBB<n>_<m> carries the function's index,
which changes with file order).  Prints the kernels that differ, with their
descriptor lines that differ, and those only one side has; exit status 1 if any
kernel differs."""
import re
import subprocess
import sys


def kernels(paths, rewrites):
    out = {}
    for path in paths:
        text = open(path).read()
        desc = {m[1]: m[2] for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S)}
        for sym, d in desc.items():
            body = re.search(r"^" + re.escape(sym) + r":[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M)[1]
            lines = [re.sub(r"\s*;.*", "", l).strip() for l in body.splitlines()]
            lines = [re.sub(r"\.LBB\d+_", ".LBB_", l) for l in lines if l and (l[0] != "." or l.startswith(".LBB"))]
            name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
            name = name.replace("(anonymous namespace)::", "")
            for pat, rep in rewrites:
                name = re.sub(pat, rep, name)
            assert name not in out, name
            out[name] = ("\n".join(lines), [l.strip() for l in d.splitlines()])
    return out


def main():
    args = sys.argv[1:]
    rewrites = []
    while "-r" in args:
        i = args.index("-r")
        rewrites.append(tuple(args[i + 1].split("=>")))
        del args[i:i + 2]
    old = kernels(args[:args.index("--")], rewrites)
    new = kernels(args[args.index("--") + 1:], rewrites)
    both = sorted(set(old) & set(new))
    differ = [k for k in both if old[k] != new[k]]
    for k in differ:
        print("DIFFERS", k, "(instructions)" if old[k][0] != new[k][0] else "(descriptor only)")
        for a, b in zip(old[k][1], new[k][1]):
            if a != b:
                print(f"    {a}  ->  {b}")
    for k in sorted(set(old) - set(new)):
        print("ONLY OLD", k)
    for k in sorted(set(new) - set(old)):
        print("ONLY NEW", k)
    print(f"kernels: old {len(old)}, new {len(new)}, compared {len(both)}, identical {len(both) - len(differ)}")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
