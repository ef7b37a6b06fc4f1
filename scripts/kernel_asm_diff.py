#!/usr/bin/env python3
"""Compare the kernels of two builds' device assembly: kernel_asm_diff.py OLD_DIR NEW_DIR.

Each directory holds the `*.s` files of one build (`make asm` in csrc writes build/<unit>.s);
a kernel is found in whichever file holds it, so the two builds may cut their units
differently. For every kernel symbol (`.amdhsa_kernel NAME`) of either side the tool takes
the body, from the label `NAME:` to `.Lfunc_end`, and the `.amdhsa_kernel` block, drops
assembler comments and trailing whitespace, and replaces the function's ordinal within its
file in block labels (`BB<n>_`, `func_end<n>`). It reports the kernels present on one side
only and those whose text differs (with a unified diff of the first; -v: of all), prints
one summary line, and exits non-zero if either list is non-empty.
"""
import difflib
import glob
import os
import re
import sys


def normalise(text):
    out = []
    for line in text.splitlines():
        line = line.split(";")[0].rstrip()
        if line:
            out.append(re.sub(r"(BB|func_end)\d+", r"\1N", line))
    return out


def kernels(text):
    """{symbol: normalised lines of the body and of the .amdhsa_kernel block}."""
    syms = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    # a template instance's descriptor block comes before its .Lfunc_end label, inside the
    # body: the two are collected independently
    body, desc, in_body, in_desc = {}, {}, None, None
    for line in text.splitlines():
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            in_desc = desc.setdefault(m.group(1), [])
        if in_desc is not None:
            in_desc.append(line)
            if line.strip().startswith(".end_amdhsa_kernel"):
                in_desc = None
            continue
        if in_body is None and line[:1] not in (" ", "\t", "") and line.split(":")[0] in syms:
            in_body = body.setdefault(line.split(":")[0], [])
        if in_body is not None:
            in_body.append(line)
            if line.startswith(".Lfunc_end"):
                in_body = None
    missing = sorted(s for s in syms if s not in body)
    if missing:
        raise ValueError("no code for kernel " + missing[0])
    return {s: normalise("\n".join(body[s] + desc[s])) for s in syms}


def kernels_in(directory):
    found = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        with open(path, errors="replace") as f:
            for sym, lines in kernels(f.read()).items():
                if sym in found:
                    raise ValueError("kernel %s is in more than one file of %s" % (sym, directory))
                found[sym] = lines
    return found


def compare(old, new):
    """(symbols only in old, only in new, in both with different text), each sorted."""
    return (sorted(set(old) - set(new)), sorted(set(new) - set(old)),
            sorted(s for s in set(old) & set(new) if old[s] != new[s]))


def main(argv=None):
    args = list(sys.argv[1:] if argv is None else argv)
    verbose = "-v" in args
    args = [a for a in args if a != "-v"]
    if len(args) != 2:
        print(__doc__.split("\n\n")[0] + "\nusage: kernel_asm_diff.py [-v] OLD_DIR NEW_DIR",
              file=sys.stderr)
        return 2
    old, new = kernels_in(args[0]), kernels_in(args[1])
    only_old, only_new, differ = compare(old, new)
    for s in only_old:
        print("only in %s: %s" % (args[0], s))
    for s in only_new:
        print("only in %s: %s" % (args[1], s))
    for i, s in enumerate(differ):
        n = sum(1 for l in difflib.ndiff(old[s], new[s]) if l[0] in "+-")
        print("differs: %s (%d of %d lines)" % (s, n, len(old[s])))
        if verbose or i == 0:
            print("\n".join(difflib.unified_diff(old[s], new[s], "old", "new", lineterm="", n=2)))
    print("%d kernels in %s, %d in %s: %d on one side only, %d differ" %
          (len(old), args[0], len(new), args[1], len(only_old) + len(only_new), len(differ)))
    return 1 if only_old or only_new or differ else 0


if __name__ == "__main__":
    sys.exit(main())
