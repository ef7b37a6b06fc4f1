#!/usr/bin/env python3
"""Kernel-argument round trips at kernel entry, read from the compiled gfx950 assembly.

A kernel's arguments arrive through scalar loads from the kernel-argument segment. All of
them issued before the first `s_waitcnt lgkmcnt(0)` share one memory round trip; each one
issued after it (hipcc sinks an argument's load into the branch that uses it) costs the
workgroups that reach it another dependent round trip ahead of their first vector load.
For every kernel named on the command line this reports

  * the kernel-argument loads (s_load_* whose base is the kernel-argument pointer pair)
    that appear after the first s_waitcnt lgkmcnt(0), with their offsets; an offset
    marked `!` is reached on some path before any vector memory load has been issued
    (a dependent scalar round trip at entry), the others only behind vector loads;
  * .vgpr_count, .sgpr_count, the spill counts and .kernarg_segment_size.

usage: entry_trips.py [--asm FILE.s] [--json] KERNEL [KERNEL ...]
       KERNEL as in the source, e.g. 'k_p1_spmv<58>' or 'k_p1_axpy<12>'.

Without --asm the kernels are looked up in two-pass-lanczos_amd/csrc/build/all_units.asm,
every unit's build/<unit>.s joined (`make asm` writes them: a kernel is found whichever
unit holds it). When it is missing or older than the kernel sources, `make asm` is run
first, with at most 16 jobs (about half a minute).
"""
import argparse
import glob
import json
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "two-pass-lanczos_amd", "csrc")


# ------------------------------------------------------------------ the assembly file
ALL_UNITS = os.path.join(CSRC, "build", "all_units.asm")  # `make asm`: every <unit>.s, joined


def fresh_asm():
    """ALL_UNITS, or None when it is missing or older than the kernel sources."""
    newest_src = max(os.path.getmtime(p) for p in
                     [os.path.join(CSRC, "Makefile")] + glob.glob(os.path.join(CSRC, "*.hip")) +
                     glob.glob(os.path.join(CSRC, "tpl_*.h")))
    if os.path.exists(ALL_UNITS) and os.path.getmtime(ALL_UNITS) >= newest_src:
        return ALL_UNITS
    return None


def have_hipcc():
    return bool(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))


def compile_asm():
    jobs = str(min(16, os.cpu_count() or 4))
    subprocess.run(["make", "-C", CSRC, "-j", jobs, "asm"], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    return ALL_UNITS


def asm_path():
    return fresh_asm() or compile_asm()


# ------------------------------------------------------------------ reading it
def mangled_fragment(kernel):
    """'k_p1_spmv<58>' -> '9k_p1_spmvILi58EE', 'k_bp2_cached<4, 3>' ->
    '12k_bp2_cachedILi4ELi3EE', 'k_ftk_inv' -> '9k_ftk_invE' (Itanium)."""
    m = re.fullmatch(r"(\w+)(?:<(-?\d+(?:\s*,\s*-?\d+)*)>)?", kernel.strip())
    if not m:
        raise ValueError("kernel name %r: expected NAME or NAME<INT[, INT ...]>" % kernel)
    name, args = m.group(1), m.group(2)
    if args is None:
        return "%d%sE" % (len(name), name)
    lits = [("n" + a[1:]) if a.startswith("-") else a for a in re.split(r"\s*,\s*", args)]
    return "%d%sI%sE" % (len(name), name, "".join("Li%sE" % l for l in lits))


def find_symbol(text, kernel):
    frag = mangled_fragment(kernel)
    syms = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    hits = sorted(s for s in syms if frag in s)
    if len(hits) != 1:
        raise KeyError("%s: %d kernels match %r in the assembly" % (kernel, len(hits), frag))
    return hits[0]


def _regs(tok):
    """'s[4:5]' -> {4, 5}; 's7' -> {7}; anything else -> empty."""
    m = re.fullmatch(r"s\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"s(\d+)", tok)
    return {int(m.group(1))} if m else set()


def kernarg_pair(text, sym):
    """SGPR pair holding the kernel-argument segment pointer at entry: the user SGPRs come
    in a fixed order (private segment buffer 4, dispatch pointer 2, queue pointer 2, then
    the kernel-argument pointer)."""
    m = re.search(r"\.amdhsa_kernel\s+%s\n(.*?)\.end_amdhsa_kernel" % re.escape(sym), text, re.S)
    if not m:
        raise KeyError("no .amdhsa_kernel block for " + sym)
    blk = m.group(1)

    def on(key):
        k = re.search(r"\.amdhsa_user_sgpr_%s\s+(\d+)" % key, blk)
        return bool(k and int(k.group(1)))

    base = 4 * on("private_segment_buffer") + 2 * on("dispatch_ptr") + 2 * on("queue_ptr")
    return {base, base + 1}


def body_lines(text, sym):
    m = re.search(r"^%s:.*?\n(.*?)^\s*\.section|^%s:.*?\n(.*?)^\.Lfunc_end" %
                  (re.escape(sym), re.escape(sym)), text, re.S | re.M)
    if not m:
        raise KeyError("no code for " + sym)
    body = m.group(1) if m.group(1) is not None else m.group(2)
    end = body.find(".Lfunc_end")
    return (body if end < 0 else body[:end]).splitlines()


_NO_DST = ("s_waitcnt", "s_cbranch", "s_branch", "s_cmp", "s_endpgm", "s_barrier", "s_nop",
           "s_setprio", "s_sleep", "s_bitcmp", "s_setreg", "s_sendmsg", "s_trap", "s_code_end")


_VMEM = ("global_load", "buffer_load", "flat_load", "scratch_load", "global_atomic",
         "buffer_atomic", "flat_atomic")


def _instructions(text, sym):
    """The kernel's instructions in text order: dicts with op, args, the label(s) bound to
    the instruction, and whether it is a kernel-argument load (copies of the pointer pair
    made with s_mov_b64 are followed)."""
    pairs = [kernarg_pair(text, sym)]
    out, labels = [], []
    for raw in body_lines(text, sym):
        ins = raw.split(";")[0].strip()
        if not ins or ins.startswith("."):
            if re.fullmatch(r"\.L\w+:", ins):
                labels.append(ins[:-1])
            continue
        if ins.endswith(":"):
            labels.append(ins[:-1])
            continue
        op, _, rest = ins.partition(" ")
        args = [a.strip() for a in rest.split(",")] if rest else []
        d = {"op": op, "args": args, "text": ins, "labels": labels, "kernarg": False}
        labels = []
        if op.startswith("s_load_") and len(args) >= 2:
            d["kernarg"] = any(_regs(args[1]) == p for p in pairs)
            off = args[2] if len(args) > 2 else "0x0"
            d["offset"] = int(off, 0) if re.fullmatch(r"(0x[0-9a-fA-F]+|\d+)", off) else off
            dst = _regs(args[0])
            pairs = [p for p in pairs if not (p & dst)]
        elif op == "s_mov_b64" and len(args) == 2 and any(_regs(args[1]) == p for p in pairs):
            pairs.append(_regs(args[0]))
        elif op.startswith("s_") and op != "s_waitcnt" and not op.startswith(_NO_DST) and args:
            dst = _regs(args[0])
            pairs = [p for p in pairs if not (p & dst)]
        out.append(d)
    return out


def late_loads(text, sym):
    """Kernel-argument loads after the first s_waitcnt lgkmcnt(0), in program text order:
    [(offset, instruction, ahead)]. ahead: some path from the kernel's entry reaches the
    load behind a completed wait with no vector memory load or atomic issued yet — the
    workgroups on that path pay a dependent scalar round trip before their first vector
    load. The others sit behind vector loads already in flight."""
    ins = _instructions(text, sym)
    at = {}
    for i, d in enumerate(ins):
        for l in d["labels"]:
            at[l] = i
    # walk the control-flow graph from the entry while no vector memory access has been
    # issued; state: (instruction, a wait for lgkmcnt(0) passed on this path)
    ahead, seen, todo = set(), set(), [(0, False)]
    while todo:
        i, waited = todo.pop()
        while i < len(ins) and (i, waited) not in seen:
            seen.add((i, waited))
            d = ins[i]
            op = d["op"]
            if op.startswith(_VMEM) or op in ("s_endpgm", "s_setpc_b64", "s_swappc_b64"):
                break
            if op == "s_waitcnt" and any("lgkmcnt(0)" in a for a in d["args"] + [d["text"]]):
                waited = True
            if d["kernarg"] and waited:
                ahead.add(i)
            if op == "s_branch":
                i = at.get(d["args"][0], len(ins))
                continue
            if op.startswith("s_cbranch") and d["args"] and d["args"][-1] in at:
                todo.append((at[d["args"][-1]], waited))
            i += 1
    late, waited = [], False
    for i, d in enumerate(ins):
        if d["op"] == "s_waitcnt" and "lgkmcnt(0)" in d["text"]:
            waited = True
        elif d["kernarg"] and waited:
            late.append((d["offset"], d["text"], i in ahead))
    return late


_META = {"vgpr_count": ".vgpr_count", "sgpr_count": ".sgpr_count",
         "sgpr_spill_count": ".sgpr_spill_count", "vgpr_spill_count": ".vgpr_spill_count",
         "kernarg_segment_size": ".kernarg_segment_size"}


def metadata(text, sym):
    """The kernel's entry of the amdhsa.kernels metadata (the counts named in _META)."""
    at = text.find(".name:           " + sym + "\n")
    if at < 0:
        m = re.search(r"\.name:\s+%s\s*$" % re.escape(sym), text, re.M)
        if not m:
            raise KeyError("no metadata for " + sym)
        at = m.start()
    lo = text.rfind("\n  - ", 0, at)
    hi = text.find("\n  - ", at)
    entry = text[lo:hi if hi > 0 else len(text)]
    out = {}
    for key, tag in _META.items():
        m = re.search(r"^\s*%s:\s+(\d+)" % re.escape(tag), entry, re.M)
        out[key] = int(m.group(1)) if m else None
    return out


def report(text, kernel):
    sym = find_symbol(text, kernel)
    late = late_loads(text, sym)
    r = {"kernel": kernel, "symbol": sym,
         "late_kernarg_loads": [{"offset": o, "instruction": i, "before_vector_load": h}
                                for o, i, h in late]}
    r.update(metadata(text, sym))
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--asm", help="assembly file (default: csrc/build/all_units.asm, built if stale)")
    ap.add_argument("--json", action="store_true", help="one JSON list instead of the table")
    ap.add_argument("kernels", nargs="+")
    a = ap.parse_args(argv)
    path = a.asm or asm_path()
    text = open(path, errors="replace").read()
    reps = [report(text, k) for k in a.kernels]
    if a.json:
        print(json.dumps(reps, indent=1))
        return 0
    print("# " + os.path.relpath(path, ROOT))
    print("%-20s %5s %5s %7s %7s %8s  %s" % ("kernel", "vgpr", "sgpr", "sspill", "vspill",
                                              "kernarg", "late kernel-argument loads"))
    for r in reps:
        offs = ", ".join((hex(l["offset"]) if isinstance(l["offset"], int) else l["offset"]) +
                         ("!" if l["before_vector_load"] else "")
                         for l in r["late_kernarg_loads"])
        print("%-20s %5s %5s %7s %7s %8s  %d%s" % (
            r["kernel"], r["vgpr_count"], r["sgpr_count"], r["sgpr_spill_count"],
            r["vgpr_spill_count"], r["kernarg_segment_size"], len(r["late_kernarg_loads"]),
            (" at " + offs) if offs else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
