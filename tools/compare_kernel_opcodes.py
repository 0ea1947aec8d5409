#!/usr/bin/env python
"""Per-kernel opcode histograms of two device assembly files (hipcc ... --cuda-device-only -S), side by side — to show
that a change of the source left the generated code alone.

    python tools/compare_kernel_opcodes.py before.s after.s [--ignore s_nop]

Kernels are matched by demangled name without the parameter list; enumeration template arguments count as their
integer values (`(Epi)1` reads `1`), so a source that gave its integer template parameters enum types still lines up with
its parent.  Per kernel: instruction count, static LDS bytes, and every opcode whose count differs.
Exit status 1 when a kernel is missing on one side or differs in LDS size or in an opcode that is not ignored.
"""
import collections
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    res = {}
    for raw, d in zip(names, out):
        d = d.replace("(anonymous namespace)::", "").replace("void ", "")
        d = re.sub(r"\((?:\w+::)*\w+\)(-?\d+)", r"\1", d)          # (Epi)1 -> 1
        res[raw] = re.sub(r"\(.*", "", d)                              # drop the parameter list
    return res


def kernels(path):
    """{demangled name: (Counter of opcodes, static LDS bytes)} for every .amdhsa_kernel of the file."""
    text = open(path).read().splitlines()
    lds, body, cur = {}, {}, None
    for line in text:
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", line)
        if m and not m.group(1).startswith(".L"):
            cur = m.group(1)
            body[cur] = collections.Counter()
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            cur = None
            continue
        m = re.match(r"^\s+\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur_k = m.group(1)
            lds[cur_k] = None
            continue
        m = re.match(r"^\s+\.amdhsa_group_segment_fixed_size\s+(\d+)", line)
        if m:
            lds[cur_k] = int(m.group(1))
            continue
        m = re.match(r"^\s+([a-z][a-z0-9_]*)\b", line)
        if m and cur is not None:
            body[cur][m.group(1)] += 1
    names = demangle(list(lds))
    return {names[k]: (body[k], lds[k]) for k in lds}


def main(argv):
    ignore = set()
    if "--ignore" in argv:
        i = argv.index("--ignore")
        ignore = set(argv[i + 1].split(","))
        del argv[i:i + 2]
    if len(argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(argv[1]), kernels(argv[2])
    bad = same = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"{name:64s} only in {'before' if name in a else 'after'}")
            bad += 1
            continue
        (ca, la), (cb, lb) = a[name], b[name]
        diff = {op: (ca[op], cb[op]) for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op]}
        hard = {op: v for op, v in diff.items() if op not in ignore}
        note = "equal" if not diff else ", ".join(f"{op} {x} -> {y}" for op, (x, y) in diff.items())
        if la != lb:
            note += f"; static LDS {la} -> {lb}"
        print(f"{name:64s} instr {sum(ca.values()):6d} {sum(cb.values()):6d}  LDS {la:6d}  {note}")
        if hard or la != lb:
            bad += 1
        else:
            same += 1
    print(f"{len(set(a) | set(b))} kernels: {same} with equal opcode counts"
          f"{' (' + ', '.join(sorted(ignore)) + ' aside)' if ignore else ''} and static LDS, {bad} not")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
