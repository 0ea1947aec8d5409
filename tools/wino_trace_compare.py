#!/usr/bin/env python
"""The Winograd kernels of two kernel traces, as sets and as sequences — the check on csrc/lcnn_wino_plan.h's launch plan.

    rocprofv3 --kernel-trace --output-format csv -d DIR_A -o a -- python tools/wino_kernel_outputs.py a.npz      (one build)
    rocprofv3 --kernel-trace --output-format csv -d DIR_B -o b -- python tools/wino_kernel_outputs.py b.npz      (the other)
    python tools/wino_trace_compare.py DIR_A DIR_B

Prints how often each kernel ran in A, how many wino3x3_kernel instantiations each trace reached (all 48 is the aim), and
whether both traces show the same sequence of (kernel, grid, workgroup, LDS bytes).  Enumeration template arguments are
printed as their integer values."""
import csv, glob, re, sys

def norm(name):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "").replace(" [clone .kd]", "")
    name = re.sub(r"\((?:\w+::)*\w+\)(-?\d+)", r"\1", name)
    return re.sub(r"\(.*", "", name)

def load(d):
    files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    out = []
    for r in rows:
        n = norm(r["Kernel_Name"])
        if "wino" not in n:
            continue
        out.append((n, tuple(int(r[k]) for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y",
                                                 "Workgroup_Size_Z", "LDS_Block_Size"))))
    return out

a, b = load(sys.argv[1]), load(sys.argv[2])
for tag, t in (("A", a), ("B", b)):
    names = sorted({n for n, _ in t})
    conv = [n for n in names if n.startswith("wino3x3_kernel")]
    print(f"{tag}: {len(t)} Winograd dispatches, {len(names)} distinct kernels, {len(conv)} wino3x3_kernel instantiations")
    if tag == "A":
        for n in names:
            print("   ", n, sum(1 for m, _ in t if m == n))
print("same set of kernel names:", {n for n, _ in a} == {n for n, _ in b})
print("same sequence of (kernel, grid, workgroup, LDS):", a == b)
if a != b:
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            print("first difference at dispatch", i, x, y)
            break
    print(len(a), len(b))
