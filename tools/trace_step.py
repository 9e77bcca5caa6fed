"""Per-dispatch durations of one training step from a rocprofv3 --kernel-trace CSV: trace_step.py DIR [name-substring]
The grid column is workgroups as x*y*z (Grid_Size_* are work-items: a split-K GEMM keeps its splits in z) @ workgroup size."""
import csv, glob, sys
d = sys.argv[1]; sub = sys.argv[2] if len(sys.argv) > 2 else ""
rows = []
def wgs(r):
    try:
        g = [int(r["Grid_Size_" + a]) for a in "XYZ"]
        w = [max(int(r["Workgroup_Size_" + a]), 1) for a in "XYZ"]
        return "%d*%d*%d@%d" % (g[0] // w[0], g[1] // w[1], g[2] // w[2], w[0] * w[1] * w[2])
    except (KeyError, ValueError):
        return r.get("Grid_Size_X", r.get("Grid_Size", "?"))
for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].replace("(anonymous namespace)::", ""), wgs(r)))
rows.sort()
# last step = dispatches after the last zero_f32
last = max(i for i, r in enumerate(rows) if "zero_f32" in r[2])
# find the forward start: previous readout_molecules..., simply take the window between the previous zero_f32 and last
prev = max(i for i, r in enumerate(rows[:last]) if "zero_f32" in r[2])
t0 = rows[prev][0]
busy = 0
for s, e, n, g in rows[prev:last]:
    busy += e - s
    if sub in n:
        print(f"{(e-s)/1e3:9.1f} us  grid {g:>16s}  {n.split('(')[0][-70:]}")
print(f"# {last - prev} dispatches, sum of durations {busy/1e3:.1f} us, first start to last end {(rows[last-1][1]-t0)/1e3:.1f} us")
