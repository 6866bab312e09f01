"""measurement only: the device timeline around two consecutive k_classify_main launches late in a run, from the kernel trace of
  rocprofv3 --kernel-trace --stats -d DIR -o k --output-format csv -- python bench.py --steps 60 --warmup 10
laid out as in profiles/r07/experiments/pass_tail.txt (us relative to the first launch's end: start, duration, grid, queue, kernel).
  python tools/pass_timeline.py DIR"""
import csv, glob, os, sys
import numpy as np
paths = glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True)
if not paths:
    sys.exit("no *kernel_trace.csv under " + sys.argv[1])
rows = []
with open(paths[0], newline="") as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Queue_Id", "?"), r.get("Grid_Size", r.get("Grid_Size_X", "?"))))
rows.sort()
main = [i for i, r in enumerate(rows) if "k_classify_main" in r[2]]
late = main[len(main) // 2:]
gaps = np.array([(rows[b][0] - rows[a][1]) / 1e3 for a, b in zip(late, late[1:])])
over = np.array([(rows[a][1] - rows[b][0]) / 1e3 for a, b in zip(late, late[1:])])
print(f"{len(main)} k_classify_main launches; next start minus this end in the second half of the run: median {np.median(gaps):.1f} us, min {gaps.min():.1f}, max {gaps.max():.1f}"
      f"; launches that start before the one in front ends: {(over > 0).sum()} of {len(over)}")
queues = sorted({rows[i][3] for i in late})
print(f"  queues of k_classify_main: {queues}; consecutive launches on different queues: {sum(rows[a][3] != rows[b][3] for a, b in zip(late, late[1:]))} of {len(late) - 1}")
a, b = late[-6], late[-5]
t0 = rows[a][1]
print("  between two launches late in the run (us after the first one's end: start, duration, grid, queue):")
lo, hi = rows[a][0], rows[b][1]
for r in rows:
    if r[1] >= lo and r[0] <= hi and (r[0] >= lo):
        print(f"    {(r[0] - t0) / 1e3:+9.1f} {(r[1] - r[0]) / 1e3:8.1f}  grid {r[4]:>8}  q {r[3]:>3}  {r[2][:60]}")
