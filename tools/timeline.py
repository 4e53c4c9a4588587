"""One frame's kernels on a time axis, from a rocprofv3 --kernel-trace run: start / end (us from the frame's first kernel), queue.
Usage: python tools/timeline.py <trace_dir> [frames-from-the-end]     (kernels that started within that frame's period, either lane)"""
import csv, glob, sys
d = sys.argv[1]; back = int(sys.argv[2]) if len(sys.argv) > 2 else 10
rows = []
for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
    rows += list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
short = lambda n: n.split("(")[0].replace("void ", "").strip()
fb = [i for i, r in enumerate(rows) if short(r["Kernel_Name"]) == "k_frame_begin"]
rest = [i for i, r in enumerate(rows) if short(r["Kernel_Name"]).startswith("k_lighting_rest")]
if rest and (not fb or rest[-1] > fb[-1] + 8):      # the last frames have no k_frame_begin: a resting frame is ONE launch, and that is its start
    fb = rest
a, b = fb[-back - 1], fb[-back]
t0 = int(rows[a]["Start_Timestamp"])
qs = {}
per = sorted((int(rows[y]["Start_Timestamp"]) - int(rows[x]["Start_Timestamp"])) / 1e3 for x, y in zip(fb[-back - 1:-1], fb[-back:]))
print("period %.1f us (median of the last %d; the first frame shown: %.1f)" % (per[len(per) // 2], len(per), (int(rows[b]["Start_Timestamp"]) - t0) / 1e3))
for r in rows[a:b + 12]:
    q = qs.setdefault(r.get("Queue_Id", "?"), len(qs))
    s, e = (int(r["Start_Timestamp"]) - t0) / 1e3, (int(r["End_Timestamp"]) - t0) / 1e3
    print("%s%-28s %8.1f -> %8.1f  (%6.1f)" % ("    " * 10 * 0 + ("" if q == 0 else " " * 44), short(r["Kernel_Name"]), s, e, e - s))
