"""median / min kernel time per kernel name of the last 20 dispatches in every *_kernel_trace.csv under out/m1"""
import csv, glob, os, statistics, collections
for f in sorted(glob.glob("out/m1/**/*_kernel_trace.csv", recursive=True)):
    d = collections.defaultdict(list)
    for r in csv.DictReader(open(f)):
        d[r["Kernel_Name"]].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    print(os.path.basename(f))
    for k, v in sorted(d.items()):
        if "planes" not in k: continue
        v = v[-20:]
        print("   %-75s calls %3d  median %8.2f us  min %8.2f  max %8.2f" % (k[:75], len(v), statistics.median(v), min(v), max(v)))
