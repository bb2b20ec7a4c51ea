"""the kernel trace of scripts/planes_batch/f1.py cut into its cases: median [min, max] in microseconds of the last 10 dispatches of
every plane kernel of a case.  python scripts/planes_batch/f1_sum.py OUT   (OUT holds cases.json and *_kernel_trace.csv)"""
import csv, glob, json, os, statistics, sys
out = sys.argv[1]
cases = json.load(open(os.path.join(out, "cases.json")))
rows = []
for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        if "planes" in r["Kernel_Name"]:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
at = 0
for c in cases:
    pat = c["pattern"]
    t = {}
    for rep in range(c["reps"]):
        for j, role in enumerate(pat):
            s, e, name = rows[at]
            at += 1
            assert role in name, (c["name"], role, name)
            t.setdefault((j, role, name.split("(")[0].split("<")[0]), []).append((e - s) / 1000.0)
    cells = []
    for (j, role, name), v in sorted(t.items()):
        v = v[-10:]
        cells.append("%s %.1f [%.1f, %.1f]" % (role if role != "map" else "map" + "sj"[j // 2], statistics.median(v), min(v), max(v)))
    extra = " pad %.1f%%" % (100.0 * c["pad_elems"] / c["m_total"]) if "pad_elems" in c else ""
    print("%-44s %s%s" % (c["name"], " | ".join(cells), extra))
assert at == len(rows), (at, len(rows))
