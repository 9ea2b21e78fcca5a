"""Median per process, then the median over processes; the parent's spread = the largest relative difference between its own per-process medians."""
import json
import sys
from statistics import median

rows = [json.loads(line) for line in open(sys.argv[1])]
whats = []
for r in rows:
    if r["what"] not in whats:
        whats.append(r["what"])
print("| workload (ms) | parent | parent's processes | parent's spread | new | new's processes | new vs parent |")
print("|---|---|---|---|---|---|---|")
for w in whats:
    per = {}
    for pkg in ("parent", "new"):
        procs = sorted({r["process"] for r in rows if r["what"] == w and r["package"] == pkg})
        per[pkg] = [median([r["ms"] for r in rows if r["what"] == w and r["package"] == pkg and r["process"] == p]) for p in procs]
    pm, nm = median(per["parent"]), median(per["new"])
    spread = (max(per["parent"]) - min(per["parent"])) / min(per["parent"]) * 100
    diff = (nm - pm) / pm * 100
    verdict = "inside" if abs(diff) <= spread else "OUTSIDE"
    print(f"| `{w}` | {pm:.3f} | {min(per['parent']):.3f} .. {max(per['parent']):.3f} | {spread:.2f} % | {nm:.3f} | "
          f"{min(per['new']):.3f} .. {max(per['new']):.3f} | {diff:+.2f} % ({verdict}) |")
