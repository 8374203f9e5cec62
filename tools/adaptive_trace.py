#!/usr/bin/env python3
"""Per-kernel durations of adaptive supersampling from a rocprofv3 kernel
trace of tools/adaptive_time.py: the dispatches grouped by kernel and grid
size (the plain frame's and the sample frame's integrate and shade launches
are the same kernels at different grids), the first --skip dispatches of each
group left out as warm-up. One JSON line.

  rocprofv3 --kernel-trace --stats --output-format csv -d RUN_DIR -- \\
      python tools/adaptive_time.py --ss 4 --thresholds 254 --legs adaptive --rounds 1
  python tools/adaptive_trace.py RUN_DIR [--skip 8]
"""
import argparse
import csv
import glob
import json
import re


def short(name):
    m = re.match(r"(?:void )?(?:\(anonymous namespace\)::)?(\w+)", name)
    base = m.group(1) if m else name
    t = re.search(r"<([^>]*)>", name)
    return base + (f"<{t.group(1)}>" if t else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("run")
    ap.add_argument("--skip", type=int, default=8)
    a = ap.parse_args()
    groups = {}
    for p in glob.glob(f"{a.run}/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(p)):
            grid = "x".join(str(r[k]) for k in sorted(r) if k.startswith("Grid_Size"))
            key = (short(r["Kernel_Name"]), grid)
            groups.setdefault(key, []).append((int(r["Dispatch_Id"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    out = []
    for (name, grid), v in sorted(groups.items()):
        us = [d for _, d in sorted(v)][a.skip:] or [d for _, d in sorted(v)]
        out.append({"kernel": name, "grid": grid, "dispatches": len(v), "us_mean": round(sum(us) / len(us), 2),
                    "us_min": round(min(us), 2), "us_max": round(max(us), 2)})
    print(json.dumps({"tool": "adaptive_trace", "skip": a.skip, "kernels": out}))


if __name__ == "__main__":
    main()
