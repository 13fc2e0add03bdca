"""Per-kernel summary of one `rocprofv3 --kernel-trace --stats` run of `harness train-step` (profiles/r04/collect.sh):
    python profiles/r04/summarize.py <dir with the rocpd .db> <out.csv> <optimisation steps in the run>

Writes one row per kernel (calls, total / average / min / max ns, share of the GPU kernel time, class) and prints one JSON
line: dispatches per step and the share of kernel time per class.  Classes: `eig` = the library's eigensolver kernels,
`contract` = vdvh_kernel / vhsv_kernel, `train_layer` = the fused layer kernels of csrc/train_layer.hip, `train_small` = the
O(B D)-sized step kernels of csrc/train_small.hip (route "full"), `framework` = everything else (ATen elementwise / copy / reduce / cat kernels, rocBLAS GEMMs of the MLPs, the optimiser).
"""
import csv
import json
import os
import re
import sqlite3
import subprocess
import sys
from collections import defaultdict



def short(name):
    """rocpd stores the mangled symbol (`_ZN7admmnet...kd`): c++filt it, drop the argument list."""
    raw = name[:-3] if name.endswith(".kd") else name
    if raw.startswith("_Z"):
        try:
            raw = subprocess.run(["c++filt", raw], capture_output=True, text=True, check=True).stdout.strip() or raw
        except (OSError, subprocess.CalledProcessError):
            pass
    return re.sub(r"\(.*$", "", raw).replace("void ", "").strip()


def klass(name):
    """name: demangled, argument list dropped.  The library's kernels all live in namespace admmnet."""
    if "admmnet::" not in name:
        return "framework"
    if "vdvh_kernel" in name or "vhsv_kernel" in name:
        return "contract"
    if "admmnet::tl_" in name:
        return "train_layer"
    if "admmnet::ts_" in name:
        return "train_small"
    return "eig"      # every other library kernel on this path belongs to admmnet_eigh_c64


def main():
    src, out, steps = sys.argv[1], sys.argv[2], int(sys.argv[3])
    dbs = [os.path.join(r, f) for r, _, fs in os.walk(src) for f in fs if f.endswith(".db")]
    c = sqlite3.connect(dbs[0])
    rows = c.execute("select s.kernel_name, d.start, d.end from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s "
                     "on d.kernel_id = s.id").fetchall()
    agg, names = defaultdict(list), {}
    for name, st, en in rows:
        if name not in names:
            names[name] = short(name)
        agg[names[name]].append(en - st)
    tot = sum(sum(v) for v in agg.values())
    share, calls = defaultdict(float), defaultdict(int)
    with open(out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Name", "Class", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "Percentage"])
        for k, v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
            w.writerow([k.replace("admmnet::", ""), klass(k), len(v), sum(v), round(sum(v) / len(v), 1), min(v), max(v), round(100.0 * sum(v) / tot, 3)])
            share[klass(k)] += sum(v)
            calls[klass(k)] += len(v)
    print(json.dumps({"dispatches": len(rows), "steps": steps, "dispatches_per_step": round(len(rows) / steps, 1),
                      "kernel_ms_per_step": round(tot / steps / 1e6, 3),
                      "share_pct": {k: round(100.0 * v / tot, 2) for k, v in share.items()},
                      "dispatches_per_step_by_class": {k: round(v / steps, 1) for k, v in calls.items()}}))


if __name__ == "__main__":
    main()
