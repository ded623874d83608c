"""The batch norm's four launches inside the step, from a rocprofv3 --kernel-trace CSV of bench.py: per launch (the statistics launch
delimits the steps) min / median / max of its duration over the last 15 steps, and of the distance from the start of the statistics
launch to the end of the apply launch (the forward pair with the gap between them):  tools/bn_in_step.py <dir or kernel_trace.csv>"""
import csv, glob, os, statistics, sys
path = sys.argv[1]
if os.path.isdir(path):
    path = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))[-1]
rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
marks = [i for i, r in enumerate(rows) if "bn_stats_prep_kernel" in r["Kernel_Name"] or "bn_stats_kernel" in r["Kernel_Name"]]
steps = [(marks[i], marks[i + 1]) for i in range(len(marks) - 1)][-16:-1]
want = {"bn_stats": ("bn_stats_prep_kernel", "bn_stats_kernel"), "bn_apply": ("bn_apply_kernel",), "bn_bwd_partial": ("bn_bwd_partial_kernel",),
        "bn_bwd_final": ("bn_bwd_final_kernel",)}
per = {k: [] for k in want}
pair, spans = [], []
for s, e in steps:
    spans.append((int(rows[e]["Start_Timestamp"]) - int(rows[s]["Start_Timestamp"])) / 1e3)
    for k, pats in want.items():
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[s:e] if any(p in r["Kernel_Name"] for p in pats)]
        assert len(d) == 1, (k, len(d))
        per[k].append(d[0])
    apply_end = [int(r["End_Timestamp"]) for r in rows[s:e] if "bn_apply_kernel" in r["Kernel_Name"]][0]
    pair.append((apply_end - int(rows[s]["Start_Timestamp"])) / 1e3)
print(f"# {len(steps)} steps; min / median / max us")
for k, v in list(per.items()) + [("stats start .. apply end", pair), ("step span", spans)]:
    print(f"{k}: {min(v):.1f} / {statistics.median(v):.1f} / {max(v):.1f}")
