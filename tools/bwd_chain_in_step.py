"""The backward chain's launches inside the step, from a rocprofv3 --kernel-trace CSV of bench.py: per launch position in the step
(delimited by the batch norm's statistics launches) the duration of the pre-pass, the N-hop rows kernels, the N-hop gathers and the
bank kernels, min / median / max over the last 15 steps:  tools/bwd_chain_in_step.py <dir or kernel_trace.csv>"""
import csv, glob, os, re, statistics, sys
path = sorted(glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True))[-1]
rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
marks = [i for i, r in enumerate(rows) if "bn_stats_prep_kernel" in r["Kernel_Name"] or "bn_stats_kernel" in r["Kernel_Name"]]
steps = [(marks[i], marks[i + 1]) for i in range(len(marks) - 1)][-16:-1]
want = {"rows<7>": r"kc_backward_rows_stream<7", "gather<32>": r"csr_rows_kernel<32, true", "coef_prepare": r"coef_prepare_kernel",
        "bank<7>": r"kc_backward_bank_stream<7"}
per = {k: [] for k in want}
spans = []
for s, e in steps:
    spans.append((int(rows[e]["Start_Timestamp"]) - int(rows[s]["Start_Timestamp"])) / 1e3)
    for k, pat in want.items():
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[s:e] if pat in r["Kernel_Name"]]
        per[k].append(d)
print(f"# {len(steps)} steps; per launch position in the step: min / median / max us")
for k, lists in per.items():
    n = min(len(d) for d in lists) if lists else 0
    for j in range(n):
        v = [d[j] for d in lists]
        print(f"{k} launch {j}: {min(v):.1f} / {statistics.median(v):.1f} / {max(v):.1f}")
print(f"step span: {min(spans):.1f} / {statistics.median(spans):.1f} / {max(spans):.1f}")
