"""Image-stage timeline from a rocprofv3 kernel trace csv: per step, begin / end of the five image kernels relative to the
step's first image kernel, and which chain ends last.  usage: timeline.py TRACE_DIR TIMED_STEPS"""
import csv
import glob
import sys

d, timed = sys.argv[1], int(sys.argv[2])
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
rows = []
for r in csv.DictReader(open(f)):
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()


def tag(name):
    if "shadow_set_kernel" in name:
        return "set"
    if "shadow_image_kernel" in name:
        return "shB" if "12288" in name else "sh"
    if "grasp_image_kernel" in name:
        return "ptsB" if ("<true>" in name or "ILb1" in name) else "pts"
    return None


# a step = one run of image kernels: a new one begins with the first image kernel behind a kernel of another stage
steps = []
other = True
for s, e, n in rows:
    t = tag(n)
    if t is None:
        other = True
        continue
    if other:
        steps.append({})
        other = False
    steps[-1][t] = (s, e)
steps = [st for st in steps if all(k in st for k in ("set", "sh", "pts", "ptsB"))][-timed:]
print("names seen:", sorted({n[:70] for _, _, n in rows if tag(n)}))
print("| step | set | shadow_image | shadow<12288> | points | overflow points | A end | B end | B - A |")
print("|---|---|---|---|---|---|---|---|---|")
dur = {}
for i, st in enumerate(steps):
    t0 = min(v[0] for v in st.values())
    rel = {k: ((v[0] - t0) / 1e3, (v[1] - t0) / 1e3) for k, v in st.items()}
    a_end = max(rel[k][1] for k in ("set", "sh", "shB") if k in rel)
    b_end = max(rel[k][1] for k in ("pts", "ptsB"))
    for k, v in rel.items():
        dur.setdefault(k, []).append(v[1] - v[0])
    cell = lambda k: "%.0f-%.0f" % rel[k] if k in rel else "-"
    print("| %d | %s | %s | %s | %s | %s | %.0f | %.0f | %+.0f |" % (i, cell("set"), cell("sh"), cell("shB"), cell("pts"), cell("ptsB"), a_end, b_end, b_end - a_end))
print("mean durations us:", {k: round(sum(v) / len(v), 1) for k, v in dur.items()})
