"""The kernel boundary's own cost from a rocprofv3 kernel trace (profiles/collect.sh: <out>/stats/**/*kernel_trace.csv):
for consecutive dispatches of k_forward_backward, start-to-start minus the first one's duration -- the time between the end of
a launch and the start of the next, which holds the write-back of whatever the kernel left dirty in the L2s.
python profiles/tune/dispatch_gaps.py DIR_OR_CSV [skip]: `skip` leading dispatches are ignored (warm-up; default 10)."""
import csv, glob, os, sys
import numpy as np
src = sys.argv[1]
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 10
files = [src] if os.path.isfile(src) else glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True)
assert files, "no *kernel_trace.csv under " + src
rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(files[0])))
fb = [i for i, r in enumerate(rows) if "k_forward_backward" in r[2]][skip:]
dur, gap = [], []
for i in fb:
    dur.append(rows[i][1] - rows[i][0])
    if i + 1 < len(rows) and "k_forward_backward" in rows[i + 1][2]:  # back-to-back launches of the step only
        gap.append(rows[i + 1][0] - rows[i][1])
dur, gap = np.array(dur) / 1e3, np.array(gap) / 1e3
print("k_forward_backward: %d dispatches, duration us min %.2f median %.2f mean %.2f max %.2f" % (len(dur), dur.min(), np.median(dur), dur.mean(), dur.max()))
if len(gap):
    print("start-to-start minus duration (%d back-to-back pairs), us: min %.2f median %.2f mean %.2f max %.2f" %
          (len(gap), gap.min(), np.median(gap), gap.mean(), gap.max()))
