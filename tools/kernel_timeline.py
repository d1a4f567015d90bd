"""dev aid: kernel sequence of the last DBSCAN call in a rocprofv3 --kernel-trace CSV, then the median
duration (with its smallest and largest value) of every kernel of a step and the median gap before it over all traced steps but the first `skip`
(python tools/kernel_timeline.py <dir>/<name>_kernel_trace.csv [first_kernel [count [skip]]])"""
import csv
import statistics
import sys

rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r['Start_Timestamp']))
names = [r['Kernel_Name'].split('(')[0].replace('pyqsm::', '') for r in rows]
first = sys.argv[2] if len(sys.argv) > 2 else 'k_bbox'
count = int(sys.argv[3]) if len(sys.argv) > 3 else 45
skip = int(sys.argv[4]) if len(sys.argv) > 4 else 2
begins = [i for i, nm in enumerate(names) if nm == first]
last = begins[-1]
t0 = int(rows[last]['Start_Timestamp'])
prev_end = None
span = gap_max = 0.0
for r, nm in list(zip(rows, names))[last:last + count]:  # the last step: nothing of a next one follows
    b, e = int(r['Start_Timestamp']), int(r['End_Timestamp'])
    gap = max(0.0, (b - prev_end) / 1e3) if prev_end is not None else 0.0
    gap_max = max(gap_max, gap)
    span = (e - t0) / 1e3
    prev_end = e
    print('%-32s start %8.1f us  duration %7.1f us  gap before %6.1f us' % (nm[:32], (b - t0) / 1e3, (e - b) / 1e3, gap))
print('# step span %.1f us, largest gap %.1f us' % (span, gap_max))
# the same kernels over the steps: the k-th kernel of a step under its name (#k for a repeated name)
dur, gaps, order = {}, {}, []
for s, b0 in enumerate(begins):
    if s < skip:
        continue
    seen = {}
    prev_end = None
    for r, nm in list(zip(rows, names))[b0:min(b0 + count, begins[s + 1] if s + 1 < len(begins) else len(rows))]:
        k = seen.get(nm, 0)
        seen[nm] = k + 1
        key = nm if k == 0 else '%s#%d' % (nm, k)
        if key not in dur:
            dur[key], gaps[key] = [], []
            order.append(key)
        b, e = int(r['Start_Timestamp']), int(r['End_Timestamp'])
        dur[key].append((e - b) / 1e3)
        gaps[key].append(max(0.0, (b - prev_end) / 1e3) if prev_end is not None else 0.0)
        prev_end = e
print('# median kernel duration and gap before it over steps %d..%d' % (skip + 1, len(begins)))
for key in order:
    print('%-36s %8.2f us  (n=%d, %.2f .. %.2f)  median gap before %5.1f us' % (
        key[:36], statistics.median(dur[key]), len(dur[key]), min(dur[key]), max(dur[key]), statistics.median(gaps[key])))
print('# sum of the median durations %.1f us' % sum(statistics.median(v) for v in dur.values()))
