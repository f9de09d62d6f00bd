"""Per-step durations and gaps of the pruned exact sweep's dispatches, read from a rocprofv3 trace of bench.py
(rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -- python bench.py --steps 30 --warmup 5):
    python benchmarks/exact_chain_trace.py DIR [steps]
A step is the estimate launch (a sweep kernel of under 0.2 ms), its merge, the gated launch, its merge and any device-to-host
copy up to the next estimate launch; the last `steps` complete steps are read.  profiles/exact_fold/README.md has the numbers."""
import csv, glob, sys, statistics as S
d = sys.argv[1]
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
K = list(csv.DictReader(open(glob.glob(d + '/*/*kernel_trace.csv')[0])))
M = list(csv.DictReader(open(glob.glob(d + '/*/*memory_copy_trace.csv')[0])))
ev = []
for r in K:
    n = r['Kernel_Name']
    kind = 'sweep' if 'exact_kernel' in n else 'merge' if 'merge_rank' in n else None
    if kind: ev.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), kind, n))
for r in M:
    if r['Direction'].endswith('DEVICE_TO_HOST'): ev.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), 'd2h', ''))
ev.sort()
q = []
idx = 0
while idx < len(ev):
    if ev[idx][2] == 'sweep' and (ev[idx][1] - ev[idx][0]) < 200000:
        j = idx + 1
        grp = [ev[idx]]
        while j < len(ev) and not (ev[j][2] == 'sweep' and (ev[j][1] - ev[j][0]) < 200000):
            grp.append(ev[j]); j += 1
        q.append(grp); idx = j
    else:
        idx += 1
q = [g for g in q if sum(1 for e in g if e[2] == 'sweep') == 2][-steps:]
def med(xs):
    xs = [x / 1000.0 for x in xs]
    return '%.2f us (%.2f-%.2f)' % (S.median(xs), min(xs), max(xs)) if xs else 'none'
print('steps read:', len(q), ' dispatches per step:', sorted(set(sum(1 for e in g if e[2] != 'd2h') for g in q)), ' d2h copies per step:', sorted(set(sum(1 for e in g if e[2] == 'd2h') for g in q)))
est = [g[0] for g in q]
print('estimate launch          ', med([e[1] - e[0] for e in est]))
gated = [[e for e in g if e[2] == 'sweep'][1] for g in q]
print('gated launch             ', med([e[1] - e[0] for e in gated]))
if any(e[2] == 'merge' for g in q for e in g):
    m1 = [[e for e in g if e[2] == 'merge'][0] for g in q]
    m2 = [[e for e in g if e[2] == 'merge'][1] for g in q]
    print('seed merge               ', med([e[1] - e[0] for e in m1]))
    print('final merge              ', med([e[1] - e[0] for e in m2]))
    print('gap estimate end -> seed merge start ', med([m[0] - e[1] for m, e in zip(m1, est)]))
    print('gap seed merge end -> gated start    ', med([g_[0] - m[1] for m, g_ in zip(m1, gated)]))
    print('gap gated end -> final merge start   ', med([m[0] - g_[1] for m, g_ in zip(m2, gated)]))
    cp = [[e for e in g if e[2] == 'd2h'] for g in q]
    if all(cp):
        print('copy start - final merge end         ', med([c[0][0] - m[1] for c, m in zip(cp, m2)]))
        print('copy end   - final merge end         ', med([c[0][1] - m[1] for c, m in zip(cp, m2)]))
        print('chain: estimate start -> copy end    ', med([c[0][1] - e[0] for c, e in zip(cp, est)]))
    print('chain: estimate start -> final merge end', med([m[1] - e[0] for m, e in zip(m2, est)]))
    print('sum of the four kernels  ', med([sum(e[1] - e[0] for e in g if e[2] != 'd2h') for g in q]))
else:
    print('gap estimate end -> gated start      ', med([g_[0] - e[1] for g_, e in zip(gated, est)]))
    print('chain: estimate start -> gated end   ', med([g_[1] - e[0] for g_, e in zip(gated, est)]))
    print('sum of the two kernels   ', med([sum(e[1] - e[0] for e in g if e[2] != 'd2h') for g in q]))
print('step to step (estimate start to next estimate start)', med([b[0][0] - a[0][0] for a, b in zip(q, q[1:])]))
