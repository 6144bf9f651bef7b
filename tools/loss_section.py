"""The loss section of a training step in a rocprofv3 kernel trace CSV of bench.py: every launch from the first view-synthesis kernel of
the step (the first kernel after the depth network's forward and the up-sampling of its maps) to the last kernel of the loss's backward
(after which the depth network's backward starts), on the queue those kernels run on.  Steps are delimited by the bursts of Adam
kernels (tools/step_breakdown.py); the first `skip` steps are left out.  Prints launches, summed kernel time and wall time (start of
the first to end of the last) per step, their medians, the launches of the median step by name, and the step's at::native launches.
usage: loss_section.py trace.csv [skip]"""
import collections
import csv
import re
import statistics
import sys

LOSS = re.compile(r'view_synthesis|photometric|sum_partials|sn_mean|sn_fwd|sn_bwd|smoothness|loss_combine|l1cand')

rows = list(csv.DictReader(open(sys.argv[1])))
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 3
for r in rows:
    r['s'], r['e'] = int(r['Start_Timestamp']), int(r['End_Timestamp'])
rows.sort(key=lambda r: r['s'])
adam = [i for i, r in enumerate(rows) if re.search(r'adam_flat_kernel|adam_pack_table_kernel|adam_segments_kernel|FusedAdam', r['Kernel_Name'])]
bursts, prev = [], None
for i in adam:
    if prev is None or i - prev > 50:
        bursts.append([i, i])
    else:
        bursts[-1][1] = i
    prev = i


def short(name):
    return re.sub(r'^void ', '', re.sub(r'\(.*', '', name))[:70]


steps = []
for k in range(skip, len(bursts) - 1):
    win = rows[bursts[k][1] + 1:bursts[k + 1][1] + 1]
    loss = [i for i, r in enumerate(win) if LOSS.search(r['Kernel_Name'])]
    if not loss:
        continue
    first = next(i for i in loss if 'view_synthesis_fwd' in win[i]['Kernel_Name'])
    queue = win[first].get('Queue_Id')
    sec = [r for r in win[first:loss[-1] + 1] if r.get('Queue_Id') == queue]
    native = [r for r in win if 'at::native' in r['Kernel_Name']]
    steps.append(dict(n=len(sec), kern=sum(r['e'] - r['s'] for r in sec) / 1e3, wall=(sec[-1]['e'] - sec[0]['s']) / 1e3, sec=sec,
                      step_wall=(win[-1]['e'] - win[0]['s']) / 1e6, launches=len(win), native=len(native),
                      native_us=sum(r['e'] - r['s'] for r in native) / 1e3))
print('%d steps (first %d skipped)' % (len(steps), skip))
print(' step  section launches  kernel us   wall us   | step launches  at::native (us)   step wall ms')
for i, s in enumerate(steps):
    print('%5d  %16d  %9.1f  %8.1f   | %13d  %6d (%6.1f)   %8.3f' % (i, s['n'], s['kern'], s['wall'], s['launches'], s['native'], s['native_us'],
                                                                   s['step_wall']))
med = lambda key: statistics.median(s[key] for s in steps)
print('median: %d launches, %.1f us of kernel time, %.1f us wall; step: %d launches, %d at::native, %.3f ms'
      % (med('n'), med('kern'), med('wall'), med('launches'), med('native'), med('step_wall')))
mid = sorted(steps, key=lambda s: s['wall'])[len(steps) // 2]
agg = collections.OrderedDict()
for r in mid['sec']:
    a = agg.setdefault(short(r['Kernel_Name']), [0, 0])
    a[0] += 1
    a[1] += r['e'] - r['s']
print('launches of the median step\'s section, in order of first appearance:')
for name, (cnt, ns) in agg.items():
    print('%4d  %8.1f us  %s' % (cnt, ns / 1e3, name))
