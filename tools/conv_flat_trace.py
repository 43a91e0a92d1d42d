#!/usr/bin/env python
"""Per-step time of the 1x1 kernels from two rocprofv3 kernel traces of the same bench command (parent, pull request):
    python tools/conv_flat_trace.py PARENT_kernel_trace.csv PR_kernel_trace.csv OUT.json [STEPS]
A step starts at a launch of the stem kernel; the last STEPS (default 50) steps of each trace are used.  Per step: the summed
duration of every 1x1 kernel (conv_flat_kernel and the 1x1 conv_pipe_kernel instantiations); mean and standard deviation over
the steps.  The two launch lists have the same length, so the launches at the positions where the pull request runs
conv_flat_kernel are the same layers in the parent: their summed duration per step is given too (launches that overlap the side
stream's kernels are long in both traces and stay in the sums)."""
import csv, json, re, statistics, sys

ONE = re.compile(r'conv_flat_kernel|conv_pipe_kernel<\w+, 1,')


def steps_of(path, nsteps):
    rows = sorted(((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name'], r.get('Queue_Id', '0')) for r in csv.DictReader(open(path))), key=lambda r: r[0])
    starts = [i for i, r in enumerate(rows) if 'stem' in r[2]]
    cuts = starts + [len(rows)]
    steps = [rows[cuts[i]:cuts[i + 1]] for i in range(len(starts))]
    n = max(set(len(s) for s in steps), key=[len(s) for s in steps].count)       # launches of a regular step
    # inside a step: queue by queue, each in launch order (the side stream's launches interleave differently from step to step)
    return [[r[:3] for r in sorted(s, key=lambda r: (r[3], r[0]))] for s in steps if len(s) == n][-nsteps:]


def summary(v):
    return dict(mean_us=round(statistics.mean(v) / 1e3, 2), stddev_us=round(statistics.pstdev(v) / 1e3, 2), median_us=round(statistics.median(v) / 1e3, 2), steps=len(v))


if __name__ == '__main__':
    nsteps = int(sys.argv[4]) if len(sys.argv) > 4 else 50
    par, pr = steps_of(sys.argv[1], nsteps), steps_of(sys.argv[2], nsteps)
    assert len(par[0]) == len(pr[0]), (len(par[0]), len(pr[0]))
    pos = [i for i, r in enumerate(pr[0]) if 'conv_flat_kernel' in r[2]]
    assert all(ONE.search(par[0][i][2]) for i in pos)
    out = {'launches_per_step': len(pr[0]), 'flat_launches_per_step': len(pos)}
    for who, st in (('parent', par), ('pull_request', pr)):
        out[who] = {'all_1x1_per_step': summary([sum(e - s for s, e, k in step if ONE.search(k)) for step in st]),
                    'flat_positions_per_step': summary([sum(step[i][1] - step[i][0] for i in pos) for step in st]),
                    'all_kernels_per_step': summary([sum(e - s for s, e, k in step) for step in st]),
                    'kernels_at_flat_positions': sorted(set(st[0][i][2] for i in pos))}
    json.dump(out, open(sys.argv[3], 'w'), indent=1)
    print(json.dumps(out, indent=1))
