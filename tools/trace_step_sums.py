"""Per-step time of every kernel in rocprofv3 --kernel-trace CSVs, for A/B comparisons of two builds.

    python tools/trace_step_sums.py --out summary.csv TAG=path/to/x_kernel_trace.csv [TAG=...]

A kernel that is launched k times per step has k launch slots of different sizes, so a median over its launches mixes them.
Here the launches of a kernel (in start order) are cut from the end into chunks of k, each chunk holding every slot once; the
figure is the median over the last `--steps` chunks of the chunk's summed duration, in microseconds.  k is the kernel's launch
count divided by the count of the steps in the trace, which is taken from `--step-kernel` (a substring naming a kernel that
runs exactly once per step; default: the fused Adam update), rounded down: a few launches more than k per step are set-up
work at the start of the trace and fall outside the chunks.  Kernels with fewer launches than steps are listed with k = 0 and
the median over all their launches.
"""
import argparse
import csv
import re
import statistics
import sys
from collections import defaultdict


def short(name):
    name = name.replace('(anonymous namespace)::', '')
    name = re.sub(r'^void ', '', name)
    i = name.find('(')
    return (name if i < 0 else name[:i]).strip()


def load(path):
    per = defaultdict(list)
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            per[short(row['Kernel_Name'])].append((int(row['Start_Timestamp']), int(row['End_Timestamp'])))
    return {k: [(e - s) / 1e3 for s, e in sorted(v)] for k, v in per.items()}


def step_sums(durs, steps_in_trace, steps):
    n = len(durs)
    if steps_in_trace <= 0 or n < steps_in_trace:
        return 0, statistics.median(durs)
    k = n // steps_in_trace                                  # (launches beyond k per step are set-up work at the start)
    chunks = [sum(durs[n - (i + 1) * k:n - i * k]) for i in range(min(steps, steps_in_trace))]
    return k, statistics.median(chunks)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('traces', nargs='+', metavar='TAG=CSV')
    ap.add_argument('--out', required=True)
    ap.add_argument('--steps', type=int, default=16, help='chunks (steps) from the end of the trace to take the median over')
    ap.add_argument('--step-kernel', default='adam', help='substring of a kernel that runs once per step')
    a = ap.parse_args()
    rows = []
    for spec in a.traces:
        tag, path = spec.split('=', 1)
        per = load(path)
        once = [k for k in per if a.step_kernel.lower() in k.lower()]
        if not once:
            sys.exit(f'{path}: no kernel named like {a.step_kernel!r}')
        steps_in_trace = min(len(per[k]) for k in once)
        for name, durs in sorted(per.items()):
            k, med = step_sums(durs, steps_in_trace, a.steps)
            rows.append((tag, name, len(durs), k, f'{med:.2f}'))
    with open(a.out, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(('run', 'kernel', 'launches', 'per_step', 'median_us_per_step'))
        w.writerows(rows)
    print(f'{len(rows)} rows -> {a.out}')


if __name__ == '__main__':
    main()
