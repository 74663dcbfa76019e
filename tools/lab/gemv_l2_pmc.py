#!/usr/bin/env python3
"""L2 hit rate per matvec launch from a counters-only rocprofv3 run (`--pmc TCC_HIT_sum TCC_MISS_sum --output-format csv`).

    tools/lab/gemv_l2_pmc.py DIR            the lab (tools/lab/gemv_l2_lab.hip): variant from the kernel's TAG, m from the grid
    tools/lab/gemv_l2_pmc.py DIR eigh       the library: trd_gemv_kernel<NCH> by trailing-size bin (m from the grid)

Prints a markdown table of TCC_HIT_sum / (TCC_HIT_sum + TCC_MISS_sum) (mean hits and misses per launch beside it)."""
import collections
import csv
import glob
import os
import re
import sys

VARIANTS = ['0 parent', 'A first asc', 'A first desc', 'all nt', 'B C=16', 'B C=20', 'B C=24', 'B C=28',
            'A+B C=16', 'A+B C=20', 'A+B C=24', 'A+B C=28', 'always desc']


def dispatches(path, needle):
    """{dispatch id: (kernel name, workgroups, {counter: value})} of the kernels whose name contains `needle`"""
    out = {}
    for f in glob.glob(os.path.join(path, '**', '*counter_collection.csv'), recursive=True):
        with open(f, newline='') as fh:
            for row in csv.DictReader(fh):
                if needle not in row['Kernel_Name']:
                    continue
                key = (f, row['Dispatch_Id'])
                d = out.setdefault(key, (row['Kernel_Name'], int(row['Grid_Size']) // int(row['Workgroup_Size']), {}))
                d[2][row['Counter_Name']] = d[2].get(row['Counter_Name'], 0.0) + float(row['Counter_Value'])
    return out.values()


def table(groups, head):
    print(f'| {head} | launches | TCC_HIT_sum | TCC_MISS_sum | hit rate |')
    print('|---|---:|---:|---:|---:|')
    for key in sorted(groups):
        rows = groups[key]
        hit = sum(r.get('TCC_HIT_sum', 0.0) for r in rows) / len(rows)
        miss = sum(r.get('TCC_MISS_sum', 0.0) for r in rows) / len(rows)
        label = key if isinstance(key, str) else ' | '.join(str(k) for k in key)
        print(f'| {label} | {len(rows)} | {hit:.0f} | {miss:.0f} | {hit / max(hit + miss, 1.0):.3f} |')


def lab(path):
    groups = collections.defaultdict(list)
    for name, wgs, ctr in dispatches(path, 'mv_kernel'):
        tag = int(re.search(r'mv_kernel<\d+, (\d+)>', name).group(1))
        groups[(f'{tag:2d} {VARIANTS[tag]}', 2 * wgs)].append(ctr)
    table(groups, 'variant | m')


def eigh(path):
    groups = collections.defaultdict(list)
    for name, wgs, ctr in dispatches(path, 'trd_gemv_kernel'):
        nch = re.search(r'trd_gemv_kernel<(\d+)>', name).group(1)
        m = 2 * wgs                                     # pad + m + 2 i rows: at most 47 more than m
        groups[(f'<{nch}>', f'{m // 256 * 256:4d}-{m // 256 * 256 + 255}')].append(ctr)
    table(groups, 'kernel | rows in the launch')


if __name__ == '__main__':
    (eigh if len(sys.argv) > 2 and sys.argv[2] == 'eigh' else lab)(sys.argv[1])
