#!/usr/bin/env python
"""Batched marginal covariances (ps_covariance_marginals) against the per-column route (ps_covariance_column) at C3 and C4
(synthetic.stereo_ba as bench.py builds them: 200 / 2 000 keyframes, 50 000 / 500 000 landmarks, 10 observations each).

Per size, host wall clock around calls that end in a device synchronisation, median of --repeats:
  begin_ms            ps_covariance_begin (linearisation at lambda = 0, solver set-up)
  poses_ms            ps_covariance_marginals without landmark output: densify + Cholesky + L^-1 + Sigma = L^-T L^-1 + the pose
                      blocks' gather and read-back
  all_ms              ps_covariance_marginals with every pose and landmark block
  landmarks_ms        all_ms - poses_ms: landmark kernel + read-back of 9 nv doubles + the slot -> vid reordering on the host
  readback_ms         a device -> host copy of the landmark blocks' bytes alone (torch, pageable memory)
  column_ms           one ps_covariance_column + ps_get_dx (the existing route), mean over --columns columns
  column_route_s      column_ms x (6 nr + 3 nv): the existing route's time for the same marginals, extrapolated
The kernel split of one C3 call comes from a separate profiler run (--one C3 under rocprofv3 --kernel-trace --stats, merged
with --kernel-stats).

    python tools/cov_marginals_bench.py [--repeats 3] [--columns 24] [--out profiles/cov_marginals_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -o cov -- python tools/cov_marginals_bench.py --one C3
    python tools/cov_marginals_bench.py --kernel-stats DIR/.../cov_kernel_stats.csv --out profiles/cov_marginals_bench.json
"""
import argparse
import csv
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

SIZES = {'C3': dict(num_kf=200, num_lm=50000, seed=0), 'C4': dict(num_kf=2000, num_lm=500000, seed=1)}


def make(size):
    from pyslam_amd import synthetic
    from pyslam_amd.device import DeviceProblem
    lp, _ = synthetic.stereo_ba(obs_per_lm=10, half_window=20, **SIZES[size])
    return DeviceProblem(lp)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def marginals(dev, with_points):
    from pyslam_amd import _native as nat
    pose = np.zeros((dev.nr, dev.dof, dev.dof))
    point = np.zeros((dev.nv, 3, 3)) if with_points else None
    nat.check(dev._lib.ps_covariance_marginals(dev._h, nat.f64p(pose), nat.f64p(point)))
    return pose, point


def measure(size, repeats, ncols):
    import torch
    dev = make(size)
    try:
        begin, poses, full = [], [], []
        dev.covariance_begin()
        marginals(dev, True)                       # warm-up: code objects, the dense block's allocation
        for _ in range(repeats):
            begin.append(timed(dev.covariance_begin)[0])
            poses.append(timed(lambda: marginals(dev, False))[0])
            full.append(timed(lambda: marginals(dev, True))[0])
        nbytes = dev.nv * 9 * 8
        buf = torch.zeros(dev.nv * 9, dtype=torch.float64, device='cuda')
        buf.cpu()
        rb = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            rb.append(timed(lambda: buf.cpu())[0])
        # the existing route: one reduced solve + back-substitution + read-back per scalar unknown
        dev.covariance_column(0, 0, 0)
        cols = []
        for q in range(ncols):
            kind = q % 2
            index = (q * 7919) % (dev.nr if kind == 0 else dev.nv)
            cols.append(timed(lambda: dev.covariance_column(kind, index, q % (6 if kind == 0 else 3)))[0])
        med = lambda v: float(np.median(v))       # noqa: E731
        ncol_total = 6 * dev.nr + 3 * dev.nv
        col_ms = float(np.mean(cols))
        return {'num_reduced_poses': dev.nr, 'num_var_points': dev.nv, 'reduced_unknowns': 6 * dev.nr,
                'begin_ms': med(begin), 'poses_ms': med(poses), 'all_ms': med(full), 'landmarks_ms': med(full) - med(poses),
                'readback_ms': med(rb), 'readback_bytes': nbytes,
                'column_ms': col_ms, 'column_ms_min': float(np.min(cols)), 'column_ms_max': float(np.max(cols)), 'columns_timed': ncols,
                'columns_for_all_marginals': ncol_total, 'column_route_s': col_ms * ncol_total * 1e-3,
                'column_route_extrapolated': True, 'marginals_total_ms': med(begin) + med(full)}
    finally:
        dev.close()


def kernel_stats(path):
    rows = list(csv.DictReader(open(path)))
    out = []
    for r in rows:
        out.append({'kernel': r.get('Name', r.get('KernelName', '')), 'calls': int(r.get('Calls', 0)),
                    'total_ms': float(r.get('TotalDurationNs', 0)) * 1e-6, 'percent': float(r.get('Percentage', 0))})
    out.sort(key=lambda d: -d['total_ms'])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--columns', type=int, default=24)
    ap.add_argument('--sizes', default='C3,C4')
    ap.add_argument('--out', default=None)
    ap.add_argument('--one', default=None, help='one ps_covariance_begin + ps_covariance_marginals at this size (for a profiler)')
    ap.add_argument('--kernel-stats', default=None, help='rocprofv3 kernel_stats.csv of a --one C3 run: merged into --out')
    a = ap.parse_args()
    if a.one:
        dev = make(a.one)
        dev.covariance_begin()
        marginals(dev, True)
        dev.close()
        return
    if a.kernel_stats:
        res = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
        res['C3_one_call_kernel_stats'] = kernel_stats(a.kernel_stats)
    else:
        from __graft_entry__ import source_sha
        res = {'tool': 'tools/cov_marginals_bench.py', 'source_sha16': source_sha(), 'repeats': a.repeats}
        for s in a.sizes.split(','):
            res[s] = measure(s, a.repeats, a.columns)
            print(s, json.dumps(res[s]), flush=True)
    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
