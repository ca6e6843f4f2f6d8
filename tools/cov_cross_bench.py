#!/usr/bin/env python
"""Pose-landmark and landmark-landmark covariance blocks (ps_covariance_cross_blocks) against the per-column route
(ps_covariance_column) at C3 and C4, built as tools/cov_marginals_bench.py builds them (synthetic.stereo_ba: 200 / 2 000
keyframes, 50 000 / 500 000 landmarks, 10 observations each).

Per size, host wall clock around calls that end in a device synchronisation, median of --repeats:
  setup_ms              ps_covariance_begin + ps_covariance_marginals (poses only): the Sigma_pp the cross blocks read
  obs_pairs             observations of a variable landmark on a variable pose
  all_obs_ms            every observation's (pose, landmark) block in ONE ps_covariance_cross_blocks call (chunks of
                        PS_COV_CROSS_CHUNK pairs, results read back into pageable host memory)
  ll_pairs / ll_ms      --ll-pairs random landmark-landmark pairs (l1 != l2) in one call
  column_ms             one landmark column (ps_covariance_column kind 1 + ps_get_dx), mean over --columns columns
  all_obs_column_s      column_ms x 3 x (landmarks with an observation on a variable pose): the column route's time for the
                        same blocks (three columns per landmark give all its pose blocks), extrapolated
  ll_column_s           column_ms x 3 x (distinct second landmarks of the pairs), extrapolated
The kernel split of one set-up + all-observation call + landmark-pair call comes from a separate profiler run (--one under
rocprofv3 --kernel-trace --stats, merged with --kernel-stats).

    python tools/cov_cross_bench.py [--repeats 3] [--columns 24] [--out profiles/cov_cross_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o cross -- python tools/cov_cross_bench.py --one C3
    python tools/cov_cross_bench.py --kernel-stats DIR/.../cross_kernel_stats.csv [--stats-size C3] --out profiles/cov_cross_bench.json
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))

import numpy as np  # noqa: E402

from cov_marginals_bench import SIZES, kernel_stats, make, timed  # noqa: E402,F401


def obs_pairs(dev):
    lp = dev.lp
    rid = lp.pose_rid[lp.obs_pose]
    vid = lp.point_vid[lp.obs_point]
    keep = (rid >= 0) & (vid >= 0)
    return rid[keep].astype(np.int32), vid[keep].astype(np.int32)


def ll_pairs(dev, n, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.integers(dev.nv, size=n).astype(np.int32)
    b = ((a + rng.integers(1, dev.nv, size=n)) % dev.nv).astype(np.int32)
    return a, b


def setup(dev):
    dev.covariance_begin()
    from pyslam_amd import _native as nat
    pose = np.zeros((dev.nr, dev.dof, dev.dof))
    nat.check(dev._lib.ps_covariance_marginals(dev._h, nat.f64p(pose), None))


def measure(size, repeats, ncols, nll):
    dev = make(size)
    try:
        rid, vid = obs_pairs(dev)
        z, o = np.zeros_like(rid), np.ones_like(rid)
        la, lb = ll_pairs(dev, nll)
        lo = np.ones_like(la)
        setup(dev)
        dev.covariance_cross_blocks(z[:1000], rid[:1000], o[:1000], vid[:1000])     # warm-up: code object, pair buffer
        setups, obs, ll = [], [], []
        for _ in range(repeats):
            setups.append(timed(lambda: setup(dev))[0])
            obs.append(timed(lambda: dev.covariance_cross_blocks(z, rid, o, vid))[0])
            ll.append(timed(lambda: dev.covariance_cross_blocks(lo, la, lo, lb))[0])
        # the existing route: one reduced solve + back-substitution + read-back per landmark column
        dev.covariance_column(1, 0, 0)
        cols = []
        for q in range(ncols):
            v = (q * 7919) % dev.nv
            cols.append(timed(lambda: dev.covariance_column(1, v, q % 3))[0])
        med = lambda v: float(np.median(v))       # noqa: E731
        col_ms = float(np.mean(cols))
        nlm_obs = int(np.unique(vid).size)
        nlm_ll = int(np.unique(lb).size)
        return {'num_reduced_poses': dev.nr, 'num_var_points': dev.nv, 'reduced_unknowns': 6 * dev.nr,
                'setup_ms': med(setups), 'obs_pairs': int(rid.size), 'all_obs_ms': med(obs),
                'all_obs_us_per_pair': med(obs) * 1e3 / rid.size, 'all_obs_readback_bytes': int(rid.size) * 36 * 8,
                'll_pairs': nll, 'll_ms': med(ll),
                'column_ms': col_ms, 'column_ms_min': float(np.min(cols)), 'column_ms_max': float(np.max(cols)),
                'columns_timed': ncols, 'all_obs_columns': 3 * nlm_obs, 'all_obs_column_s': col_ms * 3 * nlm_obs * 1e-3,
                'll_columns': 3 * nlm_ll, 'll_column_s': col_ms * 3 * nlm_ll * 1e-3, 'column_route_extrapolated': True}
    finally:
        dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--columns', type=int, default=24)
    ap.add_argument('--ll-pairs', type=int, default=10000)
    ap.add_argument('--sizes', default='C3,C4')
    ap.add_argument('--out', default=None)
    ap.add_argument('--one', default=None, help='one set-up + all-observation + landmark-pair call at this size (for a profiler)')
    ap.add_argument('--kernel-stats', default=None, help='rocprofv3 kernel_stats.csv of a --one run: merged into --out')
    ap.add_argument('--stats-size', default='C3', help='the size of that --one run')
    a = ap.parse_args()
    if a.one:
        dev = make(a.one)
        rid, vid = obs_pairs(dev)
        la, lb = ll_pairs(dev, a.ll_pairs)
        setup(dev)
        dev.covariance_cross_blocks(np.zeros_like(rid), rid, np.ones_like(rid), vid)
        dev.covariance_cross_blocks(np.ones_like(la), la, np.ones_like(la), lb)
        dev.close()
        return
    if a.kernel_stats is not None:
        res = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
        res['{}_one_call_kernel_stats'.format(a.stats_size)] = kernel_stats(a.kernel_stats)
    else:
        from __graft_entry__ import source_sha
        res = {'tool': 'tools/cov_cross_bench.py', 'device': 'MI355X', 'source_sha16': source_sha(), 'repeats': a.repeats}
        for s in a.sizes.split(','):
            res[s] = measure(s, a.repeats, a.columns, a.ll_pairs)
            print(s, json.dumps(res[s]), flush=True)
    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
