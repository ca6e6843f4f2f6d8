#!/usr/bin/env python
"""Monocular BA and multi-view triangulation on the MI355X: the figures of DESIGN.md section 7 -> profiles/mono_bench.json.

    python tools/mono_bench.py [--out profiles/mono_bench.json] [--c4]

  iteration      ms per LM iteration (ps_gn_iteration, warm, median of `--iters` calls from the same perturbed start) and CG
                 iterations per LM iteration of synthetic.mono_ba(200, 50000) beside synthetic.stereo_ba(200, 50000) -- the
                 same scene, keyframes, landmarks and observation lists; the monocular one holds two poses, the stereo one
                 one.  pcg_max_iters reached is reported.
  triangulation  all 50 000 landmarks (and, with --c4, the 500 000 of mono_ba(2000, 500000)) at the true poses: wall clock of
                 ps_triangulate with refine_iters = 0 (the linear start) and 5, per refinement step = their difference / 5
                 (median of `--reps` calls, one synchronisation each), beside the numpy restatement on the same input.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from pyslam_amd import synthetic, triangulation  # noqa: E402
from pyslam_amd.device import DeviceProblem  # noqa: E402

PCG_MAX = 2000


def iteration_figures(lp, iters):
    dev = DeviceProblem(lp)
    ms, cg = [], []
    for k in range(iters + 2):
        dev.set_params(lp.poses, lp.points)
        dev.reset_solver_state()
        t0 = time.perf_counter()
        cost, nrm, its, rel = dev.gn_iteration(0., 0., PCG_MAX, True)
        if k >= 2:                                   # (two warm-up calls)
            ms.append((time.perf_counter() - t0) * 1e3)
            cg.append(its)
    # a whole solve: CG iterations of every LM iteration
    dev.set_params(lp.poses, lp.points)
    dev.reset_solver_state()
    per_iter = []
    for _ in range(6):
        per_iter.append(int(dev.gn_iteration(0., 0., PCG_MAX, True)[2]))
    dev.close()
    return {'ms_per_iteration_median': float(np.median(ms)), 'ms_per_iteration_min': float(np.min(ms)), 'ms_per_iteration_max': float(np.max(ms)),
            'cg_iterations_first': int(np.median(cg)), 'cg_iterations_six_iterations': per_iter,
            'pcg_max_iters': PCG_MAX, 'pcg_max_reached': bool(max(per_iter + cg) >= PCG_MAX)}


def triangulation_figures(lp, truth, reps, min_parallax_deg=0.05):
    lp = lp.copy()
    lp.poses = synthetic.pack_pose_matrices(truth['poses'])
    dev = DeviceProblem(lp)
    out = {'landmarks': int(lp.num_var_points), 'observations': int(lp.num_obs), 'min_parallax_deg': min_parallax_deg}
    for iters in (0, 5):
        dev.triangulate(None, iters, min_parallax_deg, write_back=False)
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            pts, st = dev.triangulate(None, iters, min_parallax_deg, write_back=False)
            t.append((time.perf_counter() - t0) * 1e3)
        out['device_ms_refine_{}'.format(iters)] = float(np.median(t))
        out['device_ms_refine_{}_min_max'.format(iters)] = [float(np.min(t)), float(np.max(t))]
        out['status_counts_refine_{}'.format(iters)] = np.bincount(st, minlength=4).tolist()
    out['device_ms_per_refinement_step'] = (out['device_ms_refine_5'] - out['device_ms_refine_0']) / 5.
    dev.close()
    t0 = time.perf_counter()
    want, wst = triangulation.triangulate(lp, None, 5, min_parallax_deg)
    out['host_restatement_ms_refine_5'] = (time.perf_counter() - t0) * 1e3
    ok = (st == 0) & (wst == 0)
    out['status_equal'] = bool(np.array_equal(st, wst))
    out['max_rel_diff_to_restatement'] = float((np.linalg.norm(pts[ok] - want[ok], axis=1) / np.linalg.norm(want[ok], axis=1)).max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mono_bench.json'))
    ap.add_argument('--iters', type=int, default=11)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--c4', action='store_true')
    a = ap.parse_args()
    res = {}
    mono, truth = synthetic.mono_ba(200, 50000, 10, 20, seed=0)
    stereo, _ = synthetic.stereo_ba(200, 50000, 10, 20, seed=0)
    res['iteration'] = {'mono_ba_200x50000': iteration_figures(mono, a.iters), 'stereo_ba_200x50000': iteration_figures(stereo, a.iters)}
    print(json.dumps(res['iteration']), flush=True)
    res['triangulation'] = {'c3_200x50000': triangulation_figures(mono, truth, a.reps)}
    print(json.dumps(res['triangulation']), flush=True)
    if a.c4:
        mono4, truth4 = synthetic.mono_ba(2000, 500000, 10, 20, seed=1)
        res['triangulation']['c4_2000x500000'] = triangulation_figures(mono4, truth4, a.reps)
        print(json.dumps(res['triangulation']['c4_2000x500000']), flush=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
