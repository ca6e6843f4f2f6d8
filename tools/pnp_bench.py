#!/usr/bin/env python
"""Absolute-pose (PnP) registration on the MI355X: the figures of DESIGN.md section 7 -> profiles/pnp_bench.json.

    python tools/pnp_bench.py [--out profiles/pnp_bench.json] [--reps 7]

Per shape (hypotheses x points: 400 x 2048 and the test shape 400 x 192, synthetic.pnp_scene): wall clock of one PnPRANSAC call
on fixed samples (ps_pnp_ransac: upload, every launch, the one download that synchronises), median of `--reps` calls after a
warm-up call, with the refinement and without; the same for ps_pnp_hypotheses alone; the restatement (pipelines/absolute.py) once
on the same input; and whether the two agree.  A host clock around a call that ends in a synchronising copy: a call time, not a
kernel time (kernel times: rocprofv3 --kernel-trace --stats, a run of its own)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from pyslam_amd import synthetic  # noqa: E402
from pyslam_amd.pipelines import absolute, pnp  # noqa: E402
from pyslam_amd.sensors import MonoCamera  # noqa: E402


def timed(fn, reps):
    fn()                                                 # warm-up: code object, allocator
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, {'ms_median': float(np.median(t)), 'ms_min': float(np.min(t)), 'ms_max': float(np.max(t))}


def figures(num_pts, num_hyp, reps):
    cam = MonoCamera(*synthetic.TWO_VIEW_CAMERA)
    pts, obs, T, outlier = synthetic.pnp_scene(num_pts=num_pts)
    rs = pnp.PnPRANSAC(cam)
    rs.ransac_iters = num_hyp
    rs.set_obs(pts, obs)
    np.random.seed(5)
    samples = rs.draw_samples()
    out = {'hypotheses': num_hyp, 'points': num_pts, 'reps': reps}
    res, out['ransac_refine'] = timed(lambda: rs._device_ransac(samples), reps)
    rs.refine = False
    raw, out['ransac_no_refine'] = timed(lambda: rs._device_ransac(samples), reps)
    _, out['hypotheses_only'] = timed(lambda: rs._device_hypotheses(samples), reps)
    t0 = time.perf_counter()
    ref = absolute.ransac(pts, obs, cam.intrinsics(), samples, rs.ransac_thresh)
    out['host_restatement_ms'] = (time.perf_counter() - t0) * 1e3
    out['inliers_raw'], out['inliers_final'], out['refine_kept'] = raw['count'], res['count'], res['refine_kept']
    out['true_inliers'] = int((~outlier).sum())
    out['winner_equals_restatement'] = bool((res['best'], res['best_slot']) == (ref['best'], ref['best_slot']))
    out['masks_equal_restatement'] = bool(np.array_equal(res['mask'], ref['mask']))
    out['T_max_abs_diff_to_restatement'] = float(np.abs(res['T_cw'] - ref['T_cw']).max())
    out['T_max_abs_diff_to_truth'] = float(np.abs(res['T_cw'] - T).max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'pnp_bench.json'))
    ap.add_argument('--reps', type=int, default=7)
    a = ap.parse_args()
    from pyslam_amd import _native as nat
    nat.require_gpu()                                    # no device: fail, do not time the host
    res = {'build_sha': nat.load().ps_build_sha().decode()}
    for name, (h, n) in {'400x2048': (400, 2048), 'test_shape_400x192': (400, 192)}.items():
        res[name] = figures(n, h, a.reps)
        print(json.dumps({name: res[name]}), flush=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
