#!/usr/bin/env python
"""Similarity (Sim(3)) alignment on the MI355X: the figures of DESIGN.md section 7 -> profiles/sim3_bench.json.

    python tools/sim3_bench.py [--out profiles/sim3_bench.json] [--reps 9]

Per shape (hypotheses x points: 400 x 2000 and 400 x 20000): wall clock of one Sim3RANSAC call on fixed samples (ps_sim3_ransac:
upload, every launch, the one download that synchronises) in the pixel mode with the refit and without, and in the metric mode;
the same for ps_sim3_hypotheses alone; and, as the yardstick, ps_pnp_ransac of the same library at the same shape (synthetic.pnp_scene,
its defaults) -- it scores four slots per sample with one projection per point, this call one model with two.  Median of `--reps` calls
after two warm-up calls.  Beside them align_maps as one call (draw + device) at the test shape, the draw alone, and PnPRANSAC's draw.
A host clock around a call that ends in a synchronising copy: a call time, not a kernel time."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from pyslam_amd import synthetic  # noqa: E402
from pyslam_amd.pipelines import pnp, sim3, similarity  # noqa: E402
from pyslam_amd.sensors import MonoCamera  # noqa: E402


def timed(fn, reps):
    fn()                                                 # two warm-up calls: code object, allocator
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, {'ms_median': float(np.median(t)), 'ms_min': float(np.min(t)), 'ms_max': float(np.max(t))}


def figures(num_pts, num_hyp, reps, restate):
    cam = MonoCamera(*synthetic.TWO_VIEW_CAMERA)
    p1, p2, o1, o2, scale, T, outlier = synthetic.sim3_scene(num_pts=num_pts)
    rs = sim3.Sim3RANSAC(cam)
    rs.ransac_iters = num_hyp
    rs.set_obs(p1, p2, o1, o2)
    np.random.seed(5)
    samples = rs.draw_samples()
    out = {'hypotheses': num_hyp, 'points': num_pts, 'reps': reps}
    res, out['sim3_ransac_pixel'] = timed(lambda: rs._device_ransac(samples), reps)
    rs.refit_iters = 0
    raw, out['sim3_ransac_pixel_no_refit'] = timed(lambda: rs._device_ransac(samples), reps)
    _, out['sim3_hypotheses_pixel'] = timed(lambda: rs._device_hypotheses(samples), reps)
    rm = sim3.Sim3RANSAC()
    rm.ransac_thresh = 0.25
    rm.set_obs(p1, p2)
    met, out['sim3_ransac_metric'] = timed(lambda: rm._device_ransac(samples), reps)
    # the yardstick: ps_pnp_ransac of the same library at the same shape
    pts, obs, _, _ = synthetic.pnp_scene(num_pts=num_pts)
    rp = pnp.PnPRANSAC(cam)
    rp.ransac_iters = num_hyp
    rp.set_obs(pts, obs)
    ref_pnp, out['pnp_ransac'] = timed(lambda: rp._device_ransac(samples), reps)
    out['sim3_over_pnp'] = out['sim3_ransac_pixel']['ms_median'] / out['pnp_ransac']['ms_median']
    out['no_slower_than_pnp'] = bool(out['sim3_over_pnp'] <= 1.0)
    out['inliers_raw'], out['inliers_final'], out['rounds'], out['ended_by'] = raw['count'], res['count'], res['rounds'], sim3.REASONS[res['reason']]
    out['inliers_metric'], out['true_inliers'], out['pnp_inliers'] = met['count'], int((~outlier).sum()), ref_pnp['count']
    out['scale'], out['true_scale'] = res['scale'], scale
    if restate:
        t0 = time.perf_counter()
        ref = similarity.ransac(p1, p2, o1, o2, cam.intrinsics(), samples, rs.ransac_thresh)
        out['host_restatement_ms'] = (time.perf_counter() - t0) * 1e3
        out['winner_equals_restatement'] = bool((res['best'], res['count'], res['rounds']) == (ref['best'], ref['count'], ref['rounds']))
        out['masks_equal_restatement'] = bool(np.array_equal(res['mask'], ref['mask']))
        out['S_max_abs_diff_to_restatement'] = float(np.abs(res['S_21'] - ref['S_21']).max())
    return out


def one_call(reps):
    """align_maps as one call at the test shape (192 pairs, 400 hypotheses), its draw alone, and PnPRANSAC's draw."""
    cam = MonoCamera(*synthetic.TWO_VIEW_CAMERA)
    p1, p2, o1, o2, _, _, _ = synthetic.sim3_scene()
    rs = sim3.Sim3RANSAC(cam)
    rs.set_obs(p1, p2, o1, o2)
    out = {'points': 192, 'hypotheses': 400, 'reps': reps}
    _, out['align_maps'] = timed(lambda: sim3.align_maps(cam, p1, p2, o1, o2, seed=5, ransac=rs), reps)
    _, out['sim3_draw_samples'] = timed(rs.draw_samples, reps)
    pts, obs, _, _ = synthetic.pnp_scene()
    rp = pnp.PnPRANSAC(cam)
    rp.set_obs(pts, obs)
    _, out['pnp_draw_samples'] = timed(rp.draw_samples, reps)
    _, out['register_frame'] = timed(lambda: pnp.register_frame(cam, pts, obs, seed=5, ransac=rp), reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'sim3_bench.json'))
    ap.add_argument('--reps', type=int, default=9)
    a = ap.parse_args()
    from pyslam_amd import _native as nat
    nat.require_gpu()                                    # no device: fail, do not time the host
    res = {'build_sha': nat.load().ps_build_sha().decode()}
    for name, (h, n) in {'400x2000': (400, 2000), '400x20000': (400, 20000)}.items():
        res[name] = figures(n, h, a.reps, restate=n <= 2000)
        print(json.dumps({name: res[name]}), flush=True)
    res['one_call_400x192'] = one_call(a.reps)
    print(json.dumps({'one_call_400x192': res['one_call_400x192']}), flush=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
