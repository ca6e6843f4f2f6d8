#!/usr/bin/env python
"""Every output of the three RANSAC front ends on the committed test scenes, bit for bit, in one .npz -- and the comparison of
two such files.  The GPU tests hold the device against the numpy restatements with tolerances and margins; they cannot see a
change of the last bit.  This can: dump on the build before a change and on the build after it, then compare.

    python tools/ransac_dump.py --out before.npz                    (on an MI355X, one process per build)
    python tools/ransac_dump.py --compare before.npz after.npz [--json profiles/NAME.json]

Scenes (tests/ransac_scenes.py, tests/pnp_scenes.py):
  frame-to-frame  F2F_SWEEP, the non-finite scene, the conditioning ladder:  T_all, counts, masks (ps_ransac_cost on T_all), winner
  two-view        TV_SWEEP, tv_nonfinite_scene, with the refit and without:  E_all, counts, flags, masks (ps_twoview_score),
                  T_21, E, mask, info, parallax
  PnP             SHAPES, the seeded table, minimal_four, with the refinement and without:  T_all, counts, flags, masks
                  (ps_pnp_score), T_cw, mask, info, squared errors, cost history
`build_sha` is ps_build_sha() of the library that ran.  --compare exits 1 when any array differs (np.array_equal with
equal_nan=True: a NaN equals a NaN in the same place)."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))


def dump_f2f(out):
    import ransac_scenes as rs
    from pyslam_amd.pipelines.ransac import compute_transform_fast
    from test_gpu_ransac_edges import f2f_solver
    cases = [('f2f/n{}_h{}_s{}_{}'.format(n, h, seed, sseed), rs.f2f_scene(n, seed), rs.f2f_samples(n, h, 3, sseed))
             for n, h, seed, sseed in rs.F2F_SWEEP]
    sc, where = rs.f2f_nonfinite_scene()
    cases.append(('f2f/nonfinite', sc, rs.f2f_nonfinite_samples(where)[0]))
    for name, sc, idx in cases:
        r = f2f_solver(sc)
        T_best, mask, best, count, T_all, counts = r._device_ransac(idx, want_all=True)
        out[name + '/T_all'], out[name + '/counts'] = T_all, counts
        out[name + '/masks'] = r.compute_ransac_cost(T_all, sc['pts_1'], sc['obs_2'], sc['cam'], rs.THRESH)
        out[name + '/winner'], out[name + '/T_best'], out[name + '/mask'] = np.array([best, count]), T_best, mask
    for n in (3, 6):
        sets = [rs.ladder_set(n, rung) for rung in rs.LADDER_RUNGS]
        out['f2f/ladder_n{}/T'.format(n)] = compute_transform_fast(np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets]))


def dump_twoview(out):
    import ransac_scenes as rs
    from test_gpu_twoview import solver
    cases = [('tv/n{}_h{}_s{}_{}'.format(n, h, seed, sseed),) + rs.tv_scene(n, seed) + (rs.tv_samples(n, h, sseed),)
             for n, h, seed, sseed in rs.TV_SWEEP]
    obs_1, obs_2, planted = rs.tv_nonfinite_scene()
    cases.append(('tv/nonfinite', obs_1, obs_2, rs.tv_nonfinite_samples(planted)[0]))
    for name, obs_1, obs_2, idx in cases:
        s = solver(obs_1, obs_2)
        E, counts, flags = s._device_hypotheses(idx)
        out[name + '/E_all'], out[name + '/counts'], out[name + '/flags'] = E, counts, flags
        out[name + '/masks'] = s.compute_ransac_cost(E, obs_1, obs_2, s.camera, s.ransac_thresh)
        for refit in (True, False):
            res = solver(obs_1, obs_2, refit=refit)._device_ransac(idx)
            pre = '{}/refit{}/'.format(name, int(refit))
            for key in ('T_21', 'E', 'mask', 'cheirality_counts', 'parallax_deg'):
                out[pre + key] = res[key]
            out[pre + 'info'] = np.array([res['best'], res['raw_count'], res['count'], int(res['refit_kept'])])


def dump_pnp(out):
    import pnp_scenes as sc
    from test_gpu_pnp import solver
    cases = [('pnp/n{}_h{}'.format(n, h),) + sc.scene(n)[:2] + (sc.samples_of(n, h),) for n, h in sc.SHAPES]
    cases.append(('pnp/seeded',) + sc.scene(192)[:2] + (sc.ransac_samples(),))
    pts, obs, _, samples = sc.minimal_four()
    cases += [('pnp/minimal3', pts[:3], obs[:3], samples), ('pnp/minimal4', pts, obs, samples)]
    for name, pts, obs, idx in cases:
        s = solver(pts, obs)
        T, counts, empty, degenerate = s._device_hypotheses(idx)
        out[name + '/T_all'], out[name + '/counts'], out[name + '/empty'], out[name + '/degenerate'] = T, counts, empty, degenerate
        out[name + '/masks'] = s.compute_ransac_cost(T.reshape(-1, 4, 4), pts, obs, s.camera, s.ransac_thresh)
        for refine in (True, False):
            res = solver(pts, obs, refine=refine)._device_ransac(idx)
            pre = '{}/refine{}/'.format(name, int(refine))
            for key in ('T_cw', 'mask', 'd', 'cost_history'):
                out[pre + key] = res[key]
            out[pre + 'info'] = np.array([res['best'], res['best_slot'], res['raw_count'], res['count'], int(res['refine_kept']),
                                          int(res['pivot_failed']), res['iterations']])


def compare(a_path, b_path, json_path):
    a, b = np.load(a_path), np.load(b_path)
    keys = sorted((set(a.files) | set(b.files)) - {'build_sha'})
    arrays = {}
    for k in keys:
        if k not in a.files or k not in b.files:
            arrays[k] = {'shape': None, 'equal': False}
            continue
        same = a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and bool(np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == 'f'))
        arrays[k] = {'shape': list(a[k].shape), 'equal': same}
    differing = [k for k in keys if not arrays[k]['equal']]
    res = {'build_sha_a': str(a['build_sha']), 'build_sha_b': str(b['build_sha']), 'arrays': len(keys), 'differing': differing,
           'all_equal': not differing, 'per_array': arrays}
    print(json.dumps({k: res[k] for k in ('build_sha_a', 'build_sha_b', 'arrays', 'differing', 'all_equal')}))
    if json_path:
        with open(json_path, 'w') as fh:
            json.dump(res, fh, indent=1)
            fh.write('\n')
    return 0 if not differing else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--compare', nargs=2, metavar=('A', 'B'))
    ap.add_argument('--json')
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare[0], a.compare[1], a.json))
    if not a.out:
        ap.error('--out or --compare')
    from pyslam_amd import _native as nat
    nat.require_gpu()
    out = {'build_sha': np.array(nat.load().ps_build_sha().decode())}
    with np.errstate(all='ignore'):
        dump_f2f(out)
        dump_twoview(out)
        dump_pnp(out)
    np.savez(a.out, **out)
    print('{} arrays from build {} -> {}'.format(len(out) - 1, out['build_sha'], a.out))


if __name__ == '__main__':
    main()
