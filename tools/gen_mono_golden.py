#!/usr/bin/env python
"""Generate tests/golden/mono_ba.npz by running the VERBATIM reference Problem / ReprojectionResidual / losses with this
project's MonoCamera.

TEST INFRASTRUCTURE -- authoring machine only, like tools/gen_sparse_golden.py, whose path set-up (oracle/gen_golden.py: the
reference first on sys.path) it shares.  Run from the repository root:

    python tools/gen_mono_golden.py

The reference's ReprojectionResidual is written for any camera whose ``project(pt_c, compute_jacobians)`` returns the
prediction and its Jacobian (pyslam/residuals/reprojection_residual.py); pyslam_amd.sensors.MonoCamera returns (u, v) and a
2 x 3 Jacobian, the blocks carry 2-vector observations and a 2 x 2 stiffness.  Nothing of the reference is copied: it is
imported at run time, and only arrays are recorded.

Scene: synthetic.mono_ba(6 keyframes, 60 landmarks, 4 observations each), perturbed, the first two poses constant.
  (a) ``l2_*`` / ``huber_*``: the input tables, the reference's cost history, per-iteration steps, final poses and points,
      and compute_covariance blocks of two poses, two landmarks and one pose-landmark pair;
  (b) ``mixed_*``: 40 % of the observations stay stereo (both kinds of camera on the same landmarks): costs and steps;
  (c) ``tri_*``: every pose of the L2 scene held constant at its TRUE value (``tri_poses``), minimum parallax
      ``tri_min_parallax_deg``; ``tri_linear``: the linear-start points (the numpy restatement
      pyslam_amd/triangulation.py with refine_iters = 0 -- the reference has no triangulation from several views; every
      landmark must have status 0), ``tri_refined``: the points after a reference solve started from them with
      min_cost_decrease = 1 (it stops only when a step no longer lowers the cost) and min_update_norm = 1e-10.
"""
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as gg  # noqa: E402  (puts the reference first on sys.path)

import numpy as np  # noqa: E402

from pyslam_amd import synthetic, triangulation  # noqa: E402
from pyslam_amd import losses as own_losses  # noqa: E402
from pyslam_amd.sensors import MonoCamera  # noqa: E402
from pyslam_amd.lowering import pack_pose_matrices  # noqa: E402

NUM_KF, NUM_LM, OBS_PER_LM, HALF_WINDOW, SEED = 6, 60, 4, 3, 11
HUBER_K = 1.5
COV_POSES, COV_POINTS = (2, 4), (3, 41)
TRI_MIN_PARALLAX_DEG = 0.1

NS = types.SimpleNamespace(**vars(gg.NS))
NS.MonoCamera = MonoCamera


def scene(loss=None, stereo_fraction=0., with_truth=False):
    lp, truth = synthetic.mono_ba(NUM_KF, NUM_LM, obs_per_lm=OBS_PER_LM, half_window=HALF_WINDOW, seed=SEED, loss=loss,
                              stereo_fraction=stereo_fraction)
    assert np.bincount(lp.obs_point, minlength=NUM_LM).min() >= 3
    return (lp, truth) if with_truth else lp


def solve(prefix, lp, covariance):
    opt = gg.ref_problem.Options()
    problem = synthetic.to_objects(lp, NS, opt)
    final, out = gg.run_reference(problem)
    rec = {prefix + '_' + k: v for k, v in gg.lp_arrays(lp).items()}
    for k in ('cost_history', 'iter_cost', 'iter_dx', 'lin_cost'):
        rec[prefix + '_' + k] = out[k]
    for k, v in gg.options_dict(opt).items():
        rec[prefix + '_opt_' + k] = np.array(v)
    if covariance:
        for k, v in gg.final_tables(final, lp).items():
            rec[prefix + '_' + k] = v
        problem.compute_covariance()
        pk, lk = [lp.pose_keys[i] for i in COV_POSES], [lp.point_keys[j] for j in COV_POINTS]
        for name, (a, b) in {'cov_pose0': (pk[0], pk[0]), 'cov_pose1': (pk[1], pk[1]), 'cov_point0': (lk[0], lk[0]),
                             'cov_point1': (lk[1], lk[1]), 'cov_pose0_point0': (pk[0], lk[0])}.items():
            rec[prefix + '_' + name] = np.array(problem.get_covariance_block(a, b))
    print('{:6s} iterations {:2d}  cost {:.6e} -> {:.6e}'.format(prefix, len(out['cost_history']), out['cost_history'][0],
                                                               out['cost_history'][-1]))
    return rec


def triangulation_case(lp, truth):
    # the scene's keyframes are 5 cm apart and its landmarks 6 to 30 m away: the largest angle between two of a landmark's four
    # rays goes down to a few tenths of a degree, and under the 1 % pose perturbation some results fall behind a camera.
    # Triangulation is therefore recorded at the TRUE poses with a minimum parallax of 0.1 degrees; every landmark must be ok
    lp = lp.copy()
    lp.poses = pack_pose_matrices(truth['poses'])
    lin, status = triangulation.triangulate(lp, None, refine_iters=0, min_parallax_deg=TRI_MIN_PARALLAX_DEG)
    assert not status.any(), status
    assert not triangulation.triangulate(lp, None, refine_iters=20, min_parallax_deg=TRI_MIN_PARALLAX_DEG)[1].any()
    fixed = lp.copy()
    fixed.points = lin.copy()
    fixed.pose_rid = np.full(lp.num_poses, -1, dtype=np.int32)
    fixed.finalize()
    opt = gg.ref_problem.Options()
    opt.min_cost_decrease, opt.min_update_norm, opt.max_iters = 1.0, 1e-10, 50
    problem = synthetic.to_objects(fixed, NS, opt)
    final = problem.solve()
    refined = np.stack([final[k] for k in lp.point_keys])
    print('tri    iterations {:2d}  cost {:.6e} -> {:.6e}'.format(len(problem._cost_history), problem._cost_history[0],
                                                               problem._cost_history[-1]))
    return {'tri_poses': lp.poses, 'tri_min_parallax_deg': np.array(TRI_MIN_PARALLAX_DEG), 'tri_linear': lin, 'tri_refined': refined, 'tri_cost_history': np.array(problem._cost_history)}


def main():
    rec = {'cov_poses': np.array(COV_POSES), 'cov_points': np.array(COV_POINTS)}
    rec.update(solve('l2', scene(), True))
    rec.update(solve('huber', scene(own_losses.HuberLoss(HUBER_K)), True))
    rec.update(solve('mixed', scene(stereo_fraction=0.4), False))
    rec.update(triangulation_case(*scene(with_truth=True)))
    path = os.path.join(REPO, 'tests', 'golden', 'mono_ba.npz')
    np.savez_compressed(path, **rec)
    print('{}: {:.1f} KB'.format(path, os.path.getsize(path) / 1024.))


if __name__ == '__main__':
    main()
