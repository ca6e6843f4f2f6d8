#!/usr/bin/env python
"""Per-iteration cost of Options.hybrid_blocks on C3 (synthetic.stereo_ba defaults: 200 keyframes, 50 000 landmarks,
500 000 reprojection blocks) with 200 pose priors, three ways:

  typed    the priors as PoseResidual blocks: everything in the device tables
  hybrid   the same priors wrapped KIND-less (synthetic.Untyped), Options.hybrid_blocks = True: split into the host
           evaluation of the 200 blocks, the row upload (ps_set_host_rows) and the rest (device iteration + pose read-back +
           the host cost after the step)
  generic  the host-evaluated generic route (hybrid_blocks = False) on a problem small enough for it to finish

Each Problem.solve() runs from the same start (Options.static_blocks on C3: the 500 000 blocks are not walked again);
per-iteration times are the solve's wall clock over its iterations, the median of `--repeats` solves.  One JSON line on stdout; --out also writes it to a file.

    python tools/hybrid_bench.py [--repeats 3] [--out profiles/hybrid_bench.json]
"""
import argparse
import copy
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import numpy as np  # noqa: E402


def build(num_kf, num_lm, obs_per_lm, half_window, num_priors):
    from pyslam_amd import synthetic
    from test_host_api import build_namespace
    ns = build_namespace()
    lp, truth = synthetic.stereo_ba(num_kf=num_kf, num_lm=num_lm, obs_per_lm=obs_per_lm, half_window=half_window, seed=0)
    problem = synthetic.to_objects(lp, ns, ns.Options())
    rng = np.random.default_rng(1)
    first = len(problem.residual_blocks)
    for k in range(num_priors):
        p = 1 + k % (num_kf - 1)
        M = truth['poses'][p]
        T = ns.SE3.exp(0.01 * rng.standard_normal(6)).dot(ns.SE3(ns.SO3(M[:3, :3].copy()), M[:3, 3].copy()))
        problem.add_residual_block(ns.PoseResidual(T, 10. * np.identity(6)), [lp.pose_keys[p]], ns.HuberLoss(1.0))
    return problem, list(range(first, len(problem.residual_blocks)))


def timed_solves(problem, start, repeats):
    out = []
    for _ in range(repeats):
        problem.initialize_params(start)
        dev = problem._device
        if dev is not None and dev.host is not None:
            dev.host_seconds = [0., 0.]
        t0 = time.perf_counter()
        problem.solve()
        wall = time.perf_counter() - t0
        iters = len(problem._cost_history) - 1
        dev = problem._device
        host = list(dev.host_seconds) if dev is not None and dev.host is not None else [0., 0.]
        out.append((wall / iters, host[0] / iters, host[1] / iters, iters))
    return sorted(out)[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from pyslam_amd import synthetic
    res = {'config': 'C3 + 200 pose priors'}

    problem, prior_idx = build(200, 50000, 10, 20, 200)
    problem.options.static_blocks = True                   # per-iteration time of the solve, not of walking 500 000 blocks
    start = copy.deepcopy(problem.param_dict)
    problem.solve()                                        # warm-up: tables, code objects
    it_ms, _, _, iters = timed_solves(problem, start, a.repeats)
    res['typed'] = {'ms_per_iter': 1e3 * it_ms, 'iterations': iters}

    for k in prior_idx:
        problem.residual_blocks[k] = synthetic.Untyped(problem.residual_blocks[k])
    problem.options.hybrid_blocks = True
    problem.options.static_blocks = False                  # (the blocks did change: lower them once more)
    problem.initialize_params(start)
    problem.solve()
    problem.options.static_blocks = True
    it_ms, ev, up, iters = timed_solves(problem, start, a.repeats)
    res['hybrid'] = {'ms_per_iter': 1e3 * it_ms, 'host_eval_ms_per_iter': 1e3 * ev, 'row_upload_ms_per_iter': 1e3 * up,
                     'device_and_rest_ms_per_iter': 1e3 * (it_ms - ev - up), 'iterations': iters,
                     'host_eval_us_per_block': 1e6 * ev / len(prior_idx)}

    small, prior_idx = build(20, 500, 5, 3, 200)
    for k in prior_idx:
        small.residual_blocks[k] = synthetic.Untyped(small.residual_blocks[k])
    start = copy.deepcopy(small.param_dict)
    it_ms, _, _, iters = timed_solves(small, start, a.repeats)
    assert small._device is None                          # the generic route
    n = sum(len(small._update_partition_dict[k]) for k in small._update_partition_dict)
    res['generic'] = {'ms_per_iter': 1e3 * it_ms, 'iterations': iters, 'config': '20 keyframes, 500 landmarks, 2 500 reprojection '
                      'blocks + 200 priors', 'unknowns': n}
    small.options.hybrid_blocks = True
    small.initialize_params(start)
    small.solve()
    it_ms, ev, up, iters = timed_solves(small, start, a.repeats)
    res['hybrid_small'] = {'ms_per_iter': 1e3 * it_ms, 'host_eval_ms_per_iter': 1e3 * ev, 'iterations': iters}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
