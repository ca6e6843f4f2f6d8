#!/usr/bin/env python
"""Cost of Options.lm_adaptive per iteration at C3 (synthetic.stereo_ba defaults: 200 keyframes, 50 000 landmarks,
500 000 reprojection blocks), on one build:

  lm_adaptive   the adaptive loop (ps_solve_lm) from lambda0 = --lam; a run with a rejected step is reported, not hidden
  fixed_lambda  ps_solve at the same constant lambda (Options.lm_lambda): the same damped linearisation without the model
                decrease, the snapshots, and WITH the tail's look-ahead
  default       ps_solve under the default options of the route bench.py measures (lambda = 0)

Cold solves as bench.py does them: ps_reset_solver_state and the upload of the start parameters before every solve, neither
timed; the solve's wall clock, fenced by a stream synchronisation, over its iterations.  --warmup solves first, then the
median of --repeats (>= 7).  --parent-line FILE: a bench.py JSON line of the parent commit measured in the same session, copied
into the output beside the figures.  One JSON line on stdout; --out also writes it to a file.

    python tools/lm_bench.py [--repeats 9] [--warmup 2] [--lam 1e-3] [--out profiles/lm_bench.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402


def timed(dev, start, opt, warmup, repeats):
    import torch
    from pyslam_amd.problem import device_solve
    per_iter, hist, rows = [], None, None
    dev.lm_history = None
    for k in range(warmup + repeats):
        dev.reset_solver_state()
        dev.set_params(*start)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hist, stats = device_solve(dev, opt)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if k >= warmup:
            per_iter.append(dt * 1e3 / max(len(stats), 1))
        rows = getattr(dev, 'lm_history', None)
    out = {'ms_per_iteration_median': round(float(np.median(per_iter)), 4), 'ms_per_iteration_min': round(float(np.min(per_iter)), 4),
           'ms_per_iteration_max': round(float(np.max(per_iter)), 4), 'repeats': repeats, 'iterations': len(hist) - 1,
           'cost_first': hist[0], 'cost_last': hist[-1], 'pcg_iters': [int(s[0]) for s in stats]}
    if rows is not None:
        out['rejected_steps'] = int(np.sum(rows[:, 2] == 0.))
        out['lambda'] = [float(x) for x in rows[:, 0]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--lam', type=float, default=1e-3)
    ap.add_argument('--max-iters', type=int, default=4)
    ap.add_argument('--parent-line', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error('--repeats must be at least 7')
    import __graft_entry__ as ge
    ge.build()
    import torch  # noqa: F401  (the fences)
    from pyslam_amd import synthetic, _native as nat
    from pyslam_amd.device import DeviceProblem
    from pyslam_amd.problem import Options
    lp, _ = synthetic.stereo_ba()
    start = (lp.poses.copy(), lp.points.copy())
    dev = DeviceProblem(lp)

    def options(**kw):
        opt = Options()
        opt.max_iters = a.max_iters
        opt.allow_nondecreasing_steps, opt.max_nondecreasing_steps = True, a.max_iters + 2      # (runs all its iterations)
        opt.min_update_norm, opt.min_cost_decrease = 0., 1.                                  # (the adaptive loop too)
        for k, v in kw.items():
            setattr(opt, k, v)
        return opt
    res = {'config': 'C3', 'build_sha': nat.load().ps_build_sha().decode(), 'lambda0': a.lam, 'max_iters': a.max_iters,
           'lm_adaptive': timed(dev, start, options(lm_adaptive=True, lm_lambda=a.lam), a.warmup, a.repeats),
           'fixed_lambda': timed(dev, start, options(lm_lambda=a.lam), a.warmup, a.repeats),
           'default': timed(dev, start, options(), a.warmup, a.repeats)}
    dev.close()
    res['lm_over_fixed'] = round(res['lm_adaptive']['ms_per_iteration_median'] / res['fixed_lambda']['ms_per_iteration_median'], 4)
    if a.parent_line and os.path.exists(a.parent_line):
        for line in open(a.parent_line):
            line = line.strip()
            if line.startswith('{'):
                p = json.loads(line)
                res['parent_bench_line'] = {k: p[k] for k in ('value', 'unit', 'metric', 'build_sha', 'ms_median_of_solves') if k in p}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
