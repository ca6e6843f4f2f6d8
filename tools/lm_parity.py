#!/usr/bin/env python
"""Trace parity of Options.lm_adaptive as numbers: for every case of tests/lm_restatement.py: parity_cases, the device's
deviation from the numpy restatement (cost history, lambda, model decrease, final parameters; the decisions must be equal) next
to the floor of the comparison -- the restatement solved with spsolve against the restatement solved by Schur elimination.
tests/test_gpu_lm.py asserts max(project bound, 10 x floor); this writes what was measured.

    python tools/lm_parity.py [--out profiles/lm_parity.json]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import lm_restatement as lmr
    import test_gpu_lm as t
    res = {'bounds': {'cost_lambda_model_decrease_relative': t.TOL_COST, 'parameters_absolute': t.TOL_PARAM,
                      'rule': 'max(bound, 10 x floor); decisions equal where the restatement has |rho| >= 0.05'},
           'cases': [t.trace_deviation(name, lp, kw) for name, (lp, kw) in lmr.parity_cases().items()],
           'model_decrease_one_iteration': []}
    from pyslam_amd.device import DeviceProblem
    for which, lp in (('ba_small', lmr.parity_cases()['ba_small'][0]), ('long_tracks', t._long_tracks())):
        for lam in (1e-3, 1., 1e3):
            md_a, md_b = lmr.lm_step(lp, lam, 'spsolve')[1], lmr.lm_step(lp, lam, 'schur')[1]
            dev = DeviceProblem(lp)
            md = dev.lm_iteration(lam, t.PCG_TOL, 4000, True)[2]
            dev.close()
            res['model_decrease_one_iteration'].append({'case': which, 'lambda': lam, 'restatement': md_a, 'device': md,
                                                        'dev': abs(md - md_a) / abs(md_a), 'floor': abs(md_b - md_a) / abs(md_a)})
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
