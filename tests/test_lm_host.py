"""CPU tests of the adaptive Levenberg-Marquardt feature (Options.lm_adaptive): the claim it rests on, restated in numpy
(tests/lm_restatement.py); the options and the routes that decline; the C ABI of the two new exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lm_restatement as lmr
from oracle import gn_oracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_restatement_converges_where_the_reference_loop_diverges():
    lp, kw = lmr.parity_cases()['ba_8x120']
    _, gn = orc.solve(lp, dict(max_iters=30, allow_nondecreasing_steps=True, max_nondecreasing_steps=3))
    assert gn['cost_history'][-1] > 1e6
    for solver in ('spsolve', 'schur'):
        _, lm = lmr.lm_solve(lp, kw, solver)
        hist = lm['cost_history']
        assert abs(hist[-1] - 525.04) <= 1e-6 * 525.04 + 5e-3, hist      # (525.04 as the issue states it: two decimals)
        assert abs(hist[-1] - 525.0401898813542) <= 1e-6 * 525.04
        assert all(b <= a for a, b in zip(hist[:-1], hist[1:]))
        assert lm['lm_history'][:, 2].all() and len(hist) == 9            # eight accepted steps


def test_the_two_restatements_agree_on_every_compared_decision():
    """What tests/test_gpu_lm.py relies on: inside the compared range of every parity case the spsolve and the Schur restatement
    take the same decisions; at most one case ends early (|rho| < 0.05), none before its fifth iteration; the seed-1 case holds
    genuine rejections, the first with rho <= -0.05 (the forced rejection of the GPU test)."""
    early = 0
    for name, (lp, kw) in lmr.parity_cases().items():
        a = lmr.lm_solve(lp, kw, 'spsolve')[1]['lm_history']
        b = lmr.lm_solve(lp, kw, 'schur')[1]['lm_history']
        k = lmr.compared_iterations(a)
        assert len(b) >= k and np.array_equal(a[:k, 2], b[:k, 2]), name
        if k < len(a):
            early += 1
            assert k >= 5, name
        if name == 'ba_8x120_seed1':
            assert a[0, 2] == 0. and a[0, 1] <= -0.05 and (a[:k, 2] == 0.).sum() >= 3 and (a[:k, 2] == 1.).sum() >= 3
    assert early <= 1


def test_the_damping_rule():
    assert lmr.lm_update(1., 2., 1., 1e-12, 1e12) == (True, 1. / 3., 2.)
    assert lmr.lm_update(1., 2., 0.5, 1e-12, 1e12) == (True, 1., 2.)
    assert lmr.lm_update(1., 4., -1., 1e-12, 1e12) == (False, 4., 8.)
    assert lmr.lm_update(1e11, 16., 0., 1e-12, 1e12) == (False, 1e12, 32.)
    assert lmr.lm_update(2e-12, 2., 1., 1e-12, 1e12)[1] == 1e-12


def test_options_defaults_and_the_shim():
    from pyslam_amd.problem import Options, lm_options
    import pyslam.problem as shim
    opt = Options()
    assert opt.lm_adaptive is False and opt.lm_lambda_min == 1e-12 and opt.lm_lambda_max == 1e12 and opt.lm_lambda == 0.
    assert shim.Options is Options
    assert lm_options(opt) == (1e-3, 1e-12, 1e12)
    opt.lm_lambda = 5.
    assert lm_options(opt)[0] == 5.
    opt.lm_lambda_max = 1.
    assert lm_options(opt)[0] == 1.
    opt.lm_lambda_min = 2.
    with pytest.raises(ValueError, match='lm_lambda_min'):
        lm_options(opt)


def _ba_problem(**options):
    from test_host_api import build_namespace
    from pyslam_amd import synthetic
    ns = build_namespace()
    lp = synthetic.stereo_ba(num_kf=4, num_lm=12, obs_per_lm=3, half_window=2, seed=0)[0]
    opt = ns.Options()
    for k, v in options.items():
        setattr(opt, k, v)
    return synthetic.to_objects(lp, ns, opt), lp, ns


def test_the_declined_routes_raise_before_a_device_is_needed():
    from pyslam_amd import synthetic
    problem, lp, ns = _ba_problem(lm_adaptive=True, devices='all')
    with pytest.raises(ValueError, match='lm_adaptive.*sharded'):
        problem.solve()
    problem, lp, ns = _ba_problem(lm_adaptive=True, linesearch_max_iters=0)
    with pytest.raises(ValueError, match='linesearch_max_iters'):
        problem.solve()
    # a block without a typed kernel and hybrid_blocks off: the generic host path
    problem, lp, ns = _ba_problem(lm_adaptive=True)
    problem.residual_blocks[0] = synthetic.Untyped(problem.residual_blocks[0])
    with pytest.raises(ValueError, match='lm_adaptive.*generic'):
        problem.solve()
    # a device without ps_lm_iteration (the sharded view, the photometric device) never gets the fixed-lambda loop in silence
    from pyslam_amd.problem import Options, device_solve

    class NoLm:
        def gn_iteration(self, *a):
            raise AssertionError('the fixed-lambda loop ran')
    opt = Options()
    opt.lm_adaptive = True
    with pytest.raises(ValueError, match='lm_adaptive.*NoLm'):
        device_solve(NoLm(), opt)


def test_summary_without_lm_is_unchanged():
    problem, _, _ = _ba_problem()
    problem._cost_history = [2., 1.]
    assert problem.summary() == 'Iterations: {:3} | Cost: {:12e} --> {:12e}'.format(2, 2., 1.)
    problem.lm_history = np.array([[1e-3, 0.9, 1., 1.], [3e-4, -1., 0., 1.], [6e-4, 0.5, 1., 1.]])
    assert problem.summary().endswith('\nLM steps: 2 accepted, 1 rejected')
    assert problem.summary('full').endswith('LM steps: 2 accepted, 1 rejected\n')


def test_the_c_abi_of_the_new_exports():
    from pyslam_amd import _native as nat
    assert C.sizeof(nat.LmOptions) == 72                      # include/pyslam_hip.h: sizeof(ps_lm_options) == 72
    assert C.sizeof(nat.LmOptions) == C.sizeof(nat.SolveOptions) + 24
    assert [f[0] for f in nat.LmOptions._fields_[:8]] == [f[0] for f in nat.SolveOptions._fields_]
    header = open(os.path.join(REPO, 'include', 'pyslam_hip.h')).read()
    assert 'sizeof(ps_lm_options) == 72' in header
    body = re.search(r'typedef struct ps_lm_options \{(.*?)\} ps_lm_options;', header, re.S).group(1)
    names = re.findall(r'(\w+)\s*[,;]', body)
    assert names == [f[0] for f in nat.LmOptions._fields_]
    for name in ('ps_lm_iteration', 'ps_solve_lm'):
        decl = re.search(r'\bint ' + name + r'\((.*?)\);', header, re.S).group(1)
        assert name in nat.SIGNATURES and len(decl.split(',')) == len(nat.SIGNATURES[name][1]), name
    # model_decrease travels beside the cost and ||dx||: an output of ps_lm_iteration, a row entry of ps_solve_lm
    assert 'double* model_decrease_out' in header and 'double* lm_rows' in header
