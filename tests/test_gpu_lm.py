"""GPU tests of Options.lm_adaptive: the adaptive Levenberg-Marquardt loop with step rejection on the device (ps_lm_iteration,
ps_solve_lm) against the numpy restatement of the same rule (tests/lm_restatement.py).

Bounds.  The project's solve-trace bounds (tests/test_gpu_parity.py: cost 1e-10 relative, parameters 1e-9) where the case holds
them; where a longer, damped trajectory does not, 10 x the deviation between the restatement solved with spsolve and the
restatement solved with gn_oracle.schur_solve on the same case -- two CPU solvers of the same equations, the noise floor of the
comparison, with one decade of margin.  Never a bound derived from the device's output.  A decision (accepted / rejected) is
compared only where the restatement's |rho| >= 0.05; the first iteration below that ends the comparison of the case (at most one
case may end early, none before its fifth iteration).  The measured deviations and the floors are written side by side into
profiles/lm_parity.json by tools/lm_parity.py, which runs the comparison of test_trace_parity."""
import copy

import numpy as np
import pytest

import lm_restatement as lmr
from oracle import gn_oracle as orc
from pyslam_amd import synthetic
from pyslam_amd.problem import Options, device_solve

pytestmark = pytest.mark.gpu

TOL_COST, TOL_PARAM = 1e-10, 1e-9       # tests/test_gpu_parity.py
PCG_TOL = 1e-14                         # the reduced solve is not the limit of the comparison


def _options(**kw):
    opt = Options()
    opt.lm_adaptive = True
    opt.pcg_tol = PCG_TOL
    opt.pcg_max_iters = 4000
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


def _device(lp):
    from pyslam_amd.device import DeviceProblem
    return DeviceProblem(lp)


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.abs(b))) if a.size else 0.


def trace_deviation(name, lp, kw, use_core_loop=True):
    """Device against the spsolve restatement over the compared iterations, beside the floor (spsolve against Schur
    restatement).  -> dict of measured deviations, floors and what must hold exactly."""
    fa, a = lmr.lm_solve(lp, kw, 'spsolve')
    fb, b = lmr.lm_solve(lp, kw, 'schur')
    ha, hb = a['lm_history'], b['lm_history']
    k = lmr.compared_iterations(ha)
    whole = k == len(ha)
    dev = _device(lp)
    hist, _ = device_solve(dev, _options(**kw), use_core_loop=use_core_loop)
    rows = dev.lm_history
    poses, points = dev.get_params()
    dev.close()
    ca, cb, cd = np.array(a['cost_history']), np.array(b['cost_history']), np.array(hist)
    out = dict(case=name, iterations_restatement=len(ha), iterations_device=len(rows), compared=k,
               decisions_restatement=ha[:k, 2].astype(int).tolist(), decisions_device=rows[:k, 2].astype(int).tolist(),
               floor_decisions_agree=bool(len(hb) >= k and np.array_equal(ha[:k, 2], hb[:k, 2])),
               cost_dev=_rel(cd[:k + 1], ca[:k + 1]), cost_floor=_rel(cb[:k + 1], ca[:k + 1]),
               lambda_dev=_rel(rows[:k, 0], ha[:k, 0]), lambda_floor=_rel(hb[:k, 0], ha[:k, 0]),
               model_decrease_dev=_rel(rows[:k, 3], ha[:k, 3]), model_decrease_floor=_rel(hb[:k, 3], ha[:k, 3]),
               whole_trace=whole)
    if whole:                            # the final parameters belong to the comparison only when no iteration was left out
        out.update(length_equal=len(hist) == len(ca),
                   poses_dev=float(np.abs(poses - fa.poses).max()), poses_floor=float(np.abs(fb.poses - fa.poses).max()),
                   points_dev=float(np.abs(points - fa.points).max()) if fa.points.size else 0.,
                   points_floor=float(np.abs(fb.points - fa.points).max()) if fa.points.size else 0.)
    return out


def check_trace(d):
    assert d['floor_decisions_agree'], d
    assert d['whole_trace'] or d['compared'] >= 5, d
    assert d['decisions_device'] == d['decisions_restatement'], d
    for key, tol in (('cost', TOL_COST), ('lambda', TOL_COST), ('model_decrease', TOL_COST)):
        assert d[key + '_dev'] <= max(tol, 10. * d[key + '_floor']), (key, d)
    if d['whole_trace']:
        assert d['length_equal'], d
        for key in ('poses', 'points'):
            assert d[key + '_dev'] <= max(TOL_PARAM, 10. * d[key + '_floor']), (key, d)


def test_trace_parity():
    """1. cost_history, the accepted column, lambda and the final parameters of every case against the restatement."""
    results = [trace_deviation(name, lp, kw) for name, (lp, kw) in lmr.parity_cases().items()]
    for d in results:
        print(d)
    assert sum(1 for d in results if not d['whole_trace']) <= 1
    assert any(0 in d['decisions_restatement'] for d in results)          # genuine rejections are among the cases
    for d in results:
        check_trace(d)


def test_converges_where_gauss_newton_fails():
    """2. The device's default loop leaves the 8 x 120 case above 1e6 (or raises); the adaptive loop ends at the optimum."""
    from pyslam_amd._native import NativeError
    lp, kw = lmr.parity_cases()['ba_8x120']
    gn = Options()
    gn.max_iters, gn.allow_nondecreasing_steps, gn.max_nondecreasing_steps = 30, True, 3
    dev = _device(lp)
    try:
        hist, _ = device_solve(dev, gn)
        gn_failed = not np.isfinite(hist[-1]) or hist[-1] > 1e6
    except NativeError:
        gn_failed = True
    dev.close()
    assert gn_failed
    dev = _device(lp)
    hist, _ = device_solve(dev, _options(**kw))
    rows = dev.lm_history
    dev.close()
    assert abs(hist[-1] - 525.0401898813542) <= 1e-6 * 525.04, hist
    assert all(b <= a for a, b in zip(hist[:-1], hist[1:]))
    assert rows.shape == (len(hist) - 1, 4)


def _long_tracks():
    lp = synthetic.stereo_ba(num_kf=40, num_lm=90, obs_per_lm=24, half_window=20, seed=3, pose_noise=0.05, point_noise=0.1)[0]
    assert np.bincount(lp.obs_point).max() > 16          # beyond the packed kernel: the 16-lane back-substitution
    return lp


@pytest.mark.parametrize('which', ['ba_small', 'long_tracks'])
@pytest.mark.parametrize('lam', [1e-3, 1., 1e3])
def test_model_decrease_of_one_iteration(which, lam):
    """3. The scalar of ps_lm_iteration against 0.5 h^T (lambda D h + g) of the restatement."""
    lp = lmr.parity_cases()['ba_small'][0] if which == 'ba_small' else _long_tracks()
    _, md_a = lmr.lm_step(lp, lam, 'spsolve')
    _, md_b = lmr.lm_step(lp, lam, 'schur')
    dev = _device(lp)
    dev.reset_solver_state()
    c0 = dev.eval_cost(True)
    cost, _, md, _, _ = dev.lm_iteration(lam, PCG_TOL, 4000, True)
    dev.close()
    floor = abs(md_b - md_a) / abs(md_a)
    print(which, lam, 'model_decrease', md, md_a, 'deviation', abs(md - md_a) / abs(md_a), 'floor', floor)
    assert abs(md - md_a) <= max(TOL_COST, 10. * floor) * abs(md_a)
    h, _ = lmr.lm_step(lp, lam, 'spsolve')
    want = orc.eval_cost(orc.apply_update(lp, h, False))
    assert abs(c0 - orc.eval_cost(lp)) <= TOL_COST * c0 and abs(cost - want) <= 1e-9 * abs(want)


def test_a_rejection_restores_the_parameters_exactly():
    """4. lambda0 = 1e-3 on the seed-1 case: the restatement rejects the first step with rho = -18.  The parameters after the
    rejected iteration are those before it, bit for bit, and so is the cost at the point the next iteration linearises at."""
    lp, kw = lmr.parity_cases()['ba_8x120_seed1']
    _, ref = lmr.lm_solve(lp, dict(kw, max_iters=0), 'spsolve')
    assert ref['lm_history'][0, 2] == 0. and ref['lm_history'][0, 1] <= -0.05
    for core in (True, False):
        dev = _device(lp)
        before = dev.get_params()
        c0 = dev.eval_cost(True)
        hist, _ = device_solve(dev, _options(**dict(kw, max_iters=0)), use_core_loop=core)
        after = dev.get_params()
        assert dev.lm_history.shape == (1, 4) and dev.lm_history[0, 2] == 0. and dev.lm_history[0, 1] <= -0.05
        assert hist == [c0, c0]
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert dev.eval_cost(True) == c0
        # the next iteration linearises at the restored point: its step under the raised damping equals a fresh handle's
        lam2 = 2e-3
        dev.reset_solver_state()
        got = dev.lm_iteration(lam2, PCG_TOL, 4000, True)
        dev.close()
        fresh = _device(lp)
        fresh.reset_solver_state()
        want = fresh.lm_iteration(lam2, PCG_TOL, 4000, True)
        fresh.close()
        assert got[0] == want[0] and got[2] == want[2]


def test_two_solves_are_bit_identical():
    """5. A fresh handle, another fresh handle and a reused one: the same cost_history and lm_history bits."""
    lp, kw = lmr.parity_cases()['ba_8x120_seed1']
    outs = []
    dev = None
    for k in range(3):
        if k < 2:
            dev = _device(lp)
        else:
            dev.set_params(lp.poses, lp.points)
        hist, _ = device_solve(dev, _options(**kw))
        outs.append((hist, dev.lm_history.copy(), dev.get_params()))
        if k == 0:
            dev.close()
    dev.close()
    for hist, rows, params in outs[1:]:
        assert hist == outs[0][0] and np.array_equal(rows, outs[0][1])
        assert np.array_equal(params[0], outs[0][2][0]) and np.array_equal(params[1], outs[0][2][1])


@pytest.mark.parametrize('name', ['ba_8x120', 'ba_8x120_seed1', 'pg_small_huber', 'pg_se2'])
def test_core_loop_equals_the_python_loop(name):
    """6. ps_solve_lm against the same statements in Python on ps_lm_iteration."""
    lp, kw = lmr.parity_cases()[name]
    outs = []
    for core in (True, False):
        dev = _device(lp)
        hist, stats = device_solve(dev, _options(**kw), use_core_loop=core)
        outs.append((hist, dev.lm_history.copy(), dev.get_params(), [a for a, _ in stats]))
        dev.close()
    (h_c, r_c, p_c, s_c), (h_p, r_p, p_p, s_p) = outs
    assert h_c == h_p and np.array_equal(r_c, r_p) and s_c == s_p
    assert np.array_equal(p_c[0], p_p[0]) and np.array_equal(p_c[1], p_p[1])


def test_hybrid_priors_equal_typed_priors():
    """7. Pose priors as user-defined blocks (Options.hybrid_blocks: the Python loop, the host blocks' cost in rho) against the
    same priors typed, at the bounds of tests/test_gpu_hybrid_blocks.py."""
    from test_host_api import build_namespace
    from pyslam_amd.lowering import pack_pose, pose_rows_to_matrices
    ns = build_namespace()
    lp, truth = synthetic.stereo_ba(num_kf=8, num_lm=120, obs_per_lm=4, half_window=3, seed=0, pose_noise=0.2, point_noise=0.4)
    opt = ns.Options()
    opt.lm_adaptive, opt.max_iters, opt.min_cost_decrease, opt.pcg_tol = True, 30, 0.999999, PCG_TOL
    problem = synthetic.to_objects(lp, ns, opt)
    first = len(problem.residual_blocks)
    rng = np.random.default_rng(1)
    for p in range(1, 8, 2):
        M = truth['poses'][p] if np.ndim(truth['poses'][p]) == 2 else pose_rows_to_matrices(truth['poses'][p:p + 1], 6)[0]
        T = ns.SE3.exp(0.01 * rng.standard_normal(6)).dot(ns.SE3(ns.SO3(M[:3, :3].copy()), M[:3, 3].copy()))
        problem.add_residual_block(ns.PoseResidual(T, np.identity(6) * 10.), [lp.pose_keys[p]], ns.HuberLoss(1.0))
    start = copy.deepcopy(problem.param_dict)
    problem.solve()
    assert problem._device.host is None
    typed = (np.array(problem._cost_history), problem.lm_history.copy(), copy.deepcopy(problem.param_dict))
    assert 'LM steps: {} accepted'.format(int(typed[1][:, 2].sum())) in problem.summary()
    problem.initialize_params(start)
    for k in range(first, len(problem.residual_blocks)):
        problem.residual_blocks[k] = synthetic.Untyped(problem.residual_blocks[k])
    problem.options.hybrid_blocks = True
    problem.solve()
    assert problem._device.host is not None
    hist, rows = np.array(problem._cost_history), problem.lm_history
    assert len(hist) == len(typed[0]) and np.array_equal(rows[:, 2], typed[1][:, 2])
    prev = np.concatenate([[typed[0][0]], typed[0][:-1]])
    assert np.all(np.abs(hist - typed[0]) <= 1e-10 * np.abs(typed[0]) + 1e-15 * prev), np.abs(hist - typed[0]) / typed[0]
    for key, val in typed[2].items():
        got = problem.param_dict[key]
        if hasattr(val, 'rot'):
            assert np.abs(pack_pose(got) - pack_pose(val)).max() < 1e-9, key
        else:
            assert np.abs(got - val).max() < 1e-9, key


def test_off_means_off():
    """8. lm_adaptive = False: the bits of a solve whose Options object does not have the new fields at all."""
    lp = synthetic.stereo_ba(num_kf=40, num_lm=1500, obs_per_lm=8, half_window=6, seed=9)[0]
    outs = []
    for strip in (False, True):
        opt = Options()
        opt.allow_nondecreasing_steps, opt.max_nondecreasing_steps, opt.pcg_tol = True, 3, 1e-12
        assert opt.lm_adaptive is False
        if strip:
            for k in ('lm_adaptive', 'lm_lambda_min', 'lm_lambda_max'):
                delattr(opt, k)
        dev = _device(lp)
        hist, stats = device_solve(dev, opt)
        outs.append((hist, stats, dev.get_params()))
        assert getattr(dev, 'lm_history', None) is None
        dev.close()
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1]
    assert np.array_equal(outs[0][2][0], outs[1][2][0]) and np.array_equal(outs[0][2][1], outs[1][2][1])


def test_a_one_pose_problem_takes_the_general_loop():
    """The one-launch motion-only kernel declines under lm_adaptive: lm_history exists and the cost does not rise."""
    from conftest import load_golden, golden_lp
    lp = golden_lp(load_golden('motion_only_cauchy'))
    dev = _device(lp)
    hist, _ = device_solve(dev, _options(max_iters=10))
    assert dev.lm_history.shape[0] == len(hist) - 1 and all(b <= a for a, b in zip(hist[:-1], hist[1:]))
    dev.close()
