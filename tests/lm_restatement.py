"""Numpy restatement of the adaptive Levenberg-Marquardt loop (Nielsen 1999; Madsen, Nielsen, Tingleff, "Methods for
non-linear least squares problems", algorithm 3.16) on the oracle's pieces: gn_oracle.linearize / apply_update / eval_cost,
the damped system solved by scipy's spsolve or by gn_oracle.schur_solve (a problem without landmarks, for which schur_solve
is the same spsolve call: by a dense solve with iterative refinement).  The reference of tests/test_lm_host.py and
tests/test_gpu_lm.py -- the project this one is modelled on has no LM, so there is nothing else to compare with.

    H = J~^T J~,  g = -J~^T e~,  D = diag(H),  (H + lambda D) h = g
    model_decrease = 0.5 h^T (lambda D h + g)
    rho = (cost(x) - cost(x [+] h)) / model_decrease
    rho > 0: accept, lambda *= max(1/3, 1 - (2 rho - 1)^3), nu = 2;   else: reject, lambda *= nu, nu *= 2

The stopping rules are those of Options.lm_adaptive (pyslam_amd/problem.py: _lm_loop), statement for statement."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import gn_oracle as orc

DEFAULTS = dict(max_iters=100, min_update_norm=1e-6, min_cost=1e-12, min_cost_decrease=0.9,
                lm_lambda=0., lm_lambda_min=1e-12, lm_lambda_max=1e12)


def lm_step(lp, lam, linear_solver='spsolve', points_first=False):
    """One damped step at `lp`: -> (h, model_decrease)."""
    J, e, _ = orc.linearize(lp, points_first)
    JT = J.T.tocsr()
    H = JT.dot(J).tocsr()
    g = -JT.dot(e)
    D = H.diagonal()
    A = (H + lam * sp.diags(D)).tocsr()
    if linear_solver == 'spsolve':
        h = np.atleast_1d(spla.spsolve(A.tocsc(), g))
    elif lp.num_var_points == 0:
        h = refined_dense_solve(A.toarray(), g)     # (no landmarks: schur_solve would be the same spsolve call, no second solver)
    else:
        h = np.atleast_1d(orc.schur_solve(lp, A, g, points_first))
    return h, 0.5 * float(h.dot(lam * D * h + g))


def refined_dense_solve(A, b):
    """Jacobi-scaled dense solve with three steps of iterative refinement on long-double residuals (the arbiter of
    tests/test_gpu_parity.py: accurate_solve): the second CPU solver of a problem without landmarks, whose normal matrix --
    priors of stiffness 1e6 beside loop closures of 1 -- is too ill-conditioned for one LU to define the answer."""
    d = 1. / np.sqrt(np.diag(A))
    As, bs = A * d[:, None] * d[None, :], b * d
    x = np.linalg.solve(As, bs)
    for _ in range(3):
        res = bs.astype(np.longdouble) - As.astype(np.longdouble) @ x.astype(np.longdouble)
        x = x + np.linalg.solve(As, res.astype(float))
    return x * d


def lm_update(lam, nu, rho, lam_min, lam_max):
    """The damping rule: -> (accepted, lambda, nu), lambda clamped."""
    if rho > 0.:
        lam, nu = lam * max(1. / 3., 1. - (2. * rho - 1.) ** 3), 2.
        return True, min(max(lam, lam_min), lam_max), nu
    lam, nu = lam * nu, 2. * nu
    return False, min(max(lam, lam_min), lam_max), nu


def lm_solve(lp, options=None, linear_solver='spsolve', points_first=False):
    """-> (final LoweredProblem, dict(cost_history, lm_history (n, 4): lambda used, rho, accepted, model_decrease))."""
    opt = dict(DEFAULTS)
    opt.update(options or {})
    lam = opt['lm_lambda'] if opt['lm_lambda'] > 0. else 1e-3
    lam = min(max(lam, opt['lm_lambda_min']), opt['lm_lambda_max'])
    nu = 2.
    cur = lp.copy()
    cost = orc.eval_cost(cur)
    history, rows = [cost], []
    it, done = 0, False
    while not done:
        it += 1
        prev = cost
        h, md = lm_step(cur, lam, linear_solver, points_first)
        trial = orc.apply_update(cur, h, points_first)
        new_cost = orc.eval_cost(trial)
        ok = np.isfinite(md) and md > 0. and np.isfinite(new_cost)
        rho = (prev - new_cost) / md if ok else -1.
        used = lam
        raw = lam * nu                          # what a rejection asks for, before the clamp
        accepted, lam, nu = lm_update(lam, nu, rho, opt['lm_lambda_min'], opt['lm_lambda_max'])
        rows.append((used, rho, 1. if accepted else 0., md))
        if accepted:
            cur, cost = trial, new_cost
        history.append(cost)
        done = it > opt['max_iters'] or float(np.linalg.norm(h)) < opt['min_update_norm'] or cost < opt['min_cost']
        if accepted:
            done = done or cost >= opt['min_cost_decrease'] * prev
        else:
            done = done or raw > opt['lm_lambda_max']
    return cur, dict(cost_history=history, lm_history=np.array(rows, float).reshape(-1, 4))


def compared_iterations(lm_history, rho_floor=0.05):
    """Number of leading iterations whose decision is compared: the first with |rho| < rho_floor ends the comparison."""
    small = np.nonzero(np.abs(lm_history[:, 1]) < rho_floor)[0]
    return int(small[0]) if small.size else len(lm_history)


def parity_cases():
    """name -> (LoweredProblem, options) of the trace-parity cases of tests/test_gpu_lm.py (checked on the CPU by
    tests/test_lm_host.py: the spsolve and the Schur restatement agree on every decision inside the compared range)."""
    from conftest import load_golden, golden_lp
    from pyslam_amd import synthetic

    def ba(seed, pose_noise, point_noise):
        return synthetic.stereo_ba(num_kf=8, num_lm=120, obs_per_lm=4, half_window=3, seed=seed, pose_noise=pose_noise,
                                   point_noise=point_noise)[0]
    tight = dict(min_cost_decrease=0.999999)
    return {
        'ba_8x120': (ba(0, 0.2, 0.4), dict(max_iters=30, **tight)),
        'ba_8x120_seed1': (ba(1, 0.4, 0.8), dict(max_iters=10, **tight)),             # genuine rejections; not run to convergence
        'ba_small': (golden_lp(load_golden('ba_small')), dict(max_iters=12, **tight)),
        'pg_small_huber': (golden_lp(load_golden('pg_small_huber')), dict(max_iters=12, **tight)),
        'pg_se2': (synthetic.pose_graph(num_poses=40, num_loops=50, dof=3, seed=5)[0], dict(max_iters=2, **tight)),     # (converged after three steps: beyond them rho is rounding noise)
    }
