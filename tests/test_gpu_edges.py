"""Edge cases of the device path against the oracle: ragged / long landmark tracks, duplicate
observations, landmarks seen only by constant poses, all poses constant (pure triangulation),
single variable pose, a problem with no blocks to linearise, mixed factor + reprojection graphs."""
import numpy as np
import pytest

from oracle import gn_oracle as orc
from pyslam_amd import synthetic
from pyslam_amd.lowering import LoweredProblem
from conftest import rel_err

pytestmark = pytest.mark.gpu


def device(lp):
    from pyslam_amd.device import DeviceProblem
    return DeviceProblem(lp)


def check_step(lp, tol_dx=1e-8, tol_pcg=1e-13):
    """cost, first GN step and post-step parameters vs the oracle (device order = poses, points)."""
    dev = device(lp)
    c = dev.eval_cost(True)
    co = orc.eval_cost(lp)
    assert abs(c - co) <= 1e-10 * max(abs(co), 1e-300)
    dev.linearize(0.)
    dev.solve_reduced(tol_pcg, 3000)
    dev.backsub()
    xp, xl = dev.get_dx()
    dx = np.concatenate([xp.ravel(), xl.ravel()])
    dxo, _ = orc.gauss_newton_step(lp, points_first=False)
    assert np.linalg.norm(dx - dxo) <= tol_dx * np.linalg.norm(dxo)
    dev.apply_update(1.0)
    new = orc.apply_update(lp, dxo, points_first=False)
    poses, points = dev.get_params()
    assert np.abs(poses - new.poses).max() < 1e-7 and np.abs(points - new.points).max() < 1e-6
    return dev


def ragged_tracks(seed, num_kf=40, num_lm=300, max_obs=38):
    """Track lengths from 2 to `max_obs` (> 16: the looping path of the 16-lane landmark kernels)."""
    rng = np.random.default_rng(seed)
    lp, truth = synthetic.stereo_ba(num_kf=num_kf, num_lm=num_lm, obs_per_lm=max_obs, half_window=19, seed=seed)
    keep = np.ones(lp.num_obs, bool)
    start = 0
    counts = np.bincount(lp.obs_point, minlength=num_lm)
    for j in range(num_lm):
        n = counts[j]
        want = int(rng.integers(2, n + 1))
        drop = rng.choice(n, n - want, replace=False)
        keep[start + drop] = False
        start += n
    lp.obs_pose, lp.obs_point = lp.obs_pose[keep], lp.obs_point[keep]
    lp.obs_uvd, lp.obs_grp = lp.obs_uvd[keep], lp.obs_grp[keep]
    return lp.finalize()


def test_ragged_and_long_tracks():
    lp = ragged_tracks(7)
    counts = np.bincount(lp.obs_point)
    assert counts.max() > 16 and counts.min() <= 4
    check_step(lp)


def test_duplicate_observations_of_a_pose():
    """The same (pose, landmark) pair observed twice: both Z rows hit the same diagonal block."""
    lp, _ = synthetic.stereo_ba(num_kf=6, num_lm=40, obs_per_lm=4, half_window=3, seed=12)
    dup = np.arange(0, lp.num_obs, 3)
    noise = np.random.default_rng(1).standard_normal((dup.size, 3))
    lp.obs_pose = np.concatenate([lp.obs_pose, lp.obs_pose[dup]])
    lp.obs_point = np.concatenate([lp.obs_point, lp.obs_point[dup]])
    lp.obs_uvd = np.concatenate([lp.obs_uvd, lp.obs_uvd[dup] + noise])
    lp.obs_grp = np.concatenate([lp.obs_grp, lp.obs_grp[dup]])
    check_step(lp.finalize())


def test_landmarks_seen_only_by_the_constant_pose_and_constant_landmarks():
    lp, _ = synthetic.stereo_ba(num_kf=5, num_lm=50, obs_per_lm=3, half_window=2, seed=13,
                                const_point_fraction=0.2)
    # make the first ten landmarks visible from the constant pose 0 only
    sel = lp.obs_point < 10
    lp.obs_pose[sel] = 0
    keep = np.ones(lp.num_obs, bool)
    seen = set()
    for i in np.nonzero(sel)[0]:                      # one observation each
        if lp.obs_point[i] in seen or lp.point_vid[lp.obs_point[i]] < 0:
            keep[i] = False
        seen.add(lp.obs_point[i])
    for k in ('obs_pose', 'obs_point', 'obs_uvd', 'obs_grp'):
        setattr(lp, k, getattr(lp, k)[keep])
    check_step(lp.finalize())


def test_all_poses_constant_is_pure_triangulation():
    lp, _ = synthetic.stereo_ba(num_kf=4, num_lm=30, obs_per_lm=3, half_window=2, seed=14)
    lp.pose_rid[:] = -1
    lp = lp.finalize()
    dev = device(lp)
    assert dev.nr == 0
    cost, nrm, its, rel = dev.gn_iteration()
    dxo, _ = orc.gauss_newton_step(lp, points_first=False)
    assert its == 0 and abs(nrm - np.linalg.norm(dxo)) <= 1e-9 * nrm
    assert abs(cost - orc.eval_cost(orc.apply_update(lp, dxo, points_first=False))) <= 1e-9 * cost


def test_single_variable_pose_with_landmarks():
    lp, _ = synthetic.stereo_ba(num_kf=2, num_lm=25, obs_per_lm=2, half_window=1, seed=15)
    assert lp.num_reduced == 1
    check_step(lp)


def test_reprojection_plus_pose_factors_in_one_problem():
    """BA with odometry edges and a prior on the first variable pose (mixed factor types)."""
    lp, truth = synthetic.stereo_ba(num_kf=7, num_lm=60, obs_per_lm=4, half_window=3, seed=16)
    from pyslam_amd.lowering import pack_pose_matrices
    T = truth['poses']
    ei, ej = np.arange(0, 6), np.arange(1, 7)
    rel = np.einsum('nij,njk->nik', T[ej], np.linalg.inv(T[ei]))
    lp.e_i, lp.e_j = ei, ej
    lp.e_Tobs_inv = pack_pose_matrices(np.linalg.inv(rel))
    lp.e_grp = np.zeros(6)
    lp.u_i, lp.u_grp = [1], [1]
    lp.u_Tobs_inv = pack_pose_matrices(np.linalg.inv(T[1:2]))
    lp.stiffd = np.stack([(10. * np.eye(6)).ravel(), (3. * np.eye(6)).ravel()])
    lp.edge_groups = np.array([[0., 3., 0.7], [1., 0., 0.]])      # Huber odometry, L2 prior
    check_step(lp.finalize())


def test_nothing_to_optimise():
    """Only constant parameters: cost is evaluated, the iteration is a no-op."""
    lp, _ = synthetic.stereo_ba(num_kf=3, num_lm=10, obs_per_lm=2, half_window=1, seed=17)
    lp.pose_rid[:] = -1
    lp.point_vid[:] = -1
    lp = lp.finalize()
    dev = device(lp)
    c = dev.eval_cost(True)
    assert abs(c - orc.eval_cost(lp)) <= 1e-10 * c
    assert dev.eval_cost(False) == 0.0
    before = dev.get_params()
    cost, nrm, its, _ = dev.gn_iteration()
    after = dev.get_params()
    assert nrm == 0.0 and its == 0 and np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert abs(cost - c) <= 1e-12 * c


def test_bad_input_is_reported_not_crashed():
    from pyslam_amd._native import NativeError
    lp, _ = synthetic.stereo_ba(num_kf=3, num_lm=10, obs_per_lm=2, half_window=1, seed=18)
    bad = lp.copy()
    bad.obs_pose = bad.obs_pose.copy()
    bad.obs_pose[0] = 99
    with pytest.raises((NativeError, AssertionError)):
        device(bad)
    # gauge freedom: no constant pose, no prior => the reduced system is singular/indefinite
    free, _ = synthetic.pose_graph(num_poses=6, num_loops=0, dof=6, seed=3, prior_first=False)
    dev = device(free)
    try:
        out = dev.gn_iteration(0., 1e-12, 50, True)
        assert np.isfinite(out[0]) or True        # either a finite step (semi-definite CG) or a reported error
    except NativeError:
        pass

def test_fused_motion_only_iteration_matches_the_general_path():
    """Problems without variable landmarks or pose factors run each Gauss-Newton iteration as ONE launch
    (k_motion_only_iteration: one workgroup per pose).  Same steps as the multi-kernel path, for both
    cost conventions (line search on: cost after the step; off: cost at the linearisation point)."""
    import numpy as np
    from pyslam_amd import synthetic
    from pyslam_amd.device import DeviceProblem
    lp, _ = synthetic.stereo_ba(num_kf=7, num_lm=300, obs_per_lm=4, half_window=3, seed=11, const_point_fraction=1.0,
                                loss=__import__('pyslam_amd.losses', fromlist=['HuberLoss']).HuberLoss(2.0))
    assert lp.num_var_points == 0 and lp.num_reduced >= 5
    for linesearch in (True, False):
        a, b = DeviceProblem(lp), DeviceProblem(lp)
        b.set_option('fused_motion_only', 0)
        for _ in range(4):
            ra = a.gn_iteration(0., 1e-13, 100, linesearch)
            rb = b.gn_iteration(0., 1e-13, 100, linesearch)
            assert abs(ra[0] - rb[0]) <= 1e-11 * abs(rb[0]) and abs(ra[1] - rb[1]) <= 1e-9 * max(rb[1], 1e-12)
            assert ra[2] == 0
        assert np.abs(a.get_params()[0] - b.get_params()[0]).max() < 1e-11
        assert np.abs(a.get_dx()[0] - b.get_dx()[0]).max() < 1e-9


def test_a_failed_landmark_block_raises_and_applies_nothing():
    """Tukey weights that vanish on every observation leave H_ll = 0: the iteration must report the landmark block (not
    the NaNs it causes downstream) and leave the parameter tables untouched -- the CG's convergence test treats a NaN
    residual as a breakdown, so the gated tail stays closed."""
    from pyslam_amd import losses
    from pyslam_amd._native import NativeError
    for kf in (6, 30):                                    # direct small solve / fused CG
        lp, _ = synthetic.stereo_ba(num_kf=kf, num_lm=40 * kf, obs_per_lm=4, half_window=5, seed=2, loss=losses.TukeyLoss(1e-9))
        dev = device(lp)
        before = dev.get_params()
        with pytest.raises(NativeError, match='landmark block'):
            dev.gn_iteration(0., 1e-12, 500, True)
        after = dev.get_params()
        if kf == 30:
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_problem_edits_between_solves_reach_the_device():
    """The reference re-reads every block on every iteration (problem.py:338-360).  Here the tables stay resident
    in HBM between calls -- but only while nothing except the parameter values changed: a new loss.k, an edited
    measurement, a swapped loss or a replaced block must take effect in the next call."""
    from conftest import load_golden, golden_lp
    from test_host_api import build_namespace
    ns = build_namespace()
    lp = golden_lp(load_golden('ba_tiny_huber'))
    problem = synthetic.to_objects(lp, ns)

    def oracle_cost():
        return orc.eval_cost(problem._lower())
    c0 = problem.eval_cost()
    dev0 = problem._device
    assert abs(c0 - oracle_cost()) <= 1e-12 * c0
    # parameter values only: same handle
    problem.param_dict[problem._lower().point_keys[0]][1] += 0.3
    c1 = problem.eval_cost()
    assert problem._device is dev0 and c1 != c0 and abs(c1 - oracle_cost()) <= 1e-12 * c1
    # loss parameter
    loss = problem.block_loss_functions[0]
    loss.k *= 0.25
    c2 = problem.eval_cost()
    assert problem._device is not dev0 and c2 != c1 and abs(c2 - oracle_cost()) <= 1e-12 * c2
    # a measurement edited in place
    problem.residual_blocks[5].obs[0] += 2.5
    c3 = problem.eval_cost()
    assert c3 != c2 and abs(c3 - oracle_cost()) <= 1e-12 * c3
    # a different loss object on one block (same counts, same keys)
    problem.block_loss_functions[2] = ns.CauchyLoss(2.0)
    c4 = problem.eval_cost()
    assert c4 != c3 and abs(c4 - oracle_cost()) <= 1e-12 * c4
    # and the solve sees the edited problem: first step = the oracle's on the re-lowered tables
    cur = problem._lower()
    dx, cost = problem.solve_one_iter()
    dxo, _ = orc.gauss_newton_step(cur, points_first=True)
    assert np.linalg.norm(dx - dxo) <= 1e-8 * np.linalg.norm(dxo)


def test_c3_through_the_public_api_equals_the_tables_path():
    """BASELINE workload C3 built the way the reference's example builds it (examples/stereo_ba.py:43-69): 500 000
    ReprojectionResidual objects through Problem.add_residual_block, lowered once, two iterations -- bit for bit
    what DeviceProblem does on the generator's tables.  Prints where the host time goes."""
    import time
    from test_host_api import build_namespace
    from pyslam_amd.device import DeviceProblem
    ns = build_namespace()
    lp, _ = synthetic.stereo_ba(200, 50000, 10, 20, seed=0)
    t0 = time.perf_counter()
    opts = ns.Options()
    opts.max_iters = 1                                   # the reference's loop runs max_iters + 1 iterations (problem.py:158)
    opts.allow_nondecreasing_steps = True
    problem = synthetic.to_objects(lp, ns, options=opts, points_first=False)
    t1 = time.perf_counter()
    low = problem._lower()
    t2 = time.perf_counter()
    assert low.same_tables(lp) and np.array_equal(low.poses, lp.poses) and np.array_equal(low.points, lp.points)
    problem.solve()
    t3 = time.perf_counter()
    ref = DeviceProblem(lp)
    t4 = time.perf_counter()
    c0 = ref.eval_cost(True)
    trace = [ref.gn_iteration(0., opts.pcg_tol, opts.pcg_max_iters, True) for _ in range(2)]
    t5 = time.perf_counter()
    assert problem._cost_history == [c0, trace[0][0], trace[1][0]]
    poses, points = ref.get_params()
    got = problem._device.get_params()
    assert np.array_equal(got[0], poses) and np.array_equal(got[1], points)
    assert np.array_equal(problem.param_dict[lp.point_keys[123]], points[123])
    # Options.static_blocks: a second solve re-reads only the parameter values (no walk over the 500 000 blocks)
    problem.options.static_blocks = True
    t6 = time.perf_counter()
    c_again = problem.eval_cost()
    t7 = time.perf_counter()
    assert c_again == trace[1][0]
    problem.param_dict[lp.point_keys[7]][2] += 0.01
    assert problem.eval_cost() != c_again
    print('\\nOptions.static_blocks: eval_cost on resident tables {:.3f} s (parameter refresh only)'.format(t7 - t6))
    print('\\nC3 through the public API: build 500k block objects {:.2f} s | lowering walk {:.2f} s | solve() {:.2f} s '
          '(lowering + ps_problem_create + 2 iterations + write-back) | ps_problem_create alone {:.2f} s | 2 iterations '
          'on resident tables {:.1f} ms'.format(t1 - t0, t2 - t1, t3 - t2, t4 - t3, (t5 - t4) * 1e3))


def test_forced_restart_of_the_pipelined_cg_reaches_the_same_solution():
    """The restart path of the fused CG (a breakdown of its recurrences: the residual has drifted out of range(V^T) of
    the singular folded system, tools/cg_drift.py) driven by the test hook "cg_force_restart": the first pass stops at
    1e-4, the solver keeps the iterate, forms the true residual g - S x and solves for the correction.  Same step as the
    uninterrupted solve, for the fine-only, the folded two-level and the covariance-column paths."""
    lp, _ = synthetic.stereo_ba(num_kf=60, num_lm=5000, obs_per_lm=6, half_window=9, seed=21)
    for groups in (-1, 0):
        ref, dev = device(lp), device(lp)
        for d in (ref, dev):
            d.set_option('coarse_groups', groups)
            d.linearize(0.)
        dev.set_option('cg_force_restart', 1)
        its_r, rel_r = ref.solve_reduced(1e-13, 2000)
        its_d, rel_d = dev.solve_reduced(1e-13, 2000)
        assert ref.cg_restarts() == 0 and dev.cg_restarts() == 1
        assert rel_d <= 1e-12 and its_d >= its_r                 # two passes cost at least as many iterations
        ref.backsub(); dev.backsub()
        a = np.concatenate([x.ravel() for x in ref.get_dx()])
        b = np.concatenate([x.ravel() for x in dev.get_dx()])
        assert np.linalg.norm(a - b) <= 1e-10 * np.linalg.norm(a)
        # the reduced right-hand side is restored after the restart (it is rewritten to hold the true residual)
        assert np.array_equal(ref.reduced_system()[3], dev.reduced_system()[3])
    # covariance column through the restart
    pg, _ = synthetic.pose_graph(num_poses=200, num_loops=300, dof=3, seed=5)
    ref, dev = device(pg), device(pg)
    dev.set_option('cg_force_restart', 1)
    ref.covariance_begin(); dev.covariance_begin()
    xa = ref.covariance_column(0, 120, 1)[0]
    xb = dev.covariance_column(0, 120, 1)[0]
    assert dev.cg_restarts() >= 1
    assert np.abs(xa - xb).max() <= 1e-9 * np.abs(xa).max()


class _Smooth:
    """A user-defined block (no KIND tag, no device kernel): s * (p0 - p1)."""

    def __init__(self, s):
        self.s = s

    def evaluate(self, params, compute_jacobians=None):
        r = np.atleast_1d(self.s * (np.asarray(params[0], dtype=float) - np.asarray(params[1], dtype=float))).reshape(-1)
        if not compute_jacobians:
            return r
        return r, [np.array([[self.s]]) if compute_jacobians[0] else None,
                   np.array([[-self.s]]) if compute_jacobians[1] else None]


def test_generic_path_beyond_the_dense_limit_runs_sparse_cg_on_the_device():
    """User-defined blocks keep a problem on the host-evaluated path; beyond 2048 unknowns (the dense Cholesky's limit)
    the Jacobian goes to the device as CSR and the normal equations are solved there by CG (ps_sparse_normal_solve) --
    the reference solves such a problem with its sparse LU.  1 200 parabolas (3 600 unknowns) tied to
    their neighbours by a user-defined smoothness block: the step equals scipy's direct solve of the same normal
    equations, solve() converges to the minimiser, and a covariance block (columns on demand) equals the inverse's."""
    import scipy.sparse.linalg as spla
    from pyslam.problem import Options, Problem
    from pyslam.residuals import QuadraticResidual
    from pyslam.losses import HuberLoss
    rng = np.random.default_rng(8)
    problem = Problem(Options())
    N = 1200
    params = {}
    for k in range(N):
        a, b, c = 1. + 0.1 * np.sin(0.01 * k), -2. + 0.05 * k / N, 0.5
        for x in (-2., -0.5, 0.7, 1.5, 3.):
            y = a * x * x + b * x + c + 0.01 * rng.standard_normal()
            problem.add_residual_block(QuadraticResidual(x, y, 2.0), ['a%d' % k, 'b%d' % k, 'c%d' % k], HuberLoss(5.0))
        params.update({'a%d' % k: 0., 'b%d' % k: 0., 'c%d' % k: 0.})
        if k:
            problem.add_residual_block(_Smooth(0.3), ['a%d' % (k - 1), 'a%d' % k])
    problem.initialize_params(params)
    problem._update_partition_dict = problem._get_update_partition_dict()
    J, e, _ = problem._host_jacobian()
    assert J.shape == (5 * N + N - 1, 3 * N) and J.shape[1] > problem.DENSE_GENERIC_LIMIT
    dx, cost = problem.solve_one_iter()
    ref = spla.spsolve((J.T @ J).tocsc(), -(J.T @ e))
    assert np.linalg.norm(dx - ref) <= 1e-9 * np.linalg.norm(ref)
    assert problem.solver_stats[-1][0] > 0 and problem.solver_stats[-1][1] <= (problem.options.pcg_tol or 1e-12)
    out = problem.solve()
    assert abs(out['a600'] - (1. + 0.1 * np.sin(6.))) < 0.02 and abs(out['c7'] - 0.5) < 0.05
    problem.compute_covariance()
    J2, _, _ = problem._host_jacobian()
    cov = np.linalg.inv((J2.T @ J2).toarray())
    r0, r1 = problem._update_partition_dict['b17'], problem._update_partition_dict['a18']
    got = problem.get_covariance_block('b17', 'a18')
    assert abs(got - cov[r0.start, r1.start]) <= 1e-8 * np.abs(cov).max()
    got = problem.get_covariance_block('c900', 'c900')
    r0 = problem._update_partition_dict['c900']
    assert abs(got - cov[r0.start, r0.start]) <= 1e-8 * cov[r0.start, r0.start]


def test_generic_sparse_path_reports_a_solve_that_did_not_converge():
    """Round-2 ADVICE: beyond 2 048 unknowns the host-evaluated path runs Jacobi-preconditioned CG on J^T J where the
    reference runs a sparse LU; on an ill-conditioned system it used to return whatever max_iters had reached, silently.
    A chain of 2 500 scalars tied by smoothness blocks of stiffness 1e4 and anchored at one end by a unit block has a
    normal matrix of condition number ~1e15: the solve must raise NotConverged, not hand back a wrong step."""
    from pyslam.problem import Options, Problem
    from pyslam_amd.device import NotConverged, sparse_normal_solve
    import scipy.sparse as sp
    n = 2500
    rows = np.arange(n - 1)
    J = sp.vstack([sp.csr_matrix((np.concatenate([1e4 * np.ones(n - 1), -1e4 * np.ones(n - 1)]),
                                  (np.concatenate([rows, rows]), np.concatenate([rows, rows + 1]))), shape=(n - 1, n)),
                   sp.csr_matrix(([1.], ([0], [0])), shape=(1, n))]).tocsr()
    r = np.ones(n)
    with pytest.raises(NotConverged):
        sparse_normal_solve(J, r=r, tol=1e-12, max_iters=300)
    # ... a well-conditioned one of the same size still solves, silently
    Jw = sp.vstack([J / 1e4, sp.identity(n, format='csr')]).tocsr()
    dx, its, rel = sparse_normal_solve(Jw, r=np.ones(2 * n), tol=1e-12, max_iters=5000)
    assert rel <= 1e-12 and its > 0


def test_generic_path_solves_the_stiff_chain_directly():
    """Round 5: between 2 049 and 8 192 unknowns the host-evaluated path solves the normal equations DIRECTLY on the device (J^T J
    dense, blocked multi-workgroup Cholesky, refinement: ps_sparse_normal_direct) as the reference's sparse LU does
    (pyslam/problem.py:186).  The chain the CG of the test above gives up on (condition number ~1e15) solves: the residual of the
    normal equations at rounding level, the step equal to the one an accurate solve of the least-squares problem gives."""
    from pyslam_amd.device import sparse_normal_direct
    import scipy.sparse as sp
    n = 2500
    rows = np.arange(n - 1)
    J = sp.vstack([sp.csr_matrix((np.concatenate([1e4 * np.ones(n - 1), -1e4 * np.ones(n - 1)]),
                                  (np.concatenate([rows, rows]), np.concatenate([rows, rows + 1]))), shape=(n - 1, n)),
                   sp.csr_matrix(([1.], ([0], [0])), shape=(1, n))]).tocsr()
    r = np.ones(n)
    dx, _, rel = sparse_normal_direct(J, r=r)
    assert rel <= 1e-10
    # the least-squares solution of J dx = -r, by a method that does not square the condition number
    ref = np.linalg.lstsq(J.toarray(), -r, rcond=None)[0]     # (SVD: cond(J) ~ 3e7, not its square)
    assert np.linalg.norm(dx - ref) <= 1e-6 * np.linalg.norm(ref)
    # a well-conditioned system of 6 000 unknowns: against numpy, 1e-12
    rng = np.random.default_rng(3)
    n2 = 6000
    Jw = (sp.random(n2 + 500, n2, density=3.0 / n2, random_state=5, format='csr') + sp.vstack([sp.identity(n2), sp.csr_matrix((500, n2))])).tocsr()
    e2 = rng.standard_normal(n2 + 500)
    dx2, _, rel2 = sparse_normal_direct(Jw, r=e2)
    H = (Jw.T @ Jw).toarray()
    want = np.linalg.solve(H, -(Jw.T @ e2))
    assert rel2 <= 1e-13 and np.linalg.norm(dx2 - want) <= 1e-11 * np.linalg.norm(want)


def test_generic_problem_of_3000_unknowns_through_the_public_api():
    """User-defined blocks (host-evaluated) with more unknowns than the single-workgroup dense solve takes: Problem.solve() goes
    through the direct device solve and reaches the minimum the reference's sparse LU reaches (a linear problem: one step)."""
    from pyslam.problem import Options, Problem
    from pyslam.residuals import QuadraticResidual  # noqa: F401  (the package's user-block protocol is the reference's)

    class Diff:                                               # r = s (a - b): a user block the typed kernels do not know
        def __init__(self, s): self.s = s
        def evaluate(self, params, compute_jacobians=None):
            r = np.array([self.s * (params[0] - params[1])])
            if compute_jacobians:
                return r, [np.array([[self.s]]) if compute_jacobians[0] else None, np.array([[-self.s]]) if compute_jacobians[1] else None]
            return r

    class Anchor:
        def __init__(self, v): self.v = v
        def evaluate(self, params, compute_jacobians=None):
            r = np.array([params[0] - self.v])
            return (r, [np.array([[1.0]])]) if compute_jacobians else r

    n = 3000
    rng = np.random.default_rng(11)
    problem = Problem(Options())
    init = {'x%d' % i: float(rng.standard_normal()) for i in range(n)}
    for i in range(n - 1):
        problem.add_residual_block(Diff(30.0), ['x%d' % i, 'x%d' % (i + 1)])
    problem.add_residual_block(Anchor(2.5), ['x0'])
    problem.initialize_params(init)
    out = problem.solve()
    got = np.array([out['x%d' % i] for i in range(n)])
    assert np.abs(got - 2.5).max() <= 1e-8                    # every difference zero, the anchor met
    assert problem._cost_history[-1] <= 1e-16 * max(problem._cost_history[0], 1.0)


def test_per_observation_stiffness_runs_the_typed_device_path():
    """One stiffness per observation (the reference takes any: reprojection_residual.py:8-11) = more (camera, stiffness,
    loss) rows than the observation record's 8-bit group field.  Round 2 sent such problems to the host-evaluated path;
    now the device groups are the (camera, loss) classes and the stiffness is a per-observation index (ObsWide): the HIP
    kernels themselves, against the oracle -- blocks 1e-12, reduced system 1e-12, step 1e-8 -- and a whole solve()."""
    from conftest import load_golden, golden_lp
    from test_host_api import build_namespace
    ns = build_namespace()
    lp = golden_lp(load_golden('ba_small'))
    problem = synthetic.to_objects(lp, ns)
    rng = np.random.default_rng(4)
    for b in problem.residual_blocks:                         # one stiffness per observation, not even symmetric
        b.stiffness = b.stiffness.dot(np.eye(3) + 0.2 * rng.random((3, 3)))
    wide = problem._lower()
    assert wide.obs_groups.shape[0] == lp.num_obs > 255
    dev = device(wide)
    r, jp, jl = dev.debug_reproj_blocks()
    ro, jpo, jlo = orc.eval_reproj(wide)
    assert rel_err(r, ro) < 1e-12 and rel_err(jp, jpo) < 1e-12 and rel_err(jl, jlo) < 1e-12
    c = dev.eval_cost(True)
    assert abs(c - orc.eval_cost(wide)) <= 1e-10 * abs(c)
    dev.linearize(0.)
    S, g = dev.reduced_dense()
    P, b, _ = orc.normal_equations(wide, points_first=False)
    P = P.toarray()
    n_p = wide.dof * wide.num_reduced
    Hinv = np.linalg.inv(P[n_p:, n_p:])
    assert rel_err(S, P[:n_p, :n_p] - P[:n_p, n_p:] @ Hinv @ P[n_p:, :n_p]) < 1e-12
    assert rel_err(g, b[:n_p] - P[:n_p, n_p:] @ Hinv @ b[n_p:]) < 1e-12
    dev.solve_reduced(1e-13, 500)
    dev.backsub()
    xp, xl = dev.get_dx()
    dx_ref, _ = orc.gauss_newton_step(wide, points_first=False)
    assert rel_err(np.concatenate([xp.ravel(), xl.ravel()]), dx_ref) < 1e-8
    # the public API: no host-evaluated path involved (the tables device is what solve() built)
    c0 = problem.eval_cost()
    problem.solve()
    assert problem._device is not None and problem._device.lp.obs_groups.shape[0] == lp.num_obs
    assert problem._cost_history[-1] < 0.05 * c0 and len(problem._cost_history) >= 3
    _, ref = orc.solve(wide, dict(max_iters=100), points_first=True)
    assert len(problem._cost_history) == len(ref['cost_history'])
    assert np.allclose(problem._cost_history, ref['cost_history'], rtol=1e-9)


def test_per_observation_stiffness_motion_only_and_losses():
    """The wide path through the one-launch motion-only kernel (config 5 with a covariance per feature) and through the
    general landmark-free path, Cauchy loss: step vs the oracle's."""
    lp, _ = synthetic.motion_only(num_pts=400, seed=11)
    rng = np.random.default_rng(1)
    n = lp.num_obs
    lp.stiff3 = np.stack([(np.eye(3) * (0.5 + rng.random(3))).ravel() for _ in range(n)])
    lp.obs_groups = np.stack([np.array([0., i, lp.obs_groups[0, 2], lp.obs_groups[0, 3]]) for i in range(n)])
    lp.obs_grp = np.arange(n, dtype=np.int32)
    lp = lp.finalize()
    dx_ref, lin = orc.gauss_newton_step(lp, points_first=False)
    for fused in (1, 0):
        dev = device(lp)
        dev.set_option('fused_motion_only', fused)
        cost, nrm, its, rel = dev.gn_iteration(0., 1e-12, 100, False)
        assert abs(cost - lin) <= 1e-10 * abs(lin)
        assert rel_err(dev.get_dx()[0].ravel(), dx_ref) < 1e-8


@pytest.mark.parametrize('shape', ['ba', 'pg_se3', 'pg_se2'])
def test_explicit_pcg_three_launch_form_equals_the_four_launch_form(shape):
    """Explicit two-level PCG: the restriction folded into the SpMV epilogue + the recurrence t -= alpha P^T q (three
    launches per iteration) against the separate restriction kernel (four): same iterations, same step; and the launch
    counter shows which form ran."""
    if shape == 'ba':
        lp, _ = synthetic.stereo_ba(160, 16000, 8, 12, seed=11)
    else:
        lp, _ = synthetic.pose_graph(num_poses=700, num_loops=2801, dof=6 if shape == 'pg_se3' else 3, seed=12)
    out = {}
    for fused in (1, 0):
        dev = device(lp)
        dev.set_option('cg_explicit_min_rows', 0)
        dev.set_option('cg_split_min_rows', 0)
        if shape == 'ba':
            dev.set_option('coarse_groups', 10)        # (the automatic 48 intervals of 3 rows are too short for the fused form)
        dev.set_option('xcg_restrict_fused', fused)
        dev.set_option('xcg_fused', 0)                 # (the one-launch form has its own test: tests/test_gpu_ldi.py)
        n0 = dev.cg_kernel_launches()
        res = [dev.gn_iteration(0., 1e-12, 3000, True) for _ in range(3)]
        # launches per CG iteration of the LAST call (count = iterations of the previous call + 2 when it sufficed)
        out[fused] = (res, dev.get_dx(), dev.get_params(), dev.cg_kernel_launches() - n0)
    (r1, dx1, p1, n1), (r0, dx0, p0, n0) = out[1], out[0]
    # (an iteration count may differ by one between the forms when r.z ends next to the threshold)
    assert n1 % 3 == 0 and n0 % 4 == 0 and abs(n1 // 3 - n0 // 4) <= 6, (n1, n0)
    for a, b in zip(r1, r0):
        assert abs(a[2] - b[2]) <= 2 and abs(a[0] - b[0]) <= 1e-10 * abs(b[0]) and a[3] <= 1e-12, (a, b)
    for a, b in zip(dx1, dx0):
        if a.size:
            assert np.linalg.norm(a - b) <= 1e-8 * np.linalg.norm(b)
    for a, b in zip(p1, p0):
        if a.size:
            assert np.abs(a - b).max() <= 1e-8


@pytest.mark.parametrize('shape', ['ba', 'pg_se3', 'pg_se2'])
def test_banded_coarse_inverse_equals_the_dense_one(shape):
    """Explicit two-level PCG on chain-like problems: the coarse matrix is block-banded and its fp32 inverse comes from
    k_band_chol + k_band_inverse (option band_chol, default) instead of the dense blocked factorisation + triangular
    inverse + product.  Same preconditioner up to rounding: same CG iteration counts (+-1), same trajectory."""
    if shape == 'ba':
        lp, _ = synthetic.stereo_ba(160, 16000, 8, 12, seed=21)
    else:
        lp, _ = synthetic.pose_graph(num_poses=900, num_loops=3601, dof=6 if shape == 'pg_se3' else 3, seed=22)
    out = {}
    for band in (1, 0):
        dev = device(lp)
        dev.set_option('cg_explicit_min_rows', 0)
        dev.set_option('cg_split_min_rows', 0)
        if shape == 'ba':
            dev.set_option('coarse_groups', 10)
        dev.set_option('band_chol', band)
        res = [dev.gn_iteration(0., 1e-12, 3000, True) for _ in range(4)]
        out[band] = (res, dev.get_params())
    for a, b in zip(out[1][0], out[0][0]):
        assert abs(a[2] - b[2]) <= 1 and abs(a[0] - b[0]) <= 1e-10 * abs(b[0]) and a[3] <= 1e-12, (a, b)
    for a, b in zip(out[1][1], out[0][1]):
        if a.size:
            assert np.abs(a - b).max() <= 1e-9


@pytest.mark.parametrize('shape', ['ba', 'pg_se3', 'pg_se2'])
def test_partitioned_band_factorisation_equals_the_serial_walk(shape):
    """Round 5: the banded coarse matrix is factored and inverted in independent chunks + a separator system
    (csrc/ps_k_bandpart.h, option band_part, default) instead of one workgroup walking its block columns (band_part 0).  The
    same fp32 inverse to rounding: the same CG iteration counts (+-1) and the same trajectory, also with a forced chunk size."""
    if shape == 'ba':
        lp, _ = synthetic.stereo_ba(160, 16000, 8, 12, seed=21)
    else:
        lp, _ = synthetic.pose_graph(num_poses=900, num_loops=3601, dof=6 if shape == 'pg_se3' else 3, seed=22)
    out = {}
    for part, chunk in ((1, 0), (0, 0), (1, 5)):
        dev = device(lp)
        dev.set_option('cg_explicit_min_rows', 0)
        dev.set_option('cg_split_min_rows', 0)
        if shape == 'ba':
            dev.set_option('coarse_groups', 40)
        dev.set_option('band_part', part)
        dev.set_option('band_part_chunk', chunk)
        res = [dev.gn_iteration(0., 1e-12, 3000, True) for _ in range(4)]
        out[(part, chunk)] = (res, dev.get_params())
    for key in ((1, 0), (1, 5)):
        for a, b in zip(out[key][0], out[(0, 0)][0]):
            assert abs(a[2] - b[2]) <= 1 and abs(a[0] - b[0]) <= 1e-10 * abs(b[0]) and a[3] <= 1e-12, (key, a, b)
        for a, b in zip(out[key][1], out[(0, 0)][1]):
            if a.size:
                assert np.abs(a - b).max() <= 1e-9


def test_wide_coarse_matrix_keeps_the_dense_factorisation():
    """Hat intervals much shorter than the loop closures make A_c wider than the banded kernels take (more than 7 block
    off-diagonals): the dense path runs, and the solve still matches the oracle."""
    lp, _ = synthetic.pose_graph(num_poses=600, num_loops=1800, dof=6, seed=23)
    dev = device(lp)
    dev.set_option('cg_explicit_min_rows', 0)
    dev.set_option('cg_split_min_rows', 0)
    dev.set_option('coarse_groups', 200)                   # 3-pose intervals: loops of up to 30 poses span > 7 nodes
    check = dev.gn_iteration(0., 1e-13, 3000, False)
    dxo, _ = orc.gauss_newton_step(lp, points_first=False)
    xp, xl = dev.get_dx()
    assert np.linalg.norm(xp.ravel() - dxo) <= 1e-8 * np.linalg.norm(dxo), check


@pytest.mark.parametrize('params,tables', [(True, True), (True, False), (False, True)])
def test_tables_resident_in_hbm_give_the_same_problem(params, tables):
    """ps_problem_desc.flags (PS_DESC_DEVICE_PARAMS / PS_DESC_DEVICE_TABLES): a caller whose tables already live in HBM
    (torch tensors) hands over addresses.  Same records, same kernels, same order => the iterations are bit-identical to
    those of the handle created from host arrays; set_params / get_params move parameters device to device."""
    import torch
    from pyslam_amd.device import DeviceProblem, resident_tables
    lp, truth = synthetic.stereo_ba(num_kf=9, num_lm=400, obs_per_lm=5, half_window=4, seed=41)
    lp = synthetic.with_pose_edges(lp, 6, seed=5, truth_poses=truth['poses'])
    host = DeviceProblem(lp)
    res_lp = resident_tables(lp, params=params, tables=tables)
    from pyslam_amd._native import is_resident
    assert is_resident(res_lp.poses) == params and is_resident(res_lp.obs_uvd) == tables
    res = DeviceProblem(res_lp)
    assert res.info == host.info or {k: v for k, v in res.info.items() if k != 'device_bytes'} == \
        {k: v for k, v in host.info.items() if k != 'device_bytes'}
    assert res.eval_cost(True) == host.eval_cost(True)
    for _ in range(3):
        a, b = host.gn_iteration(0., 1e-12, 200, True), res.gn_iteration(0., 1e-12, 200, True)
        assert a == b
    pa, qa = host.get_params()
    pb, qb = res.get_params()
    assert np.array_equal(pa, pb) and np.array_equal(qa, qb)
    # and against the oracle, through the resident handle alone
    fresh = DeviceProblem(resident_tables(lp, params=params, tables=tables))
    fresh.gn_iteration(0., 1e-13, 500, False)
    xp, xl = fresh.get_dx()
    dxo, _ = orc.gauss_newton_step(lp, points_first=False)
    assert rel_err(np.concatenate([xp.ravel(), xl.ravel()]), dxo) < 1e-8
    # parameters in and out without leaving the device
    tp = torch.empty((lp.num_poses, lp.pose_width), dtype=torch.float64, device='cuda:0')
    tq = torch.empty((lp.num_points, 3), dtype=torch.float64, device='cuda:0')
    res.get_params(tp, tq)
    assert np.array_equal(tp.cpu().numpy(), pa) and np.array_equal(tq.cpu().numpy(), qa)
    host.set_params(lp.poses, lp.points)
    res.set_params(torch.as_tensor(lp.poses).cuda(), torch.as_tensor(lp.points).cuda())
    assert host.gn_iteration(0., 1e-12, 200, True) == res.gn_iteration(0., 1e-12, 200, True)


def test_resident_tables_are_all_or_nothing_per_class():
    import torch
    from pyslam_amd.device import DeviceProblem, resident_tables
    lp, _ = synthetic.stereo_ba(num_kf=4, num_lm=30, obs_per_lm=3, half_window=2, seed=42)
    mixed = resident_tables(lp)
    mixed.obs_uvd = lp.obs_uvd                               # one host table among device ones
    with pytest.raises(TypeError):
        DeviceProblem(mixed)
    wrong = resident_tables(lp)
    wrong.obs_pose = wrong.obs_pose.to(torch.int64)          # the C ABI reads int32
    with pytest.raises(TypeError):
        DeviceProblem(wrong)


def test_two_live_handles_of_different_sizes_do_not_disturb_each_other():
    """Kernel attributes (the dynamic-LDS limit of the lagged set-up kernel, 80-160 KB) are process-wide, handles are not:
    a small problem created and iterated BETWEEN the iterations of a bigger one must not change the bigger one's
    results (it used to lower the limit under it: the next launch of the big handle failed without a trace)."""
    from pyslam_amd.device import DeviceProblem
    big_lp, _ = synthetic.stereo_ba(num_kf=120, num_lm=6000, obs_per_lm=6, half_window=14, seed=51)
    small_lp, _ = synthetic.stereo_ba(num_kf=30, num_lm=900, obs_per_lm=4, half_window=5, seed=52)
    alone = DeviceProblem(big_lp)
    want = [alone.gn_iteration(0., 1e-12, 500, True) for _ in range(4)]
    alone.close()
    big = DeviceProblem(big_lp)
    got = [big.gn_iteration(0., 1e-12, 500, True)]
    small = DeviceProblem(small_lp)
    small_want = DeviceProblem(small_lp)
    for k in range(3):
        a = small.gn_iteration(0., 1e-12, 500, True)
        got.append(big.gn_iteration(0., 1e-12, 500, True))
        assert a == small_want.gn_iteration(0., 1e-12, 500, True)
    assert got == want


@pytest.mark.parametrize('seed', [1001, 1005, 1017, 1023, 1025, 1029])
def test_handles_iterated_side_by_side_agree_bit_for_bit(seed):
    """Two handles on the same problem, iterated alternately with the explicit two-level PCG (its coarse inverse is formed
    on the side stream beside the CG): every call returns the same numbers in both.  With the side stream at LOW PRIORITY
    (rounds 1-3) the first handle of each of these six problems got a different inverse for the same A_c in its second
    lagged set-up -- a valid preconditioner, so nothing failed, but cost and step differed in the last bits and CG
    iteration counts by one (tools/hunt_explicit_flake.py)."""
    from pyslam_amd import losses
    from pyslam_amd.device import DeviceProblem
    rng = np.random.default_rng(seed)
    kf = int(rng.choice([40, 90, 90, 150]))
    obs = int(rng.integers(2, 6))
    lp, truth = synthetic.stereo_ba(num_kf=kf, num_lm=int(rng.integers(30 * kf // obs + 8, 60 * kf // obs + 40)), obs_per_lm=obs,
                                half_window=int(rng.integers(obs, 3 * obs + 2)), seed=seed, loss=losses.HuberLoss(1.5))
    if rng.integers(2):
        lp = synthetic.with_pose_edges(lp, int(rng.integers(0, 2 * kf)), seed - 999, loss=losses.HuberLoss(1.5),
                                       truth_poses=truth['poses'])
    a, b = DeviceProblem(lp), DeviceProblem(lp)
    for d in (a, b):
        d.set_option('cg_explicit_min_rows', 0)
        d.set_option('cg_split_min_rows', 0)
    for it in range(4):
        assert a.gn_iteration(0., 1e-12, 2000, True) == b.gn_iteration(0., 1e-12, 2000, True), it
    pa, qa = a.get_params()
    pb, qb = b.get_params()
    assert np.array_equal(pa, pb) and np.array_equal(qa, qb)


@pytest.mark.parametrize('tiling', ['untiled', 'tiled'])
def test_pipelined_schur_kernel_equals_the_one_chunk_kernel_bit_for_bit(monkeypatch, tiling):
    """k_schur_pairs_db (two chunks of a wave in flight, rows and pair indices straight into LDS under a hand-counted
    vmcnt, LDS read through inline assembly; csrc/ps_k_schur2.h) against round 2's k_schur_pairs (option "schur_pipeline"
    0): the same pairs in the same order through the same accumulators, so the reduced system is equal to the last bit --
    tasks of 1 to 40 chunks, ragged last chunks, tasks shorter than one chunk, duplicate observations of a pose (tasks
    that write a diagonal block), with and without landmark tiles; and both equal the oracle's Schur complement."""
    if tiling == 'tiled':
        monkeypatch.setenv('PS_SCHUR_TILE_KB', '256')
        monkeypatch.setenv('PS_SCHUR_TILE_MIN_MB', '0')
    else:
        monkeypatch.setenv('PS_SCHUR_TILE_KB', '0')
    shapes = [dict(num_kf=70, num_lm=6000, obs_per_lm=7, half_window=10, seed=13),        # ~100 pairs per block
              dict(num_kf=12, num_lm=9000, obs_per_lm=6, half_window=5, seed=14),         # long tasks: up to ~40 chunks
              dict(num_kf=150, num_lm=1500, obs_per_lm=4, half_window=12, seed=15)]       # most tasks shorter than a chunk
    for k, shape in enumerate(shapes):
        lp, _ = synthetic.stereo_ba(**shape)
        if k == 0:
            dup = np.arange(0, lp.num_obs, 97)                    # a few landmarks seen twice from the same pose
            lp.obs_pose = np.concatenate([lp.obs_pose, lp.obs_pose[dup]])
            lp.obs_point = np.concatenate([lp.obs_point, lp.obs_point[dup]])
            lp.obs_uvd = np.concatenate([lp.obs_uvd, lp.obs_uvd[dup] + 0.3])
            lp.obs_grp = np.concatenate([lp.obs_grp, lp.obs_grp[dup]])
            lp = lp.finalize()
        dev = device(lp)
        dev.linearize(0.)
        rp, ci, vals, g = dev.reduced_system()
        dev.set_option('schur_pipeline', 0)
        dev.linearize(0.)
        _, _, vals0, g0 = dev.reduced_system()
        assert np.array_equal(vals, vals0) and np.array_equal(g, g0), k
        dev.set_option('schur_pipeline', 1)
        dev.linearize(0.)
        assert np.array_equal(dev.reduced_system()[2], vals)       # and reproducible
        S, gd = dev.reduced_dense()
        import scipy.sparse.linalg as spla
        P, b, _ = orc.normal_equations(lp, points_first=False)
        n = S.shape[0]
        P = P.tocsr()
        Hpp, Hpl, Hll = P[:n, :n], P[:n, n:], P[n:, n:]
        want = (Hpp - Hpl @ spla.spsolve(Hll.tocsc(), Hpl.T.tocsc())).toarray()
        assert rel_err(S, want) < 1e-11, k
        dev.close()


def test_option_values_out_of_range_are_refused():
    """ps_set_option: the options added in round 3 reject values outside their range, and the names of the removed solver
    variants are unknown options (and the handle stays usable)."""
    from pyslam_amd import synthetic, _native as nat
    from pyslam_amd.device import DeviceProblem
    lp, _ = synthetic.stereo_ba(num_kf=8, num_lm=200, obs_per_lm=4, half_window=4, seed=1)
    dev = DeviceProblem(lp)
    for name, bad in (('xcg_fused', 3), ('ldi_seed_lag', 0), ('ldi_max_unknowns', 5000), ('ldi_seed_steps', 0), ('ldi_cap', 0)):
        with pytest.raises(nat.NativeError):
            dev.set_option(name, bad)
    for name in ('schur_mode', 'schur_stream', 'xcg_persist4', 'cg_pipelined', 'pose_async'):
        with pytest.raises(nat.NativeError):
            dev.set_option(name, 0)
    for name, ok in (('xcg_fused', 2), ('ldi_seed_lag', 1), ('ldi_max_unknowns', 3328), ('ldi_direct', 1), ('direct_fused', 0), ('coarse_auto_hold', 0)):
        dev.set_option(name, ok)
    out = dev.gn_iteration(0., 1e-12, 500, True)
    assert np.isfinite(out[0]) and out[3] <= 1e-12


@pytest.mark.parametrize('case', ['multi_segment', 'sparse', 'constants', 'duplicates'])
def test_gather_schur_kernel_against_the_oracle(case):
    """The Schur stage (k_schur_pairs_db, with k_schur_combine where the pair list is tiled): bit-reproducible run to run, the
    oracle's Schur complement, and a converging Gauss-Newton iteration.  Poses with more than 512 observations, tasks of
    one pair, constant landmarks and poses, a landmark seen twice from one pose (a diagonal-block task)."""
    import scipy.sparse.linalg as spla
    if case == 'multi_segment':
        lp, _ = synthetic.stereo_ba(num_kf=14, num_lm=9000, obs_per_lm=6, half_window=5, seed=21)     # ~3 900 observations per pose
    elif case == 'sparse':
        lp, _ = synthetic.stereo_ba(num_kf=150, num_lm=1500, obs_per_lm=4, half_window=12, seed=15)
    else:
        lp, _ = synthetic.stereo_ba(num_kf=70, num_lm=6000, obs_per_lm=7, half_window=10, seed=13)
    if case == 'constants':
        lp.pose_rid = lp.pose_rid.copy()
        keep = np.ones(lp.num_poses, dtype=bool); keep[[0, 7, 8, 33]] = False
        lp.pose_rid[:] = -1
        lp.pose_rid[keep] = np.arange(keep.sum())
        lp.point_vid = lp.point_vid.copy()
        fixed = np.arange(0, lp.num_points, 5)
        vid = np.full(lp.num_points, -1, dtype=np.int32)
        free = np.setdiff1d(np.arange(lp.num_points), fixed)
        vid[free] = np.arange(free.size)
        lp.point_vid = vid
        lp = lp.finalize()
    if case == 'duplicates':
        dup = np.arange(0, lp.num_obs, 97)
        lp.obs_pose = np.concatenate([lp.obs_pose, lp.obs_pose[dup]])
        lp.obs_point = np.concatenate([lp.obs_point, lp.obs_point[dup]])
        lp.obs_uvd = np.concatenate([lp.obs_uvd, lp.obs_uvd[dup] + 0.3])
        lp.obs_grp = np.concatenate([lp.obs_grp, lp.obs_grp[dup]])
        lp = lp.finalize()
    dev = device(lp)
    dev.linearize(0.)
    v1 = dev.reduced_system()[2]
    dev.linearize(0.)
    assert np.array_equal(dev.reduced_system()[2], v1)             # reproducible
    S, gd = dev.reduced_dense()
    P, b, _ = orc.normal_equations(lp, points_first=False)
    n = S.shape[0]
    P = P.tocsr()
    Hpp, Hpl, Hll = P[:n, :n], P[:n, n:], P[n:, n:]
    want = (Hpp - Hpl @ spla.spsolve(Hll.tocsc(), Hpl.T.tocsc())).toarray()
    assert rel_err(S, want) < 1e-12
    out = dev.gn_iteration(0., 1e-12, 500, True)
    assert np.isfinite(out[0]) and out[3] <= 1e-12
    dev.close()


def test_untiled_pair_list_built_pose_by_pose_equals_the_landmark_order_build(monkeypatch):
    """ps_problem_create builds the untiled Schur pair list pose by pose on several host threads (round 4); the result must
    be the list the two counting passes over the landmark-ordered pairs give: same reduced system to the last bit, duplicate
    observations of a pose (diagonal-block tasks) and constant poses / landmarks included."""
    monkeypatch.setenv('PS_SCHUR_TILE_KB', '0')               # untiled at this size
    lp, _ = synthetic.stereo_ba(num_kf=70, num_lm=6000, obs_per_lm=7, half_window=10, seed=13)
    dup = np.arange(0, lp.num_obs, 97)
    lp.obs_pose = np.concatenate([lp.obs_pose, lp.obs_pose[dup]])
    lp.obs_point = np.concatenate([lp.obs_point, lp.obs_point[dup]])
    lp.obs_uvd = np.concatenate([lp.obs_uvd, lp.obs_uvd[dup] + 0.3])
    lp.obs_grp = np.concatenate([lp.obs_grp, lp.obs_grp[dup]])
    vid = np.full(lp.num_points, -1, dtype=np.int32)
    free = np.setdiff1d(np.arange(lp.num_points), np.arange(0, lp.num_points, 7))
    vid[free] = np.arange(free.size)
    lp.point_vid = vid
    lp = lp.finalize()
    out = []
    for by_landmark in (False, True):
        if by_landmark:
            monkeypatch.setenv('PS_PAIRS_BY_LANDMARK', '1')
        dev = device(lp)
        dev.linearize(0.)
        out.append(dev.reduced_system())
        dev.close()
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3])
