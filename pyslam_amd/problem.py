"""Problem / Options: the reference's user-facing API over the HIP core.

Same public surface as reference pyslam/problem.py:11-409 (Options fields,
``add_residual_block``, ``initialize_params``, ``set_parameters_constant`` /
``_variable``, ``eval_cost``, ``solve``, ``solve_one_iter``,
``compute_covariance``, ``get_covariance_block``, ``summary`` and the public
attributes the reference's tests read).  What differs is where the work runs:

* recognised blocks (reprojection, pose-pose, pose prior -- ``KIND`` tags) are
  lowered ONCE into HBM tables (pyslam_amd/lowering.py) and the whole
  Gauss-Newton iteration -- residuals, Jacobians, IRLS weights, J^T J, landmark
  elimination, block-PCG, back-substitution, retraction, post-step cost -- runs
  on the MI355X (include/pyslam_hip.h: ps_gn_iteration); the host sees two
  scalars per iteration and runs the reference's termination logic on them;
* with Options.hybrid_blocks, user-defined blocks on poses are evaluated on the host beside the typed tables and their
  pose-pair blocks of J^T J join the device's reduced system (pyslam_amd/hybrid.py);
* other problems with user-defined blocks / parameters are evaluated through the
  block protocol on the host (that is user Python code) and only the normal
  equations are formed and solved on the device (ps_dense_normal_solve; beyond 2048
  unknowns J goes up as CSR and the device runs CG on J^T J: ps_sparse_normal_solve).

There is no CPU solver: without the HIP library or a GPU, solve() raises.
"""
import copy
import time

import numpy as np

from pyslam_amd.losses import L2Loss
from pyslam_amd import lowering
from pyslam_amd.lowering import NotLowerable


class Options:
    """Optimisation options (reference pyslam/problem.py:11-37) plus the knobs
    of the device solver, whose defaults reproduce the reference (lambda = 0)."""

    def __init__(self):
        self.max_iters = 100
        self.min_update_norm = 1e-6
        self.min_cost = 1e-12
        self.min_cost_decrease = 0.9

        self.linesearch_alpha = 0.8
        self.linesearch_max_iters = 10
        self.linesearch_min_cost_decrease = 0.9

        self.allow_nondecreasing_steps = False
        self.max_nondecreasing_steps = 3

        self.num_threads = 1            # kept for API compatibility; the device path ignores it

        # build-only
        self.lm_lambda = 0.             # Marquardt damping lambda * diag(J^T J); 0 = Gauss-Newton
        self.pcg_tol = None             # relative (preconditioned) residual of the reduced solve; None: the core's default -- 1e-12
                                        # for bundle adjustments, 1e-14 for pose graphs (include/pyslam_hip.h: ps_solve_reduced)
        self.pcg_max_iters = 2000
        # None / 1: this process's GPU.  'auto': landmark-sharded over the torch.distributed process group when one
        # with more than one rank exists (every rank runs the same script on the same Problem: one process per GPU).
        # 'all' or the world size: sharded, an error without a process group.
        self.devices = None
        # True: the caller promises that residual blocks, their measurements, stiffnesses and losses do not change between
        # calls on this Problem; eval_cost / solve / solve_one_iter / compute_covariance then re-read only the parameter
        # VALUES instead of walking every block again (0.29 s at 500 000 blocks).  Default False = the reference's
        # semantics: everything is re-read on every call (pyslam/problem.py:338-360).
        self.static_blocks = False
        # solve() of a one-pose motion-only Problem (the per-frame Problem of the reference's sparse pipeline) runs its
        # whole loop -- iterations, stopping rules, best-parameter bookkeeping -- in one device launch.  False: one call
        # per iteration, as every other problem shape.  Same decisions, same cost history either way.
        self.fused_solve_loop = True
        # True: a block without a typed device kernel (no KIND) whose parameters are all poses of the problem's group, at most 8
        # of them, no longer moves the whole problem to the host-evaluated generic path.  Those blocks alone are evaluated on the
        # host (their evaluate(), once with Jacobians per linearisation and once more for the cost after a step); their
        # pose-pair blocks of J~^T J~ join the typed blocks' reduced system on the device (pyslam_amd/hybrid.py).  Not for:
        # blocks on a landmark or a non-pose parameter, photometric problems, the sharded route, mixed SE(2)/SE(3) problems --
        # those take the generic path as with False.  False (default): every problem routes as before, bit for bit.
        self.hybrid_blocks = False
        # True: solve() runs the adaptive Levenberg-Marquardt loop (Nielsen's rule) instead of the reference's:
        # every step is judged by its gain ratio rho = (cost before - cost after) / (decrease the quadratic model predicted), a
        # step with rho <= 0 is taken back and retried under a larger damping, and lambda follows rho between lm_lambda_min and
        # lm_lambda_max.  lm_lambda is then the STARTING value (0, its default: 1e-3).  The cost history never increases;
        # allow_nondecreasing_steps / max_nondecreasing_steps are ignored; linesearch_max_iters must be > 0 (rho needs the cost
        # after the step).  Single-GPU typed and hybrid routes only: Options.devices and the generic host path raise ValueError.
        # False (default): nothing changes, bit for bit.
        self.lm_adaptive = False
        self.lm_lambda_min = 1e-12
        self.lm_lambda_max = 1e12


def lm_options(opt):
    """(lambda0, lambda_min, lambda_max) of an adaptive solve, lambda0 clamped as the loop clamps every lambda."""
    lo, hi = float(getattr(opt, 'lm_lambda_min', 1e-12)), float(getattr(opt, 'lm_lambda_max', 1e12))
    if not (0. < lo <= hi):
        raise ValueError('Options.lm_adaptive: 0 < lm_lambda_min <= lm_lambda_max expected, got {!r}, {!r}'.format(lo, hi))
    lam = float(getattr(opt, 'lm_lambda', 0.) or 0.)
    return min(max(lam if lam > 0. else 1e-3, lo), hi), lo, hi


def check_lm_route(opt, what=None):
    """Options.lm_adaptive on a route that does not offer it is an error, never the fixed-lambda loop in silence."""
    if not getattr(opt, 'lm_adaptive', False):
        return
    if what is not None:
        raise ValueError('Options.lm_adaptive is not offered on {} (single-GPU typed and hybrid routes only)'.format(what))
    if getattr(opt, 'devices', None) not in (None, 1, 'single'):
        raise ValueError('Options.lm_adaptive is not offered on the landmark-sharded route (Options.devices = {!r})'.format(opt.devices))
    if not opt.linesearch_max_iters > 0:
        raise ValueError('Options.lm_adaptive needs the cost after the step: Options.linesearch_max_iters must be > 0')
    lm_options(opt)


def solve_horizon(opt, iteration, nondecreasing_steps_taken):
    """Iterations the stopping rule of Problem.solve still allows AFTER iteration number `iteration` (1-based) if its step
    turns out non-decreasing: none without allow_nondecreasing_steps, else what max_nondecreasing_steps and max_iters leave.
    The device core does not start side work that needs several more iterations to pay back when fewer are to come
    (ps_set_option "solve_horizon").  csrc/ps_stop_rule.h: ps_stop_horizon."""
    if not opt.allow_nondecreasing_steps:
        return 0
    left_nd = opt.max_nondecreasing_steps - (nondecreasing_steps_taken + 1)
    left_it = opt.max_iters + 1 - iteration       # the loop stops once optimization_iters > max_iters
    return max(0, min(left_nd, left_it))


class StopRule:
    """THE stopping rule of Problem.solve (reference pyslam/problem.py:159-178) for every Python loop here; the contract of
    csrc/ps_stop_rule.h (which says the rule in words), held against that header by tests/test_stop_rule_host.py.
    `cost` is the last entry of the cost history, `iters` the iterations judged, `nd` the consecutive non-decreasing steps."""
    DONE, KEEP_BEST, RESTORE_BEST = 1, 2, 4

    def __init__(self, opt, start_cost):
        self.opt, self.iters, self.nd, self.cost = opt, 0, 0, start_cost

    @staticmethod
    def base(opt, iters, cost, dx_norm):
        """The three threshold tests (all the adaptive LM loop shares with the default one)."""
        return bool(iters > opt.max_iters or dx_norm < opt.min_update_norm or cost < opt.min_cost)

    def step(self, cost, dx_norm):
        """One finished iteration -> flags.  KEEP_BEST: store the current (post-step) parameters as best, now; RESTORE_BEST
        (implies DONE): make best the current parameters; both: store first, then restore."""
        opt = self.opt
        nondecreasing = cost >= opt.min_cost_decrease * self.cost      # (the tie counts as non-decreasing)
        self.iters += 1
        self.cost = cost
        flags = self.DONE if self.base(opt, self.iters, cost, dx_norm) else 0
        if opt.allow_nondecreasing_steps:
            if self.nd == 0:                                            # (before this step moves the count)
                flags |= self.KEEP_BEST
            self.nd = self.nd + 1 if nondecreasing else 0
            if self.nd >= opt.max_nondecreasing_steps:
                flags |= self.DONE | self.RESTORE_BEST
        elif nondecreasing:
            flags |= self.DONE
        return flags

    def horizon(self):
        """solve_horizon for the iteration about to start."""
        return solve_horizon(self.opt, self.iters + 1, self.nd)


def device_solve(dev, opt, use_core_loop=True, call_ms=None):
    """The loop of Problem.solve (reference pyslam/problem.py:130-178) on a problem resident on the device: start cost,
    then whole iterations (one ps_gn_iteration call each) until the reference's stopping rules fire, with the best
    parameters kept on the device (snapshot / restore = best_params).  -> (cost history, [(pcg iterations, relative
    residual)] per iteration).  Problem.solve() runs exactly this; bench.py times exactly this.

    `dev`: DeviceProblem, ShardedProblemView / ShardedDeviceProblem or PhotometricDevice.  A DeviceProblem runs the loop in
    the core (ps_solve: the same statements in C, no interpreter between two iterations, the start cost's pass enqueued in
    front of the first iteration); tests/test_gpu_solve_loop.py holds the two against each other.  `call_ms`, if a list, receives
    the wall clock of every iteration call in ms."""
    counts = getattr(dev, 'cg_persist_counts', None)
    failures_before = counts()[1] if counts is not None else 0
    try:
        return _device_solve_loop(dev, opt, use_core_loop, call_ms)
    finally:
        if counts is not None:
            try:
                failed = counts()[1] - failures_before
            except Exception:       # noqa: BLE001  (a closed handle: nothing to report)
                failed = 0
            if failed > 0:
                import warnings
                warnings.warn('pyslam_amd: {} reduced solve(s) of this handle ran the one-launch CG into its time-out (its workgroups were '
                              'not resident together: another process on the device, a CU mask below HIP?) and were solved again launch '
                              'by launch; the handle keeps the launch-per-iteration kernels from here on (slower, same results) -- '
                              'ps_problem_info.cg_persist_failures'.format(failed), RuntimeWarning, stacklevel=3)


def _device_solve_loop(dev, opt, use_core_loop, call_ms):
    """device_solve's body (the wrapper reports a one-launch CG that timed out)."""
    if getattr(opt, 'lm_adaptive', False):
        return _lm_solve_loop(dev, opt, use_core_loop, call_ms)
    loop = getattr(dev, 'solve_loop', None) if use_core_loop else None
    if loop is not None:
        out = loop(opt)
        if out is not None:
            if call_ms is not None:
                call_ms.extend(out[2])
            return out[0], out[1]
    if hasattr(dev, 'reset_solver_state'):
        dev.reset_solver_state()          # a solve is a function of (parameters, options), not of the handle's history
    horizon = getattr(dev, 'set_solve_horizon', None)
    # (a hybrid handle's own costs miss the host blocks: the core decides nothing from them -- ps_problem_create_hybrid)
    expect = getattr(dev, 'set_expect_next', None) if getattr(dev, 'host', None) is None else None
    linesearch = opt.linesearch_max_iters > 0
    lam = getattr(opt, 'lm_lambda', 0.)
    pcg_tol, pcg_max = (getattr(opt, 'pcg_tol', None) or 0.), getattr(opt, 'pcg_max_iters', 2000)      # (0: the core's default)
    cost = dev.eval_cost(True)
    try:
        return _reference_loop(dev, opt, expect, horizon, cost, lam, pcg_tol, pcg_max, linesearch, call_ms)
    finally:
        if expect is not None:
            expect(False)        # (also when an iteration raises: the handle must not keep "a successor follows" for later callers)


def _reference_loop(dev, opt, expect, horizon, cost, lam, pcg_tol, pcg_max, linesearch, call_ms):
    """The loop of reference pyslam/problem.py:141-178 on whole-iteration calls of `dev` (gn_iteration, snapshot, restore)."""
    history, stats = [cost], []
    rule = StopRule(opt, cost)
    last_ratio = 1.
    flags = 0
    while not flags & StopRule.DONE:
        it = rule.iters + 1
        if horizon is not None:
            horizon(rule.horizon())
        if expect is not None:            # as ps_solve (csrc/ps_abi_solver.h): will another iteration follow?
            expect(it <= opt.max_iters and
                   (rule.horizon() >= 1 if opt.allow_nondecreasing_steps else (it >= 2 and last_ratio < 0.5)))
        # one device call: linearise, solve, update, post-step cost
        t0 = time.perf_counter()
        cost, dx_norm, its, rel = dev.gn_iteration(lam, pcg_tol, pcg_max, linesearch)
        if call_ms is not None:
            call_ms.append((time.perf_counter() - t0) * 1e3)
        stats.append((its, rel))
        history.append(cost)
        last_ratio = cost / rule.cost if rule.cost > 0. else 1.
        flags = rule.step(cost, dx_norm)
        if flags & StopRule.KEEP_BEST:
            dev.snapshot()
        if flags & StopRule.RESTORE_BEST:
            dev.restore()
    return history, stats


class _HostIterations:
    """The generic host path of Problem.solve (a block without a typed kernel) as _reference_loop's `dev`: an iteration is
    solve_one_iter + the update, best parameters are a deep copy of param_dict (reference pyslam/problem.py:141-178)."""

    def __init__(self, problem):
        self.problem, self.best = problem, None

    def gn_iteration(self, *_):
        p = self.problem
        dx, cost = p.solve_one_iter()
        for k, r in p._update_partition_dict.items():
            p._perturb_by_key(k, dx[r])
        return cost, np.linalg.norm(dx), 0, 0.

    def snapshot(self):
        self.best = copy.deepcopy(self.problem.param_dict)

    def restore(self):
        self.problem.param_dict.update(self.best)


def _lm_solve_loop(dev, opt, use_core_loop, call_ms):
    """Options.lm_adaptive: the core's loop (ps_solve_lm) where the device offers it, else the same statements here on
    ps_lm_iteration (hybrid handles: the host blocks' cost is part of every cost below).  The per-iteration rows
    (lambda used, rho, accepted, model_decrease) are left on the device object as `lm_history`."""
    check_lm_route(opt)
    if not hasattr(dev, 'lm_iteration'):
        check_lm_route(opt, type(dev).__name__)
    loop = getattr(dev, 'solve_lm_loop', None) if use_core_loop else None
    if loop is not None:
        out = loop(opt)
        if out is not None:
            if call_ms is not None:
                call_ms.extend(out[2])
            dev.lm_history = out[3]
            return out[0], out[1]
    dev.reset_solver_state()
    history, stats, rows = _lm_loop(dev, opt, dev.eval_cost(True), call_ms)
    dev.lm_history = np.array(rows, dtype=np.float64).reshape(-1, 4)
    return history, stats


def _lm_loop(dev, opt, cost, call_ms):
    """Nielsen's damping rule around whole iterations (csrc/ps_abi_solver.h: ps_solve_lm is the same loop in the core).  Of
    the stopping rule it shares StopRule.base; its own two conditions are below."""
    lam, lam_min, lam_max = lm_options(opt)
    nu = 2.
    pcg_tol, pcg_max = (getattr(opt, 'pcg_tol', None) or 0.), getattr(opt, 'pcg_max_iters', 2000)
    history, stats, rows = [cost], [], []
    iters = 0
    done = False
    while not done:
        iters += 1
        prev_cost = cost
        dev.snapshot()
        t0 = time.perf_counter()
        new_cost, dx_norm, md, its, rel = dev.lm_iteration(lam, pcg_tol, pcg_max, True)
        if call_ms is not None:
            call_ms.append((time.perf_counter() - t0) * 1e3)
        stats.append((its, rel))
        ok = np.isfinite(md) and md > 0. and np.isfinite(new_cost)
        rho = (prev_cost - new_cost) / md if ok else -1.
        used, raw = lam, lam * nu
        accepted = rho > 0.
        if accepted:
            q = 2. * rho - 1.
            cost, lam, nu = new_cost, lam * max(1. / 3., 1. - q * q * q), 2.
        else:
            lam, nu = raw, nu * 2.
            dev.restore()
        lam = min(max(lam, lam_min), lam_max)
        rows.append((used, rho, 1. if accepted else 0., md))
        history.append(cost)
        done = StopRule.base(opt, iters, cost, dx_norm)
        if accepted:
            done = done or cost >= opt.min_cost_decrease * prev_cost
        else:
            done = done or raw > lam_max
    return history, stats, rows


def solve_tables(lp, options=None, stream=None, device=None):
    """BATCH ENTRY for large problems: the solve of ``Problem.solve()`` from TABLES instead of one Python object per residual
    block (INTEGRATION.md "Batch entry").  ``lp``: a ``pyslam_amd.lowering.LoweredProblem`` -- pose rows (R | t), points,
    observation columns (pose index, point index, (u, v, d), group), camera / stiffness / loss group tables, pose-pose edges and
    priors -- i.e. exactly what ``Problem.solve()`` lowers its registries to (``Problem._lower()`` returns it; ``pyslam_amd.
    synthetic`` builds it directly).  Same options, same loop (device_solve: reference pyslam/problem.py:130-178), same cost
    history bit for bit; what is skipped is the walk over 500 000 block objects (58 of the 68 ms of a C3 solve through the
    object API).  -> (cost history, poses (P, 12 | 6), points (L, 3), [(pcg iterations, relative residual)]).
    ``device``: a DeviceProblem of the same tables kept from an earlier call (its parameters are reset to ``lp``'s)."""
    from pyslam_amd.device import DeviceProblem
    options = options if options is not None else Options()
    dev = device
    if dev is None:
        dev = DeviceProblem(lp, stream=stream)
    else:
        dev.set_params(lp.poses, lp.points)
    try:
        history, stats = device_solve(dev, options)
        poses, points = dev.get_params()
    finally:
        if device is None:
            dev.close()
    return history, poses, points, stats


def triangulate_tables(lp, refine_iters=5, min_parallax_deg=1.0, stream=None, device=None):
    """Multi-view triangulation of every variable landmark of the tables ``lp`` on the device, from its observations and
    ``lp``'s poses (constant ones included): a linear start, ``refine_iters`` Gauss-Newton steps on the landmark's own robust
    reprojection cost with the poses held, a status per landmark (pyslam_amd/triangulation.py is the same
    definition in numpy).  -> (points (L, 3): ``lp.points`` with the landmarks of status 0 replaced, status (L,) int32: 0 ok,
    1 too few observations, 2 no parallax / linear start not positive definite, 3 behind a camera, -1 a constant point, not
    touched).  A refinement step whose 3 x 3 system cannot be solved (L1's NaN weight at a zero residual) ends the refinement
    like a step that does not lower the cost: the landmark keeps its last accepted point and stays 0.
    ``device``: a DeviceProblem of the same tables kept from an earlier call (its parameters are reset to ``lp``'s)."""
    from pyslam_amd.device import DeviceProblem
    dev = device
    if dev is None:
        dev = DeviceProblem(lp, stream=stream)
    else:
        dev.set_params(lp.poses, lp.points)
    try:
        pts, st = dev.triangulate(None, refine_iters, min_parallax_deg, write_back=False)
    finally:
        if device is None:
            dev.close()
    points = np.array(lp.points, dtype=np.float64).reshape(-1, 3)
    status = np.full(points.shape[0], -1, dtype=np.int32)
    var = np.nonzero(np.asarray(lp.point_vid) >= 0)[0]
    vid = np.asarray(lp.point_vid)[var]
    points[var] = pts[vid]
    status[var] = st[vid]
    return points, status


class Problem:
    def __init__(self, options=Options()):
        self.options = options
        self.param_dict = dict()
        self.residual_blocks = []
        self.block_param_keys = []
        self.block_loss_functions = []
        self.constant_param_keys = []

        self._update_partition_dict = {}
        self._covariance_matrix = None
        self._cost_history = []

        self._device = None
        self._device_sig = None
        self._device_route = None
        self._static_sig = None
        self.solver_stats = []          # per iteration: (pcg iterations, pcg relative residual)

    # ------------------------------------------------------------------
    # registry (reference problem.py:72-108)
    # ------------------------------------------------------------------
    def add_residual_block(self, block, param_keys, loss=L2Loss()):
        if isinstance(param_keys, str):
            param_keys = [param_keys]
        self.residual_blocks.append(block)
        self.block_param_keys.append(param_keys)
        self.block_loss_functions.append(loss)

    def initialize_params(self, param_dict):
        self.param_dict.update(copy.deepcopy(param_dict))

    def set_parameters_constant(self, param_keys):
        if isinstance(param_keys, str):
            param_keys = [param_keys]
        for key in param_keys:
            if key not in self.constant_param_keys:
                self.constant_param_keys.append(key)

    def set_parameters_variable(self, param_keys):
        if isinstance(param_keys, str):
            param_keys = [param_keys]
        for key in param_keys:
            if key in self.constant_param_keys:
                self.constant_param_keys.remove(key)

    # ------------------------------------------------------------------
    # lowering / device handle
    # ------------------------------------------------------------------
    def _lower(self, param_dict=None):
        pd = self.param_dict if param_dict is None else param_dict
        hybrid = getattr(self.options, 'hybrid_blocks', False) and self._route() == 'single'
        return lowering.lower(pd, self.residual_blocks, self.block_param_keys,
                              self.block_loss_functions, self.constant_param_keys, hybrid=hybrid)

    def _attach_host(self, dev):
        """A hybrid handle gets the Problem's user blocks (evaluated on the host at the device's current poses)."""
        if dev.lp.hybrid:
            from pyslam_amd.hybrid import HostBlocks
            dev.attach_host(HostBlocks(dev.lp, self.residual_blocks, self.block_param_keys, self.block_loss_functions,
                                       self.param_dict))
        return dev

    def _photometric_form(self):
        """'se3' / 'split' when the problem is ONE PhotometricResidualSE3 block on variable parameters (the dense VO
        pipeline's per-pyramid-level problem, reference pipelines/dense.py:174-186), else None."""
        if len(self.residual_blocks) != 1 or getattr(self.residual_blocks[0], 'KIND', None) != 'photometric':
            return None
        keys = self.block_param_keys[0]
        if any(k in self.constant_param_keys for k in keys) or set(keys) != set(self.param_dict.keys()):
            return None
        return {1: 'se3', 2: 'split'}.get(len(keys))

    def _get_photometric_device(self, param_dict=None):
        from pyslam_amd.device import PhotometricDevice
        form = self._photometric_form()
        block, loss, keys = self.residual_blocks[0], self.block_loss_functions[0], self.block_param_keys[0]
        sig = ('photometric', form, id(block), id(loss))
        if self._device is None or self._device_sig != sig:
            if self._device is not None:
                self._device.close()
            self._device = PhotometricDevice(block, loss, form == 'split')
            self._device_sig = sig
        pd = self.param_dict if param_dict is None else param_dict
        if form == 'se3':
            T = pd[keys[0]]
            self._device.set_pose(T.rot.as_matrix(), T.trans)
        else:
            self._device.set_pose(pd[keys[0]].as_matrix(), pd[keys[1]])
        return self._device

    def _get_device(self, param_dict=None):
        """DeviceProblem for the current structure; parameters refreshed from param_dict."""
        from pyslam_amd.device import DeviceProblem
        if self._photometric_form():
            return self._get_photometric_device(param_dict)
        dev = self._device
        if getattr(self.options, 'static_blocks', False) and dev is not None and self._device_sig == 'tables' and \
                self._device_route == self._route() and self._static_sig == self._cheap_sig():
            # the caller has declared the blocks unchanged since the tables were built: only the values are re-read
            pd = self.param_dict if param_dict is None else param_dict
            poses, points = lowering.refresh_params(pd, dev.lp)
            dev.set_params(poses, points)
            dev.lp.poses, dev.lp.points = poses, points
            if dev.lp.hybrid and dev.host is None:
                self._attach_host(dev)
            return dev
        lp = self._lower(param_dict)
        # The resident tables are reused only if EVERYTHING but the parameter values is unchanged: measurements,
        # stiffness / loss / camera groups, connectivity, constant masks (the reference re-reads all of it on every
        # iteration, problem.py:338-360, so an edited block.obs, loss.k or a swapped block must take effect).
        dev = self._device
        if dev is not None and self._device_sig == 'tables' and dev.lp.same_tables(lp) and \
                self._device_route == self._route():
            dev.set_params(lp.poses, lp.points)
            dev.lp = lp
        else:
            if dev is not None:
                dev.close()
            self._device = self._make_device(lp)
            self._device_sig = 'tables'
            self._device_route = self._route()
        self._attach_host(self._device)
        self._static_sig = self._cheap_sig()
        return self._device

    def _cheap_sig(self):
        """What Options.static_blocks checks instead of walking the blocks: counts and the constant-key list."""
        return (len(self.residual_blocks), len(self.block_param_keys), len(self.block_loss_functions),
                len(self.param_dict), tuple(self.constant_param_keys))

    def _route(self):
        """'sharded' when Options.devices asks for the landmark-sharded multi-GPU driver and a
        torch.distributed process group exists (one process per GPU), else 'single'."""
        want = getattr(self.options, 'devices', None)
        if want in (None, 1, 'single'):
            return 'single'
        try:
            import torch.distributed as dist
        except ImportError:
            dist = None
        up = dist is not None and dist.is_available() and dist.is_initialized()
        if want == 'auto':
            return 'sharded' if up and dist.get_world_size() > 1 else 'single'
        if not up:
            raise RuntimeError("Options.devices = {!r} needs an initialised torch.distributed process group "
                               "(one process per GPU, backend 'nccl')".format(want))
        if isinstance(want, int) and want != dist.get_world_size():
            raise RuntimeError("Options.devices = {} but the process group has {} ranks".format(want, dist.get_world_size()))
        return 'sharded'

    def _make_device(self, lp):
        """Upload the tables: one GPU, or this rank's landmark shard of them behind the same interface."""
        from pyslam_amd.device import DeviceProblem
        if self._route() == 'single':
            return DeviceProblem(lp)
        import torch.distributed as dist
        from pyslam_amd.distributed import ShardedProblemView
        return ShardedProblemView(lp, dist)

    def _write_back(self, dev, poses=None):
        """Copy the device parameter tables into the live param_dict objects (`poses`: rows the caller already holds, for
        a problem without named landmarks)."""
        form = self._photometric_form()
        if form:
            R, t = dev.get_pose()
            keys = self.block_param_keys[0]
            if form == 'se3':
                self.param_dict[keys[0]].rot.mat = R
                self.param_dict[keys[0]].trans = t
            else:
                self.param_dict[keys[0]].mat = R
                val = self.param_dict[keys[1]]
                if isinstance(val, np.ndarray):
                    val[...] = t
                else:
                    self.param_dict[keys[1]] = t
            return
        lp = dev.lp
        if poses is None or len(lp.point_keys):
            poses, points = dev.get_params()
        else:
            points = ()
        for key, row in zip(lp.pose_keys, poses):
            R, t = lowering.unpack_pose(row, lp.dof)
            T = self.param_dict[key]
            T.rot.mat = R
            T.trans = t
        fast = lowering._fast_walk()
        if fast is not None and len(lp.point_keys) and type(self.param_dict) is dict and isinstance(lp.point_keys, list):
            # landmarks that are plain arrays of three doubles are written in place in C (pyslam_amd/cext/lower_fast.c: scatter3)
            todo = fast.scatter3(self.param_dict, lp.point_keys, np.ascontiguousarray(points[:len(lp.point_keys)], dtype=np.float64))
            todo = [(lp.point_keys[i], points[i]) for i in todo]
        else:
            todo = zip(lp.point_keys, points)
        for key, p in todo:
            val = self.param_dict[key]
            if isinstance(val, np.ndarray):
                val[...] = p
            else:
                self.param_dict[key] = p.copy()

    def _dx_in_reference_order(self, dev):
        xp, xl = dev.get_dx()
        lp = dev.lp
        n = max([r.stop for r in self._update_partition_dict.values()] + [0])
        dx = np.zeros(n)
        for key, rid in zip(lp.pose_keys, lp.pose_rid):
            if rid >= 0:
                dx[self._update_partition_dict[key]] = xp[rid]
        for key, vid in zip(lp.point_keys, lp.point_vid):
            if vid >= 0:
                dx[self._update_partition_dict[key]] = xl[vid]
        return dx

    # ------------------------------------------------------------------
    # landmark initialisation from several views (no reference counterpart: its cameras triangulate one observation)
    # ------------------------------------------------------------------
    def triangulate_landmarks(self, keys=None, refine_iters=5, min_parallax_deg=1.0):
        """Triangulate the landmarks `keys` (None: every non-constant landmark) on the device from their reprojection blocks
        and the CURRENT poses (constant poses included) and write the new points into the problem's parameters: a linear
        start from all views, `refine_iters` Gauss-Newton steps on the landmark's own robust cost with every pose held
        (pyslam_amd.triangulate_tables).  -> dict key -> status: 0 ok, 1 fewer than two observations and none with depth,
        2 largest angle between two viewing rays below `min_parallax_deg` and no depth, or a linear start whose normal
        equations are not positive definite, 3 the result lies behind one of its cameras.  A landmark with a non-zero
        status keeps its value.  A refinement step that does not lower the cost, or whose 3 x 3 system cannot be solved
        (not positive definite, NaN: the L1 weight at a zero residual), ends that landmark's refinement at its last accepted
        point, status 0.  Typed problems only (a block without a device kernel raises NotLowerable); a constant or unknown key raises
        KeyError."""
        dev = self._get_device()
        if self._photometric_form() or not hasattr(dev, 'triangulate'):
            raise ValueError('triangulate_landmarks: not offered on this route ({})'.format(type(dev).__name__))
        lp = dev.lp
        vid_of = {k: int(v) for k, v in zip(lp.point_keys, lp.point_vid)}
        if keys is None:
            keys = [k for k in lp.point_keys if vid_of[k] >= 0]
        else:
            keys = [keys] if isinstance(keys, str) else list(keys)
            for k in keys:
                if k not in vid_of:
                    raise KeyError('{!r} is not a landmark of this problem'.format(k))
                if vid_of[k] < 0:
                    raise KeyError('{!r} is a constant parameter: it is not triangulated'.format(k))
        pts, status = dev.triangulate([vid_of[k] for k in keys], refine_iters, min_parallax_deg, write_back=True)
        out = {}
        for k, p, s in zip(keys, pts, status):
            out[k] = int(s)
            if s == 0:
                val = self.param_dict[k]
                if isinstance(val, np.ndarray):
                    val[...] = p
                else:
                    self.param_dict[k] = p.copy()
        return out

    # ------------------------------------------------------------------
    # cost (reference problem.py:110-128)
    # ------------------------------------------------------------------
    def eval_cost(self, param_dict=None):
        try:
            dev = self._get_device(param_dict)
        except NotLowerable:
            return self._eval_cost_host(param_dict)
        return dev.eval_cost(include_all_constant=True)

    def _eval_cost_host(self, param_dict=None):
        pd = self.param_dict if param_dict is None else param_dict
        cost = 0.
        for block, keys, loss in zip(self.residual_blocks, self.block_param_keys,
                                     self.block_loss_functions):
            try:
                params = [pd[key] for key in keys]
            except KeyError as e:
                print("Parameter {} has not been initialized".format(e.args[0]))
            cost += np.sum(loss.loss(block.evaluate(params)))
        return cost

    # ------------------------------------------------------------------
    # solve (reference problem.py:130-180)
    # ------------------------------------------------------------------
    def solve(self):
        # (reference problem.py:132 rebuilds the partition here; the device path below never reads it -- it is rebuilt on first
        #  use instead: one Python statement per parameter, 0.15 s for the 500 000 landmarks of C4)
        self._partition = None
        opt = self.options
        lm = bool(getattr(opt, 'lm_adaptive', False))
        check_lm_route(opt)
        try:
            dev = self._get_device()
        except NotLowerable:
            dev = None
            check_lm_route(opt, 'the generic host path (a block without a typed kernel; see Options.hybrid_blocks)')
        self.solver_stats = []
        self.lm_history = None

        # a single pose against constant landmarks (the per-frame Problem of pipelines/sparse.py): this whole loop runs on
        # the device in one launch; identical decisions, identical cost history
        # (not under lm_adaptive: the one-launch kernel has no step rejection, a one-pose problem takes the general loop)
        fused = getattr(dev, 'motion_only_solve', None) if dev is not None and opt.fused_solve_loop and not lm else None
        if fused is not None:
            out = fused(opt, opt.linesearch_max_iters > 0)
            if out is not None:
                self._cost_history, iters, _, pose = out
                self.solver_stats = [(0, 0.0)] * iters
                self._write_back(dev, poses=pose.reshape(1, 12))      # (the call returned the pose: no second copy)
                return self.param_dict

        if dev is not None:
            self._cost_history, self.solver_stats = device_solve(dev, opt)
            if lm:
                self.lm_history = dev.lm_history
            self._write_back(dev)
            return self.param_dict

        self._cost_history, _ = _reference_loop(_HostIterations(self), opt, None, None, self._eval_cost_host(), 0., 0., 0, True, None)
        return self.param_dict

    def solve_one_iter(self):
        """One Gauss-Newton step: (step * dx, cost); parameters are NOT updated
        (reference problem.py:182-194)."""
        # the reference orders dx by the CURRENT non-constant parameters (block_cidx_dict is rebuilt on every call,
        # problem.py:294-303): recompute, a partition left by an earlier solve() may be stale after freeze / release
        self._update_partition_dict = self._get_update_partition_dict()
        opt = self.options
        try:
            dev = self._get_device()
        except NotLowerable:
            return self._solve_one_iter_host()
        if self._photometric_form():
            saved = dev.get_pose()
            dxd, cost = dev.step(opt.linesearch_max_iters > 0)
            dev.set_pose(*saved)
            dx = np.zeros(6)
            keys = self.block_param_keys[0]
            if len(keys) == 1:
                dx[self._update_partition_dict[keys[0]]] = dxd
            else:
                dx[self._update_partition_dict[keys[0]]] = dxd[3:6]
                dx[self._update_partition_dict[keys[1]]] = dxd[0:3]
            self.solver_stats.append((0, 0.0))
            return dx, cost
        saved = dev.get_params()
        dev.linearize(opt.lm_lambda)
        its, rel = dev.solve_reduced(opt.pcg_tol or 0., opt.pcg_max_iters)
        dev.backsub()
        dx = self._dx_in_reference_order(dev)
        if opt.linesearch_max_iters > 0:
            dev.apply_update(1.0)                     # the reference's search always ends at step 1
            cost = dev.eval_cost(True)
            dev.set_params(*saved)
        else:
            cost = dev.eval_cost(False)
        self.solver_stats.append((its, rel))
        return dx, cost

    # ---- generic (host-evaluated) path ---------------------------------
    # Unknowns up to which the host-evaluated path forms J dense and solves by Cholesky on the device
    # (ps_dense_normal_solve); up to 8 192 J travels as CSR and the device forms J^T J dense and factors it with the blocked
    # multi-workgroup Cholesky (ps_sparse_normal_direct, round 5); beyond that it runs CG on the normal equations
    # (ps_sparse_normal_solve) -- the reference's sparse LU has no such limits (pyslam/problem.py:186).
    DENSE_GENERIC_LIMIT = 2048

    def _host_jacobian(self):
        """IRLS-scaled J~ (scipy CSR, block-sparse: one dense (rows x dof) piece per block and parameter), e~ and cost
        by walking the blocks (reference problem.py:338-360); used only for blocks without a device kernel."""
        import scipy.sparse as sp
        part = self._update_partition_dict
        n = max([r.stop for r in part.values()] + [0])
        rows_i, cols_i, vals, es, cost, m = [], [], [], [], 0., 0
        for block, keys, loss in zip(self.residual_blocks, self.block_param_keys,
                                     self.block_loss_functions):
            params = [self.param_dict[key] for key in keys]
            want = [key not in self.constant_param_keys for key in keys]
            if not any(want):
                continue
            residual, jacobians = block.evaluate(params, want)
            residual = np.atleast_1d(residual).reshape(-1)
            s = np.sqrt(np.asarray(loss.weight(residual), dtype=float)).reshape(-1)
            nres = residual.size
            for key, jac in zip(keys, jacobians):
                if jac is not None:
                    jac = s[:, None] * np.asarray(jac, dtype=float).reshape(nres, -1)
                    c0 = part[key].start
                    rows_i.append(np.repeat(np.arange(m, m + nres), jac.shape[1]))
                    cols_i.append(np.tile(np.arange(c0, c0 + jac.shape[1]), nres))
                    vals.append(jac.ravel())
            es.append(s * residual)
            cost += np.sum(loss.loss(residual))
            m += nres
        J = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows_i), np.concatenate(cols_i))), shape=(m, n))
        J.sum_duplicates()                       # a parameter listed twice in one block: its Jacobian pieces add up
        return J, np.concatenate(es), cost

    def _generic_step(self, J, e):
        from pyslam_amd.device import dense_normal_solve, sparse_normal_solve, sparse_normal_direct, DIRECT_GENERIC_LIMIT
        if J.shape[1] <= self.DENSE_GENERIC_LIMIT:
            return dense_normal_solve(J.toarray(), e)
        if J.shape[1] <= DIRECT_GENERIC_LIMIT:
            # a direct solve, as the reference's (pyslam/problem.py:186): dense blocked Cholesky on the device + refinement.
            # Where it cannot answer -- a rank-deficient but consistent J^T J (gauge freedom, an unobserved parameter: "not positive
            # definite" / NotConverged), or 2 n^2 doubles that the device cannot allocate -- the CG on the normal equations below,
            # which converges on consistent singular systems, takes over (still on the device; round-5 ADVICE)
            from pyslam_amd.device import NotConverged
            from pyslam_amd._native import NativeError
            try:
                dx, its, rel = sparse_normal_direct(J, r=e)
                self.solver_stats.append((its, rel))
                return dx
            except (NotConverged, NativeError):
                pass
        dx, its, rel = sparse_normal_solve(J, r=e, tol=self.options.pcg_tol or 1e-12, max_iters=max(self.options.pcg_max_iters, 10 * J.shape[1]))
        self.solver_stats.append((its, rel))
        return dx

    def _solve_one_iter_host(self):
        J, e, cost = self._host_jacobian()
        dx = self._generic_step(J, e)
        if self.options.linesearch_max_iters > 0:
            test = copy.deepcopy(self.param_dict)
            for k, r in self._update_partition_dict.items():
                self._perturb_by_key(k, dx[r], test)
            cost = self._eval_cost_host(test)
        return dx, cost

    # ------------------------------------------------------------------
    # covariance (reference problem.py:196-216)
    # ------------------------------------------------------------------
    #
    # Typed problems: column k of the covariance is the solution of (J^T W J) x = e_k, computed on the
    # device by the iteration's own Schur elimination + CG + back-substitution (one call per scalar
    # unknown of the requested parameter), so blocks are available at any problem size.  The full
    # dense ``_covariance_matrix`` the reference exposes is materialised only while it is small
    # (<= DENSE_COVARIANCE_LIMIT unknowns); beyond that ``get_covariance_block`` computes columns on demand.
    DENSE_COVARIANCE_LIMIT = 1500

    def compute_covariance(self):
        try:
            self._update_partition_dict = self._get_update_partition_dict()      # (never stale: see solve_one_iter)
            self._covariance_matrix = None
            self._cov_sparse_J = None
            self._cov_device = None
            self._cov_columns = {}
            try:
                dev = self._get_device()
            except NotLowerable:
                dev = None
            if dev is None:
                from pyslam_amd.device import dense_normal_solve
                J, e, _ = self._host_jacobian()
                if J.shape[1] <= self.DENSE_GENERIC_LIMIT:
                    _, self._covariance_matrix = dense_normal_solve(J.toarray(), e, want_covariance=True)
                else:
                    self._cov_sparse_J = J           # columns on demand (get_covariance_block): CG with a unit right-hand side
                return
            if self._photometric_form():
                # 6 x 6: the device forms J~^T J~ over all pixels; its inverse in the reference's unknown order
                Hm = dev.normal_equations()[0]
                keys = self.block_param_keys[0]
                order = np.empty(6, dtype=int)
                if len(keys) == 1:
                    order[self._update_partition_dict[keys[0]]] = np.arange(6)
                else:
                    order[self._update_partition_dict[keys[0]]] = np.arange(3, 6)
                    order[self._update_partition_dict[keys[1]]] = np.arange(0, 3)
                self._covariance_matrix = np.linalg.inv(Hm[np.ix_(order, order)])
                return
            dev.covariance_begin()
            self._cov_device = dev
            # scatter maps device order -> reference ordering (vectorised: C3 has 50 000 landmarks)
            lp, part = dev.lp, self._update_partition_dict
            self._cov_where = {}
            sel = [(k, int(rid)) for k, rid in zip(lp.pose_keys, lp.pose_rid) if rid >= 0]
            for k, rid in sel:
                self._cov_where[k] = (0, rid, lp.dof)
            self._cov_pose_src = np.array([rid for _, rid in sel], dtype=np.int64)
            self._cov_pose_dst = (np.array([part[k].start for k, _ in sel], dtype=np.int64)[:, None]
                                  + np.arange(lp.dof)[None, :]).reshape(-1)
            sel = [(k, int(vid)) for k, vid in zip(lp.point_keys, lp.point_vid) if vid >= 0]
            for k, vid in sel:
                self._cov_where[k] = (1, vid, 3)
            self._cov_point_src = np.array([vid for _, vid in sel], dtype=np.int64)
            self._cov_point_dst = (np.array([part[k].start for k, _ in sel], dtype=np.int64)[:, None]
                                   + np.arange(3)[None, :]).reshape(-1)
            n = max([r.stop for r in part.values()] + [0])
            if n <= self.DENSE_COVARIANCE_LIMIT:
                cov = np.zeros((n, n))
                for key, r in part.items():
                    cov[:, r] = self._covariance_columns(key)
                self._covariance_matrix = 0.5 * (cov + cov.T)
        except Exception as e:
            print('Covariance computation failed!\n{}'.format(e))

    def _covariance_columns(self, key):
        """(n, dof_key) column block of the covariance for parameter `key`, reference ordering."""
        if key in self._cov_columns:
            return self._cov_columns[key]
        kind, index, width = self._cov_where[key]          # KeyError: constant / unknown parameter
        n = max([r.stop for r in self._update_partition_dict.values()] + [0])
        cols = np.zeros((n, width))
        for c in range(width):
            xp, xl = self._cov_device.covariance_column(kind, index, c)
            if self._cov_pose_src.size:
                cols[self._cov_pose_dst, c] = xp[self._cov_pose_src].reshape(-1)
            if self._cov_point_src.size:
                cols[self._cov_point_dst, c] = xl[self._cov_point_src].reshape(-1)
        if len(self._cov_columns) < 64:
            self._cov_columns[key] = cols
        return cols

    def get_covariance_block(self, param0, param1):
        try:
            r0 = self._update_partition_dict[param0]
            r1 = self._update_partition_dict[param1]
            if self._covariance_matrix is None and getattr(self, '_cov_sparse_J', None) is not None:
                from pyslam_amd.device import sparse_normal_solve
                J = self._cov_sparse_J
                cols = np.zeros((r0.stop - r0.start, r1.stop - r1.start))
                for c, k in enumerate(range(r1.start, r1.stop)):
                    rhs = np.zeros(J.shape[1]); rhs[k] = 1.
                    x, _, _ = sparse_normal_solve(J, rhs=rhs, tol=1e-13, max_iters=20 * J.shape[1], accept=1e-8)
                    cols[:, c] = x[r0.start:r0.stop]
                return np.squeeze(cols)
            if self._covariance_matrix is None and getattr(self, '_cov_device', None) is not None:
                return np.squeeze(self._covariance_columns(param1)[r0.start:r0.stop, :])
            return np.squeeze(self._covariance_matrix[r0.start:r0.stop, r1.start:r1.stop])
        except KeyError as e:
            print('Cannot compute covariance for constant parameter {}'.format(e.args[0]))
        return None

    # ------------------------------------------------------------------
    # batched marginal covariances (no reference counterpart: the reference inverts the whole precision matrix)
    # ------------------------------------------------------------------
    def compute_marginal_covariances(self, keys=None, pose_pairs=(), cross_pairs=()):
        """Marginal covariance blocks at the current parameters (linearised here, lambda = 0, as compute_covariance does).

        -> dict: every key of `keys` (None: every non-constant parameter) -> its (dof, dof) block, 3 x 3 for a landmark; every
        (key_a, key_b) of `pose_pairs` or `cross_pairs` -> the cross block Sigma_ab (dof_a, dof_b), oriented as
        get_covariance_block(key_a, key_b).  A constant or unknown key raises KeyError.

        Typed problems (hybrid ones included): one device call forms S^-1 of the reduced system densely in fp64 (up to
        pyslam_amd.device.COVARIANCE_MARGINALS_LIMIT reduced unknowns, else it raises) and every landmark's block from it;
        pose_pairs must then name poses, cross_pairs may name any two poses or landmarks (one more device call for all of
        them).  The photometric form slices the inverse of its 6 x 6 system, the host-evaluated generic route the dense
        covariance of dense_normal_solve (beyond DENSE_GENERIC_LIMIT: CG columns, as get_covariance_block).
        compute_covariance's state is neither read nor written."""
        part = self._get_update_partition_dict()
        want = list(part) if keys is None else list(keys)
        pairs = _check_pose_pairs(pose_pairs)
        cpairs = _check_pose_pairs(cross_pairs, 'cross_pairs')
        for k in want + [k for pr in pairs + cpairs for k in pr]:
            _check_cov_key(k, part, self.constant_param_keys)
        try:
            dev = self._get_device()
        except NotLowerable:
            dev = None
        if dev is None:
            return self._marginals_generic(part, want, pairs + cpairs)
        if self._photometric_form():
            cov = self._photometric_covariance(dev, part)
            return _slice_dense_blocks(cov, part, want, pairs + cpairs)
        dev.covariance_begin()
        pose, point = dev.covariance_marginals()
        out = marginal_blocks_by_key(dev.lp, pose, point, want)
        if pairs:
            a, b = pose_pair_indices(dev.lp, pairs)
            for pr, blk in zip(pairs, dev.covariance_pose_blocks(a, b)):
                out[pr] = blk
        if cpairs:
            ka, a, kb, b = cross_pair_indices(dev.lp, cpairs)
            out.update(cross_blocks_by_key(cpairs, ka, kb, dev.lp.dof, dev.covariance_cross_blocks(ka, a, kb, b)))
        return out

    def _photometric_covariance(self, dev, part):
        """The photometric form's 6 x 6 inverse in the reference's unknown order (as compute_covariance forms it)."""
        Hm = dev.normal_equations()[0]
        keys = self.block_param_keys[0]
        order = np.empty(6, dtype=int)
        if len(keys) == 1:
            order[part[keys[0]]] = np.arange(6)
        else:
            order[part[keys[0]]] = np.arange(3, 6)
            order[part[keys[1]]] = np.arange(0, 3)
        return np.linalg.inv(Hm[np.ix_(order, order)])

    def _marginals_generic(self, part, want, pairs):
        from pyslam_amd.device import dense_normal_solve, sparse_normal_solve
        J, e, _ = self._host_jacobian()
        if J.shape[1] <= self.DENSE_GENERIC_LIMIT:
            _, cov = dense_normal_solve(J.toarray(), e, want_covariance=True)
            return _slice_dense_blocks(cov, part, want, pairs)
        cols = {}

        def columns(key):            # (n, dof_key): one CG solve per unit right-hand side, as get_covariance_block
            if key not in cols:
                r = part[key]
                c = np.zeros((J.shape[1], r.stop - r.start))
                for q, k in enumerate(r):
                    rhs = np.zeros(J.shape[1]); rhs[k] = 1.
                    c[:, q], _, _ = sparse_normal_solve(J, rhs=rhs, tol=1e-13, max_iters=20 * J.shape[1], accept=1e-8)
                cols[key] = c
            return cols[key]
        out = {}
        for k in want:
            r = part[k]
            blk = columns(k)[r.start:r.stop]
            out[k] = 0.5 * (blk + blk.T)
        for ka, kb in pairs:
            ra = part[ka]
            out[(ka, kb)] = columns(kb)[ra.start:ra.stop].copy()
        return out

    # ------------------------------------------------------------------
    # reporting (reference problem.py:218-250; text format kept byte-identical)
    # ------------------------------------------------------------------
    def summary(self, format='brief'):
        if not self._cost_history:
            raise ValueError('solve has not yet been called')
        lm = getattr(self, 'lm_history', None)
        lm_line = '' if lm is None else '\nLM steps: {} accepted, {} rejected'.format(
            int(np.sum(lm[:, 2] != 0.)), int(np.sum(lm[:, 2] == 0.)))
        if format == 'brief':
            return 'Iterations: {:3} | Cost: {:12e} --> {:12e}'.format(
                len(self._cost_history), self._cost_history[0], self._cost_history[-1]) + lm_line
        if format == 'full':
            header = '{:>5s} | {:>12s} --> {:>12s} | {:>10s}\n'.format(
                'Iter', 'Initial cost', 'Final cost', 'Rel change')
            lines = [header, '-' * len(header) + '\n']
            for i, (ic, fc) in enumerate(zip(self._cost_history[:-1], self._cost_history[1:])):
                lines.append('{:5} | {:12e} --> {:12e} | {:+10f}\n'.format(i, ic, fc, (fc - ic) / ic))
            return ''.join(lines) + (lm_line[1:] + '\n' if lm_line else '')
        raise ValueError('Invalid summary format \'{}\'.'.format(format) +
                         'Valid formats are \'brief\' and \'full\'')

    # ------------------------------------------------------------------
    # helpers (reference problem.py:252-277, 400-409)
    # ------------------------------------------------------------------
    @property
    def _update_partition_dict(self):
        """Parameter key -> range in dx (reference problem.py:60, 132, 252-262): the reference's attribute, built when first read
        after solve() invalidated it."""
        if self._partition is None:
            self._partition = self._get_update_partition_dict()
        return self._partition

    @_update_partition_dict.setter
    def _update_partition_dict(self, value):
        self._partition = value

    def _get_update_partition_dict(self):
        out, offset = {}, 0
        for key, param in self.param_dict.items():
            if key in self.constant_param_keys:
                continue
            if hasattr(param, 'dof'):
                dof = param.dof
            elif hasattr(param, '__len__'):
                dof = len(param)
            else:
                dof = 1
            out[key] = range(offset, offset + dof)
            offset += dof
        return out

    def _perturb_by_key(self, key, dx, param_dict=None):
        pd = self.param_dict if param_dict is None else param_dict
        try:
            pd[key].perturb(dx)
        except AttributeError:
            pd[key] += dx


# ---------------------------------------------------------------------------
# batched marginals: device order -> parameter keys (pure numpy; Problem.compute_marginal_covariances)
# ---------------------------------------------------------------------------
def _check_cov_key(key, part, constant_keys):
    if key in part:
        return
    if key in constant_keys:
        raise KeyError('{!r} is a constant parameter: it has no covariance'.format(key))
    raise KeyError('{!r} is not a parameter of this problem'.format(key))


def _check_pose_pairs(pose_pairs, name='pose_pairs'):
    pairs = []
    for pr in pose_pairs:
        if isinstance(pr, (str, bytes)) or not hasattr(pr, '__len__') or len(pr) != 2:
            raise ValueError('{}: every entry must be a (key_a, key_b) pair, got {!r}'.format(name, pr))
        pairs.append((pr[0], pr[1]))
    return pairs


def marginal_blocks_by_key(lp, pose, point, keys):
    """{key: block} for `keys` from device-order marginals: pose (nr, dof, dof) indexed by lp.pose_rid, point (nv, 3, 3) by
    lp.point_vid.  A key that is a constant pose / fixed landmark of `lp`, or not in it, raises KeyError."""
    where = {}
    for k, rid in zip(lp.pose_keys, lp.pose_rid):
        where[k] = (0, int(rid))
    for k, vid in zip(lp.point_keys, lp.point_vid):
        where[k] = (1, int(vid))
    out = {}
    for k in keys:
        if k not in where:
            raise KeyError('{!r} is not a parameter of this problem'.format(k))
        kind, ix = where[k]
        if ix < 0:
            raise KeyError('{!r} is a constant parameter: it has no covariance'.format(k))
        out[k] = (pose if kind == 0 else point)[ix]
    return out


def pose_pair_indices(lp, pairs):
    """Reduced pose indices (a, b) (int32) of the (key_a, key_b) pairs; ValueError for a key that is not a variable pose."""
    rid = {k: int(r) for k, r in zip(lp.pose_keys, lp.pose_rid)}
    a, b = [], []
    for ka, kb in pairs:
        for k in (ka, kb):
            if rid.get(k, -1) < 0:
                raise ValueError('pose_pairs: {!r} is not a variable pose (cross blocks exist between poses only)'.format(k))
        a.append(rid[ka]); b.append(rid[kb])
    return np.array(a, dtype=np.int32), np.array(b, dtype=np.int32)


def cross_pair_indices(lp, pairs):
    """(kind_a, a, kind_b, b) (int32) of the (key_a, key_b) pairs for DeviceProblem.covariance_cross_blocks: kind 0 with the
    reduced pose index (rid), kind 1 with the variable landmark index (vid).  KeyError for a constant or unknown key."""
    where = {}
    for k, rid in zip(lp.pose_keys, lp.pose_rid):
        where[k] = (0, int(rid))
    for k, vid in zip(lp.point_keys, lp.point_vid):
        where[k] = (1, int(vid))
    idx = np.empty((len(pairs), 4), dtype=np.int32)
    for q, pr in enumerate(pairs):
        for s, k in enumerate(pr):
            if k not in where:
                raise KeyError('{!r} is not a parameter of this problem'.format(k))
            if where[k][1] < 0:
                raise KeyError('{!r} is a constant parameter: it has no covariance'.format(k))
            idx[q, 2 * s:2 * s + 2] = where[k]
    return tuple(np.ascontiguousarray(idx[:, c]) for c in range(4))


def cross_blocks_by_key(pairs, kind_a, kind_b, dof, blocks):
    """{(key_a, key_b): (dof_a, dof_b) block} from covariance_cross_blocks' (n, 36) rows; a landmark's dof is 3, a pose's `dof`."""
    out = {}
    for pr, ka, kb, row in zip(pairs, kind_a, kind_b, blocks):
        da, db = (dof if ka == 0 else 3), (dof if kb == 0 else 3)
        out[pr] = row[:da * db].reshape(da, db).copy()
    return out


def _slice_dense_blocks(cov, part, keys, pairs):
    """Blocks of a dense covariance in the reference's unknown order (partition `part`)."""
    out = {}
    for k in keys:
        r = part[k]
        out[k] = cov[r.start:r.stop, r.start:r.stop].copy()
    for ka, kb in pairs:
        ra, rb = part[ka], part[kb]
        out[(ka, kb)] = cov[ra.start:ra.stop, rb.start:rb.stop].copy()
    return out
