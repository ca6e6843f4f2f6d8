"""DeviceProblem: a LoweredProblem resident in HBM behind the C ABI.

Thin, stateless-on-the-host wrapper: every method maps to one ``ps_*`` entry
point of include/pyslam_hip.h.  ``Problem.solve`` (pyslam_amd/problem.py) and
bench.py drive it; multi-GPU sharding lives in pyslam_amd/distributed.py.
"""
import ctypes as C

import numpy as np

from pyslam_amd import _native as nat


# reduced unknowns (nr * dof) up to which covariance_marginals forms S^-1 densely (include/pyslam_hip.h: PS_COV_DENSE_MAX_UNKNOWNS)
COVARIANCE_MARGINALS_LIMIT = 12288


def _solve_options(o, opt, linesearch=None):
    """The fields of ps_solve_options in `o` (nat.SolveOptions, or nat.LmOptions, which begins with them) from an Options.
    `linesearch`: what the caller decided, instead of Options.linesearch_max_iters > 0.  -> o"""
    o.max_iters, o.allow_nondecreasing_steps = int(opt.max_iters), int(bool(opt.allow_nondecreasing_steps))
    o.max_nondecreasing_steps = int(opt.max_nondecreasing_steps)
    o.linesearch = int(bool(opt.linesearch_max_iters > 0 if linesearch is None else linesearch))
    o.min_update_norm, o.min_cost = float(opt.min_update_norm), float(opt.min_cost)
    o.min_cost_decrease, o.lm_lambda = float(opt.min_cost_decrease), float(getattr(opt, 'lm_lambda', 0.))
    return o


class DeviceProblem:
    def __init__(self, lp, stream=None, extra_pairs=None):
        lib = nat.require_gpu()
        self._lib = lib
        self.lp = lp
        self.dof = lp.dof
        d = nat.ProblemDesc()
        keep = []       # host arrays must outlive the create call only
        # tables a torch caller already holds in HBM (`resident_tables(lp)` below, or its own tensors) are handed over by
        # address: ps_problem_desc.flags.  All-or-nothing per class, as the C ABI has it.
        params_res = nat.is_resident(lp.poses)
        tables_res = nat.is_resident(lp.pose_rid)
        if params_res != nat.is_resident(lp.points):
            raise TypeError('poses and points must both be host arrays or both device tensors')
        d.flags = (nat.PS_DESC_DEVICE_PARAMS if params_res else 0) | (nat.PS_DESC_DEVICE_TABLES if tables_res else 0)

        def conv(a, np_dtype, want_res, to_ptr):
            if nat.is_resident(a) != want_res:
                raise TypeError('mixed host / device tables (ps_problem_desc.flags is per class: parameters, everything else)')
            if not want_res:
                a = np.ascontiguousarray(a, dtype=np_dtype)
            keep.append(a)
            return to_ptr(a) if a.shape[0] else None

        def F(a, res=None):
            return conv(a, np.float64, tables_res if res is None else res, nat.f64p)

        def I(a):
            return conv(a, np.int32, tables_res, nat.i32p)

        d.dof = lp.dof
        d.num_poses, d.poses, d.pose_rid = lp.num_poses, F(lp.poses, params_res), I(lp.pose_rid)
        d.num_points, d.points, d.point_vid = lp.num_points, F(lp.points, params_res), I(lp.point_vid)
        d.num_obs = lp.num_obs
        d.obs_pose, d.obs_point, d.obs_uvd, d.obs_grp = I(lp.obs_pose), I(lp.obs_point), F(lp.obs_uvd), I(lp.obs_grp)
        d.num_cams, d.cams = lp.cams.shape[0], F(lp.cams)
        d.num_stiff3, d.stiff3 = lp.stiff3.shape[0], F(lp.stiff3)
        d.num_obs_groups, d.obs_groups = lp.obs_groups.shape[0], F(lp.obs_groups)
        d.num_edges = lp.num_edges
        d.e_i, d.e_j, d.e_Tobs_inv, d.e_grp = I(lp.e_i), I(lp.e_j), F(lp.e_Tobs_inv), I(lp.e_grp)
        d.num_priors = lp.num_priors
        d.u_i, d.u_Tobs_inv, d.u_grp = I(lp.u_i), F(lp.u_Tobs_inv), I(lp.u_grp)
        d.num_stiffd, d.stiffd = lp.stiffd.shape[0], F(lp.stiffd)
        d.num_edge_groups, d.edge_groups = lp.edge_groups.shape[0], F(lp.edge_groups)
        if extra_pairs is not None and len(extra_pairs[0]):
            d.num_extra_pairs = len(extra_pairs[0])
            d.extra_pair_i, d.extra_pair_j = I(extra_pairs[0]), I(extra_pairs[1])
        self._h = nat.H()
        self.host = None                # hybrid.HostBlocks (attach_host): user blocks evaluated on the host
        if lp.hybrid:
            hr = nat.HostRowsDesc()
            hi, hj = np.ascontiguousarray(lp.h_i, dtype=np.int32), np.ascontiguousarray(lp.h_j, dtype=np.int32)
            keep.extend((hi, hj))
            hr.num, hr.i, hr.j = hi.shape[0], (nat.i32p(hi) if hi.shape[0] else None), (nat.i32p(hj) if hj.shape[0] else None)
            nat.check(lib.ps_problem_create_hybrid(C.byref(d), C.byref(hr), C.c_void_p(stream or 0), C.byref(self._h)))
        else:
            nat.check(lib.ps_problem_create(C.byref(d), C.c_void_p(stream or 0), C.byref(self._h)))
        info = nat.ProblemInfo()
        nat.check(lib.ps_get_info(self._h, C.byref(info)))
        self.info = {k: getattr(info, k) for k, _ in nat.ProblemInfo._fields_}
        self.nr, self.nv = info.num_reduced, info.num_var_points

    # ---- lifetime ------------------------------------------------------
    def close(self):
        if getattr(self, '_h', None):
            self._lib.ps_problem_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- user blocks on the host (Options.hybrid_blocks) ------------------
    def attach_host(self, host):
        """The user blocks of a hybrid handle (pyslam_amd/hybrid.py: HostBlocks).  From here on every linearisation uploads their
        rows at the current poses first, and every cost this object returns includes theirs."""
        if not self.lp.hybrid:
            raise ValueError('attach_host: the tables have no host rows')
        self.host = host
        self._hposes = self._read_poses()
        self.host_seconds = [0., 0.]      # (host evaluation, row upload) since attach: tools/hybrid_bench.py

    def _read_poses(self):
        poses = np.zeros((self.lp.num_poses, self.lp.pose_width))
        nat.check(self._lib.ps_get_params(self._h, nat.f64p(poses), None))
        return poses

    def set_host_rows(self, rows, cost):
        """Values of the host rows (ps_set_host_rows) and the cost of their blocks at the same point."""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        nat.check(self._lib.ps_set_host_rows(self._h, nat.f64p(rows) if rows.size else None, rows.shape[0], float(cost)))

    def _upload_host_rows(self):
        import time
        t0 = time.perf_counter()
        rows, cost = self.host.evaluate(self._hposes)
        t1 = time.perf_counter()
        self.set_host_rows(rows, cost)
        self.host_seconds[0] += t1 - t0
        self.host_seconds[1] += time.perf_counter() - t1

    # ---- hot path ------------------------------------------------------
    def eval_cost(self, include_all_constant=True):
        c = C.c_double()
        nat.check(self._lib.ps_eval_cost(self._h, int(include_all_constant), C.byref(c)))
        if self.host is not None:
            return c.value + self.host.cost(self._hposes, include_all_constant)
        return c.value

    def gn_iteration(self, lm_lambda=0., pcg_tol=1e-12, pcg_max_iters=1000, linesearch=True):
        """-> (cost, ||dx||, pcg iterations, pcg relative residual); parameters are updated."""
        if self.host is not None:
            self._upload_host_rows()
        cost, nrm, rel, it = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        nat.check(self._lib.ps_gn_iteration(self._h, lm_lambda, pcg_tol or 0., pcg_max_iters, int(linesearch),
                                            C.byref(cost), C.byref(nrm), C.byref(it), C.byref(rel)))
        c = cost.value
        if self.host is not None:
            self._hposes = self._read_poses()
            if linesearch:                # (without a line search the core returned the linearisation point's cost, rows' included)
                c += self.host.cost(self._hposes, True)
        return c, nrm.value, it.value, rel.value

    def motion_only_solve(self, opt, linesearch):
        """Problem.solve's whole loop in one launch (ps_motion_only_solve) for a one-pose motion-only problem.
        -> (cost history, iterations, last ||dx||, final pose row) or None when the problem is not of that kind (iterate
        instead)."""
        o = _solve_options(nat.SolveOptions(), opt, linesearch)
        cap = o.max_iters + 2
        if cap < 2 or cap > 238 or self.host is not None:
            return None
        hist, pose = np.zeros(cap), np.zeros(12)
        n, its, dxn = C.c_int32(), C.c_int32(), C.c_double()
        rc = self._lib.ps_motion_only_solve(self._h, C.byref(o), nat.f64p(hist), cap, C.byref(n), C.byref(its), C.byref(dxn),
                                            nat.f64p(pose))
        if rc == 1:
            return None
        nat.check(rc)
        return hist[:n.value].tolist(), its.value, dxn.value, pose

    def solve_loop(self, opt):
        """Problem.solve's loop in one C call (ps_solve).  -> (cost history, [(pcg iterations, relative residual)], [ms per
        iteration call]) or None when the core does not offer it for this handle (the caller loops itself)."""
        o = _solve_options(nat.SolveOptions(), opt)
        cap = o.max_iters + 2
        if cap < 2 or cap > 100000 or self.host is not None:
            return None
        buf = getattr(self, '_solve_buf', None)              # (result buffers kept on the object: four allocations less per solve)
        if buf is None or buf[0].size < cap:
            buf = self._solve_buf = (np.zeros(cap), np.zeros(cap), np.zeros(cap), np.zeros(cap, dtype=np.int32))
            self._solve_ptr = (nat.f64p(buf[0]), nat.f64p(buf[1]), nat.f64p(buf[2]), nat.i32p(buf[3]))
        hist, rel, ms, its = buf
        p_hist, p_rel, p_ms, p_its = self._solve_ptr
        n, iters, dxn = C.c_int32(), C.c_int32(), C.c_double()
        rc = self._lib.ps_solve(self._h, C.byref(o), float(getattr(opt, 'pcg_tol', None) or 0.), int(getattr(opt, 'pcg_max_iters', 2000)),
                                p_hist, cap, C.byref(n), C.byref(iters), C.byref(dxn), p_its, p_rel, p_ms)
        if rc == 1:
            return None
        nat.check(rc)
        k = iters.value
        return hist[:n.value].tolist(), [(int(a), float(b)) for a, b in zip(its[:k], rel[:k])], ms[:k].tolist()

    def lm_iteration(self, lm_lambda, pcg_tol=1e-12, pcg_max_iters=1000, linesearch=True):
        """gn_iteration at the damping lm_lambda that also returns the decrease its quadratic model predicted (ps_lm_iteration).
        -> (cost, ||dx||, model_decrease, pcg iterations, pcg relative residual); parameters are updated."""
        if self.host is not None:
            self._upload_host_rows()
        cost, nrm, md, rel, it = C.c_double(), C.c_double(), C.c_double(), C.c_double(), C.c_int()
        nat.check(self._lib.ps_lm_iteration(self._h, lm_lambda, pcg_tol or 0., pcg_max_iters, int(linesearch),
                                            C.byref(cost), C.byref(nrm), C.byref(md), C.byref(it), C.byref(rel)))
        c = cost.value
        if self.host is not None:
            self._hposes = self._read_poses()
            c += self.host.cost(self._hposes, True)
        return c, nrm.value, md.value, it.value, rel.value

    def solve_lm_loop(self, opt):
        """The adaptive LM loop of Problem.solve in one C call (ps_solve_lm).  -> (cost history, [(pcg iterations, relative
        residual)], [ms per iteration call], lm rows (n, 4)) or None when the core does not offer it for this handle."""
        from pyslam_amd.problem import lm_options
        o = _solve_options(nat.LmOptions(), opt)      # (the non-decreasing-step fields and lm_lambda: ps_solve_lm ignores them)
        o.lambda0, o.lambda_min, o.lambda_max = lm_options(opt)
        cap = o.max_iters + 2
        if cap < 2 or cap > 100000 or self.host is not None:
            return None
        hist, rel, ms, its, rows = np.zeros(cap), np.zeros(cap), np.zeros(cap), np.zeros(cap, dtype=np.int32), np.zeros((cap, 4))
        n, iters, dxn = C.c_int32(), C.c_int32(), C.c_double()
        rc = self._lib.ps_solve_lm(self._h, C.byref(o), float(getattr(opt, 'pcg_tol', None) or 0.), int(getattr(opt, 'pcg_max_iters', 2000)),
                                   nat.f64p(hist), cap, C.byref(n), C.byref(iters), C.byref(dxn), nat.i32p(its), nat.f64p(rel),
                                   nat.f64p(ms), nat.f64p(rows))
        if rc == 1:
            return None
        nat.check(rc)
        k = iters.value
        return (hist[:n.value].tolist(), [(int(a), float(b)) for a, b in zip(its[:k], rel[:k])], ms[:k].tolist(), rows[:k].copy())

    def gn_finish(self, linesearch=True):
        """-> (shard cost, ||dx_pose||^2, ||dx_point||^2); parameters are updated."""
        c, a, b = C.c_double(), C.c_double(), C.c_double()
        nat.check(self._lib.ps_gn_finish(self._h, int(linesearch), C.byref(c), C.byref(a), C.byref(b)))
        return c.value, a.value, b.value

    def gn_solve_finish(self, pcg_tol=1e-12, pcg_max_iters=1000, linesearch=True):
        """Reduced solve + back-substitution + update + cost with one sync.
        -> (shard cost, ||dx_pose||^2, ||dx_point||^2, pcg iterations, relative residual)."""
        c, a, b, rel, it = C.c_double(), C.c_double(), C.c_double(), C.c_double(), C.c_int()
        nat.check(self._lib.ps_gn_solve_finish(self._h, pcg_tol or 0., pcg_max_iters, int(linesearch), C.byref(c),
                                               C.byref(a), C.byref(b), C.byref(it), C.byref(rel)))
        return c.value, a.value, b.value, it.value, rel.value

    def set_collective(self, allreduce_fn_ptr, comm_ptr):
        """Native RCCL: ps_gn_iteration then performs the sharded iteration incl. both all-reduces."""
        nat.check(self._lib.ps_set_collective(self._h, C.c_void_p(allreduce_fn_ptr), C.c_void_p(comm_ptr)))

    def set_segment_exchange(self, allgather_fn_ptr, world, rank, maxlen, mine, dst, src_ptr, src_off):
        """The core's own segment exchange (include/pyslam_hip.h: ps_set_segment_exchange; plan: distributed.segment_plan)."""
        a = [np.ascontiguousarray(x, dtype=np.int64) for x in (mine, dst, src_ptr, src_off)]
        p64 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int64))
        nat.check(self._lib.ps_set_segment_exchange(self._h, C.c_void_p(allgather_fn_ptr), int(world), int(rank), int(maxlen),
                                                    int(a[0].size), p64(a[0]), int(a[1].size), p64(a[1]), p64(a[2]), p64(a[3])))

    def shard_buffer(self):
        ptr = C.c_void_p()
        nat.check(self._lib.ps_shard_buffer(self._h, C.byref(ptr)))
        return ptr.value

    def gn_solve_finish_enqueue(self, pcg_tol, pcg_max_iters, linesearch, first):
        """No host sync.  Returns True on the final (ungated) pass."""
        rc = self._lib.ps_gn_solve_finish_enqueue(self._h, pcg_tol or 0., pcg_max_iters, int(linesearch), int(first))
        if rc < 0:
            nat.check(rc)
        return rc == 1

    def gn_result(self):
        """Sync. -> (done, shard cost sum, shard ||dx_point||^2 sum, ||dx_pose||^2, iterations, relres)."""
        done, it, rel, dxp2 = C.c_int(), C.c_int(), C.c_double(), C.c_double()
        sb = (C.c_double * 2)()
        nat.check(self._lib.ps_gn_result(self._h, C.byref(done), sb, C.byref(dxp2), C.byref(it), C.byref(rel)))
        return done.value != 0, sb[0], sb[1], dxp2.value, it.value, rel.value

    def linearize(self, lm_lambda=0.):
        if self.host is not None:
            self._upload_host_rows()
        nat.check(self._lib.ps_linearize(self._h, lm_lambda))

    def solve_reduced(self, tol=1e-12, max_iters=1000):
        rel, it = C.c_double(), C.c_int()
        nat.check(self._lib.ps_solve_reduced(self._h, tol or 0., max_iters, C.byref(it), C.byref(rel)))
        return it.value, rel.value

    def backsub(self):
        nat.check(self._lib.ps_backsub(self._h))

    def apply_update(self, step=1.0):
        nat.check(self._lib.ps_apply_update(self._h, step))
        if self.host is not None:
            self._hposes = self._read_poses()

    def step_norm(self):
        n2 = C.c_double()
        nat.check(self._lib.ps_step_norm2(self._h, C.byref(n2)))
        return float(np.sqrt(n2.value))

    def snapshot(self):
        nat.check(self._lib.ps_snapshot_params(self._h))

    def restore(self):
        nat.check(self._lib.ps_restore_params(self._h))
        if self.host is not None:
            self._hposes = self._read_poses()

    def reset_solver_state(self):
        """A new solve starts here: nothing the solver carried over from earlier calls is used (ps_reset_solver_state)."""
        nat.check(self._lib.ps_reset_solver_state(self._h))

    def set_solve_horizon(self, n):
        """Further iterations the caller's stopping rule allows if the coming step is non-decreasing (-1: unknown)."""
        nat.check(self._lib.ps_set_option(self._h, b'solve_horizon', float(n)))

    def set_expect_next(self, flag):
        """The caller's loop will call gn_iteration again after the coming call unless a stopping rule on ||dx|| or the cost
        fires (what ps_solve tells the core about its own loop): the coming call's tail then runs the NEXT linearisation's
        landmark pass in place of its cost pass -- one evaluation of every observation instead of two."""
        nat.check(self._lib.ps_set_option(self._h, b'expect_next', 1.0 if flag else 0.0))

    # ---- covariance by columns (reference problem.py:196-216) ------------
    def covariance_begin(self):
        """Linearise at the current parameters and prepare the reduced solver."""
        if self.host is not None:
            self._upload_host_rows()
        nat.check(self._lib.ps_covariance_begin(self._h))

    def covariance_column(self, kind, index, comp, tol=1e-13, max_iters=4000):
        """Column of the covariance (J^T W J)^-1 for component `comp` of reduced pose `index`
        (kind 0) or variable landmark `index` (kind 1): (pose part (nr, dof), point part (nv, 3))."""
        rel, it = C.c_double(), C.c_int()
        nat.check(self._lib.ps_covariance_column(self._h, int(kind), int(index), int(comp), tol, max_iters,
                                                 C.byref(it), C.byref(rel)))
        return self.get_dx()

    # ---- batched marginals (ps_covariance_marginals) ---------------------
    def covariance_marginals(self):
        """Marginal covariances after covariance_begin(): (pose (nr, dof, dof), point (nv, 3, 3)) in device order (reduced pose
        rid, variable landmark vid).  The dense Sigma_pp = S^-1 they come from stays on the handle for covariance_pose_blocks.
        Reduced systems above COVARIANCE_MARGINALS_LIMIT unknowns raise (the column route has no limit)."""
        pose = np.zeros((self.nr, self.dof, self.dof))
        point = np.zeros((self.nv, 3, 3))
        nat.check(self._lib.ps_covariance_marginals(self._h, nat.f64p(pose), nat.f64p(point)))
        return pose, point

    def covariance_pose_blocks(self, a, b):
        """Sigma_pp[a_k, b_k] (len(a), dof, dof) for reduced pose indices a, b, from the inverse covariance_marginals() left."""
        a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
        b = np.ascontiguousarray(b, dtype=np.int32).reshape(-1)
        if a.shape != b.shape:
            raise ValueError('covariance_pose_blocks: a and b differ in length')
        out = np.zeros((a.shape[0], self.dof, self.dof))
        nat.check(self._lib.ps_covariance_pose_blocks(self._h, a.shape[0], nat.i32p(a), nat.i32p(b), nat.f64p(out)))
        return out

    def covariance_cross_blocks(self, kind_a, a, kind_b, b):
        """Sigma[(kind_a_k, a_k), (kind_b_k, b_k)] (len(a), 36) from the inverse covariance_marginals() left: kind 0 a reduced
        pose index (rid), 1 a variable landmark index (vid); block k row-major (dof_a, dof_b) in the leading entries of row k,
        the rest zero."""
        arrs = [np.ascontiguousarray(x, dtype=np.int32).reshape(-1) for x in (kind_a, a, kind_b, b)]
        if any(x.shape != arrs[0].shape for x in arrs):
            raise ValueError('covariance_cross_blocks: kind_a, a, kind_b and b differ in length')
        out = np.zeros((arrs[0].shape[0], 36))
        nat.check(self._lib.ps_covariance_cross_blocks(self._h, arrs[0].shape[0], *[nat.i32p(x) for x in arrs], nat.f64p(out)))
        return out

    # ---- multi-view triangulation (ps_triangulate) -----------------------
    def triangulate(self, vids=None, refine_iters=5, min_parallax_deg=1.0, write_back=True):
        """Variable landmarks `vids` (None: all, in vid order) from their observations and the current poses: linear start,
        `refine_iters` Gauss-Newton steps on the landmark's own cost, status per landmark (include/pyslam_hip.h:
        ps_triangulate).  -> (points (n, 3), status (n,) int32); with `write_back` the points with status 0 replace the
        handle's."""
        if vids is not None:
            vids = np.ascontiguousarray(vids, dtype=np.int32).reshape(-1)
        n = self.nv if vids is None else vids.shape[0]
        pts, status = np.zeros((n, 3)), np.zeros(n, dtype=np.int32)
        if n:
            nat.check(self._lib.ps_triangulate(self._h, n, nat.i32p(vids) if vids is not None else None, int(refine_iters),
                                               float(min_parallax_deg), int(bool(write_back)), nat.f64p(pts), nat.i32p(status)))
        return pts, status

    # ---- data movement -------------------------------------------------
    def get_dx(self):
        """(dx_pose (nr, dof), dx_point (nv, 3)) in device order."""
        xp = np.zeros((self.nr, self.dof))
        xl = np.zeros((self.nv, 3))
        nat.check(self._lib.ps_get_dx(self._h, nat.f64p(xp), nat.f64p(xl)))
        return xp, xl

    def get_params(self, poses_out=None, points_out=None):
        """Without arguments: fresh host arrays.  With torch tensors resident in HBM: filled in place, device to device."""
        if poses_out is not None or points_out is not None:
            nat.check(self._lib.ps_get_params(self._h, nat.f64p(poses_out), nat.f64p(points_out)))
            return poses_out, points_out
        poses = np.zeros((self.lp.num_poses, self.lp.pose_width))
        points = np.zeros((self.lp.num_points, 3))
        nat.check(self._lib.ps_get_params(self._h, nat.f64p(poses), nat.f64p(points)))
        return poses, points

    def set_params(self, poses=None, points=None):
        """Host arrays, or float64 torch tensors resident in HBM (copied device to device)."""
        p = poses if poses is None or nat.is_resident(poses) else np.ascontiguousarray(poses, dtype=np.float64)
        q = points if points is None or nat.is_resident(points) else np.ascontiguousarray(points, dtype=np.float64)
        nat.check(self._lib.ps_set_params(self._h, nat.f64p(p), nat.f64p(q)))
        if self.host is not None and poses is not None:
            self._hposes = self._read_poses()

    def reduce_buffer(self):
        """(device pointer, number of doubles) of the exchange buffer [upper(S) | g | cost | flag] the
        multi-GPU driver all-reduces between shard_pack() and shard_unpack()."""
        ptr, n = C.c_void_p(), C.c_int64()
        nat.check(self._lib.ps_reduce_buffer(self._h, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def shard_pack(self):
        nat.check(self._lib.ps_shard_pack(self._h))

    def shard_unpack(self):
        nat.check(self._lib.ps_shard_unpack(self._h))

    # ---- parity taps ---------------------------------------------------
    def reduced_system(self):
        """BSR (row_ptr, col_idx, vals (nnzb, d, d), g (nr*d,))."""
        nnzb, d = self.info['reduced_nnzb'], self.dof
        rp = np.zeros(self.nr + 1, dtype=np.int32)
        ci = np.zeros(max(nnzb, 1), dtype=np.int32)
        vals = np.zeros((max(nnzb, 1), d, d))
        g = np.zeros(max(self.nr * d, 1))
        nat.check(self._lib.ps_get_reduced_system(self._h, nat.i32p(rp), nat.i32p(ci), nat.f64p(vals), nat.f64p(g)))
        return rp, ci[:nnzb], vals[:nnzb], g[:self.nr * d]

    def reduced_dense(self):
        rp, ci, vals, g = self.reduced_system()
        d, n = self.dof, self.nr * self.dof
        S = np.zeros((n, n))
        for r in range(self.nr):
            for k in range(rp[r], rp[r + 1]):
                S[r * d:(r + 1) * d, ci[k] * d:(ci[k] + 1) * d] = vals[k]
        return S, g

    def landmark_factors(self):
        cinv, c = np.zeros((self.nv, 6)), np.zeros((self.nv, 3))
        nat.check(self._lib.ps_get_landmark_factors(self._h, nat.f64p(cinv), nat.f64p(c)))
        return cinv, c

    def packed_runs(self):
        """(run (nwaves, 4) = {v0, v1, row0, nrows}, first (nwaves + 1), lm_ptr (nv + 1), the back-substitution's partials of
        ||dx_point||^2 (ceil(nwaves / 4))) of the packed observation passes as the handle holds them (include/pyslam_hip.h:
        ps_debug_packed_runs); nwaves = 0: the handle keeps the 16-lane kernels."""
        nw = C.c_int32(0)
        nat.check(self._lib.ps_debug_packed_runs(self._h, C.byref(nw), 0, None, None, None, None))
        n = nw.value
        run, first, lm_ptr = np.zeros((n, 4), dtype=np.int32), np.zeros(n + 1, dtype=np.int32), np.zeros(self.nv + 1, dtype=np.int32)
        sq = np.zeros((n + 3) // 4)
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        nat.check(self._lib.ps_debug_packed_runs(self._h, C.byref(nw), n, i32(run), i32(first), i32(lm_ptr), nat.f64p(sq)))
        return run, first, lm_ptr, sq

    def pose_items(self):
        """(items (nitems, 3) = {reduced pose, first row, one past the last row}, partial (nitems, 33)) of the pose pass as the
        handle holds them after its last launch (include/pyslam_hip.h: ps_debug_pose_items)."""
        ni = C.c_int32(0)
        nat.check(self._lib.ps_debug_pose_items(self._h, C.byref(ni), 0, None, None))
        n = ni.value
        items, partial = np.zeros((n, 3), dtype=np.int32), np.zeros((n, 33))
        nat.check(self._lib.ps_debug_pose_items(self._h, C.byref(ni), n, items.ctypes.data_as(C.POINTER(C.c_int32)), nat.f64p(partial)))
        return items, partial

    def debug_reproj_blocks(self):
        n = self.lp.num_obs
        r, jp, jl = np.zeros((n, 3)), np.zeros((n, 3, 6)), np.zeros((n, 3, 3))
        nat.check(self._lib.ps_debug_reproj_blocks(self._h, nat.f64p(r), nat.f64p(jp), nat.f64p(jl)))
        return r, jp, jl

    def debug_factor_blocks(self):
        """(r~, J~_1, J~_2) of every pose-pose edge, then every prior, from the production factor kernel."""
        f, d = self.lp.num_edges + self.lp.num_priors, self.lp.dof
        r, j1, j2 = np.zeros((f, d)), np.zeros((f, d, d)), np.zeros((f, d, d))
        nat.check(self._lib.ps_debug_factor_blocks(self._h, nat.f64p(r), nat.f64p(j1), nat.f64p(j2)))
        return r, j1, j2

    def debug_ldi_state(self):
        """State record of the lagged dense inverse (include/pyslam_hip.h: ps_debug_ldi_read, PS_LDI_READ_STATE)."""
        rec = np.zeros(12)
        nat.check(self._lib.ps_debug_ldi_read(self._h, 0, nat.f64p(rec), rec.size))
        keys = ('state', 'cur', 'n', 'np', 'kp', 'direct', 'fro_limit', 'last_its', 'seed_steps', 'nr', 'dof', 'ready')
        return {k: (float(v) if k == 'fro_limit' else int(v)) for k, v in zip(keys, rec)}

    def debug_ldi_read(self, what):
        """One item of the lagged dense inverse as float64 (the fp32 matrices convert exactly): 'S32', 'X32', 'Xu', 'Xt',
        'Linv', 'coef', 'fro', 'r', 'z' (ps_debug_ldi_read).  Raises until an inverse has been seeded."""
        s = self.debug_ldi_state()
        n, npad, kp, nr, d = s['n'], s['np'], s['kp'], s['nr'], s['dof']
        code, shape = {'S32': (1, (npad, npad)), 'X32': (2, (npad, npad)), 'Xu': (3, (npad, npad)), 'Xt': (4, (npad, kp)),
                       'Linv': (5, (nr, d, d)), 'coef': (6, (3,)), 'fro': (7, (1,)), 'r': (8, (n,)), 'z': (9, (n,))}[what]
        out = np.zeros(max(int(np.prod(shape)), 1))
        nat.check(self._lib.ps_debug_ldi_read(self._h, code, nat.f64p(out), out.size))
        return out[:int(np.prod(shape))].reshape(shape)

    def get_info(self):
        """ps_problem_info as a dict, read now (sizes, and the solver counters: restarts, launches, lagged-inverse and
        one-launch-PCG statistics)."""
        info = nat.ProblemInfo()
        nat.check(self._lib.ps_get_info(self._h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in nat.ProblemInfo._fields_}

    def cg_restarts(self):
        """Restarts of the pipelined CG so far (ps_problem_info.cg_restarts)."""
        info = nat.ProblemInfo()
        nat.check(self._lib.ps_get_info(self._h, C.byref(info)))
        return int(info.cg_restarts)

    def cg_kernel_launches(self):
        """Kernels enqueued for iterations of the reduced solve so far (ps_problem_info.cg_kernel_launches)."""
        info = nat.ProblemInfo()
        nat.check(self._lib.ps_get_info(self._h, C.byref(info)))
        return int(info.cg_kernel_launches)

    def cg_persist_counts(self):
        """(folded CG solves run in one launch, of which timed out and were solved again launch by launch) --
        ps_problem_info.cg_persist_solves / cg_persist_failures (csrc/ps_k_cg_persist.h)."""
        info = nat.ProblemInfo()
        nat.check(self._lib.ps_get_info(self._h, C.byref(info)))
        return int(info.cg_persist_solves), int(info.cg_persist_failures)

    def cg_persist_recover_counts(self):
        """(one-launch folded CG launches that recover x inside the launch, launches that leave it to the gated k_coarse_recover
        behind them) -- ps_get_option "cg_persist_recovered" / "cg_persist_recover_fallbacks" (option "cg_persist_recover")."""
        return int(self.get_option('cg_persist_recovered')), int(self.get_option('cg_persist_recover_fallbacks'))

    def set_option(self, name, value):
        nat.check(self._lib.ps_set_option(self._h, name.encode(), float(value)))

    def get_option(self, name):
        """What an option comes to on this handle (ps_get_option: the launch gates and their counters)."""
        v = C.c_double()
        nat.check(self._lib.ps_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    # ---- tracing -------------------------------------------------------
    def set_profiling(self, level=2):
        """0 off; 1 = hipEvents around the whole iteration and the Schur kernel only (cheap);
        2 = around every stage (adds ~10 event records per iteration)."""
        nat.check(self._lib.ps_set_profiling(self._h, int(level)))

    def stage_times(self, reset=False):
        ms = (C.c_double * nat.PS_NUM_STAGES)()
        cnt = (C.c_int64 * nat.PS_NUM_STAGES)()
        nat.check(self._lib.ps_get_stage_times(self._h, ms, cnt, int(reset)))
        return {n: (ms[i], cnt[i]) for i, n in enumerate(nat.STAGE_NAMES)}


def dense_normal_solve(J, r, want_covariance=False):
    """Host-evaluated generic path: dx = (J^T J)^-1 (-J^T r) on the device."""
    lib = nat.require_gpu()
    J = np.ascontiguousarray(J, dtype=np.float64)
    r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
    m, n = J.shape
    dx = np.zeros(n)
    cov = np.zeros((n, n)) if want_covariance else None
    nat.check(lib.ps_dense_normal_solve(nat.f64p(J), nat.f64p(r), m, n, nat.f64p(dx), nat.f64p(cov)))
    return (dx, cov) if want_covariance else dx


def band_inverse(A, ncb, dof, bw, chunk_nodes=0):
    """Inverse (fp32) of a symmetric positive definite block-banded matrix by the coarse level's factorisation kernels
    (include/pyslam_hip.h: ps_debug_band_inverse): chunk_nodes < 0 the serial column walk, 0 / > 0 the partitioned form.
    -> (inverse, GPU microseconds of the launches)."""
    lib = nat.require_gpu()
    A = np.ascontiguousarray(A, dtype=np.float64)
    n = ncb * dof
    assert A.shape == (n, n)
    out = np.zeros((n, n), dtype=np.float32)
    us = C.c_double(0.0)
    nat.check(lib.ps_debug_band_inverse(nat.f64p(A), ncb, dof, bw, chunk_nodes, out.ctypes.data_as(C.POINTER(C.c_float)),
                                        C.cast(C.byref(us), nat.c_f64p)))
    return out, us.value


def coarse_chol(A, ncb, dof, bw, variant, timed=False):
    """One launch of an LDS-resident coarse factorisation kernel on a host matrix (include/pyslam_hip.h: ps_debug_coarse_chol):
    variant 0 k_coarse_chol, 1 k_coarse_chol_band as the solver launches it, 64 .. 1024 the band kernel with that many threads.
    -> (Li, LiT, status words, GPU microseconds or None)."""
    lib = nat.require_gpu()
    A = np.ascontiguousarray(A, dtype=np.float64)
    n = ncb * dof
    assert A.shape == (n, n)
    Li, LiT, status = np.zeros((n, n)), np.zeros((n, n)), np.zeros(8, dtype=np.int32)
    us = C.c_double(0.0)
    nat.check(lib.ps_debug_coarse_chol(nat.f64p(A), ncb, dof, bw, variant, nat.f64p(Li), nat.f64p(LiT),
                                       status.ctypes.data_as(nat.c_i32p), C.cast(C.byref(us), nat.c_f64p) if timed else None))
    return Li, LiT, status, (us.value if timed else None)


def coarse_chol_clocks(A, ncb, dof, bw, variant):
    """Phase stamps of that launch in microseconds from kernel entry (measurement build: ps_debug_coarse_chol_clocks):
    entry, loaded, factor loop, diagonal inverses, doubling levels, stored."""
    lib = nat.require_gpu()
    A = np.ascontiguousarray(A, dtype=np.float64)
    assert A.shape == (ncb * dof, ncb * dof)
    clocks = np.zeros(6)
    nat.check(lib.ps_debug_coarse_chol_clocks(nat.f64p(A), ncb, dof, bw, variant, nat.f64p(clocks)))
    return clocks


def dense_factor(A, dense_out=False, ld_extra=0, ainv_fill=0.0):
    """Every stage of the blocked dense factorisation chain on a host matrix (include/pyslam_hip.h: ps_debug_dense_factor).
    -> dict: L (working matrix), Tinv (steps x 24 x 24), Li, LiT, ainv (n x (n + ld_extra) float32, pre-filled with ainv_fill),
    diag_fail, us."""
    lib = nat.require_gpu()
    A = np.ascontiguousarray(A, dtype=np.float64)
    n = A.shape[0]
    assert A.shape == (n, n) and 0 <= ld_extra < 256
    steps = (n + 23) // 24
    out = dict(L=np.zeros((n, n)), Tinv=np.zeros((steps, 24, 24)), Li=np.zeros((n, n)), LiT=np.zeros((n, n)),
               ainv=np.full((n, n + ld_extra), ainv_fill, dtype=np.float32))
    fail, us = C.c_int32(-1), C.c_double(0.0)
    nat.check(lib.ps_debug_dense_factor(nat.f64p(A), n, (1 if dense_out else 0) | (ld_extra << 8), nat.f64p(out['L']), nat.f64p(out['Tinv']),
                                        nat.f64p(out['Li']), nat.f64p(out['LiT']), out['ainv'].ctypes.data_as(C.POINTER(C.c_float)),
                                        C.byref(fail), C.cast(C.byref(us), nat.c_f64p)))
    out['diag_fail'], out['us'] = int(fail.value), us.value
    return out


def bchol_slab(m, w, block):
    """(row_lo, row_hi, entries, grid) of workgroup `block` of k_bchol_panel on a panel of m rows x w columns (ps_debug_bchol_slab:
    host only, no GPU needed)."""
    lib = nat.load()
    v = [C.c_int32() for _ in range(4)]
    nat.check(lib.ps_debug_bchol_slab(m, w, block, *[C.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def factor_stress(A, ncb, dof, bw, mode, launches, lowprio=0, aggressor=0):
    """(n_diff, n_pivot) of ps_debug_factor_stress: `launches` runs of a factorisation family beside an aggressor, each output
    compared bit for bit with an idle run."""
    lib = nat.require_gpu()
    A = np.ascontiguousarray(A, dtype=np.float64)
    assert A.shape == (ncb * dof, ncb * dof)
    nd, npv = C.c_int32(), C.c_int32()
    nat.check(lib.ps_debug_factor_stress(nat.f64p(A), ncb, dof, bw, mode, launches, lowprio, aggressor, C.byref(nd), C.byref(npv)))
    return int(nd.value), int(npv.value)


def ldi_gemm(A, B, C0, M, N, K, alpha=1.0, beta=0.0, Dm=None, gamma=0.0, lda=None, ldb=None, ldd=None, ldc=None, krange=None,
             upper_only=False, dev_scale=None, fro_sentinel=None, need_gpu=True):
    """C = alpha A B + beta Dm + gamma I by the lagged inverse's fp32 MFMA product (include/pyslam_hip.h: ps_debug_ldi_gemm).
    A, B, C0 (and Dm): contiguous float32 arrays of M x lda, K x ldb, M x ldc (M x ldd); Dm may be the object A itself (the device
    copies alias then).  -> (C, fro_part or None); fro_part is asked for by giving fro_sentinel."""
    lib = nat.require_gpu() if need_gpu else nat.load()
    f32p = C.POINTER(C.c_float)
    lda, ldb, ldc = lda or K, ldb or N, ldc or N
    ldd = ldd or (lda if Dm is A else N)
    for a in (A, B, C0) + (() if Dm is None else (Dm,)):
        assert a.dtype == np.float32 and a.flags.c_contiguous
    out = C0.copy()
    mt, nt = max(M // 32, 1), max(N // 32, 1)
    fro = None if fro_sentinel is None else np.zeros((mt, nt))
    kr = None if krange is None else np.ascontiguousarray(krange, dtype=np.int32).reshape(-1)
    sc = None if dev_scale is None else np.array([dev_scale], dtype=np.float32)
    nat.check(lib.ps_debug_ldi_gemm(M, N, K, alpha, A.ctypes.data_as(f32p), lda, B.ctypes.data_as(f32p), ldb, beta,
                                    None if Dm is None else Dm.ctypes.data_as(f32p), ldd, gamma, out.ctypes.data_as(f32p), ldc,
                                    nat.i32p(kr), int(bool(upper_only)), None if sc is None else sc.ctypes.data_as(f32p),
                                    0.0 if fro_sentinel is None else float(fro_sentinel), nat.f64p(fro)))
    return out, fro


def ldi_ritz(rz, alpha, m=None):
    """(c, ritz_min, ritz_max) as float32 from the seed-scale kernel k_ldi_ritz on a CG's coefficients (ps_debug_ldi_ritz)."""
    lib = nat.require_gpu()
    rz = np.ascontiguousarray(rz, dtype=np.float64)
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    m = min(rz.size, alpha.size) if m is None else m
    assert m <= rz.size and m <= alpha.size
    out = np.full(3, -1.0, dtype=np.float32)
    nat.check(lib.ps_debug_ldi_ritz(nat.f64p(rz), nat.f64p(alpha), m, out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


class NotConverged(nat.NativeError):
    """The CG of the host-evaluated path stopped at max_iters with a residual too large to use."""


def sparse_normal_solve(J, r=None, rhs=None, tol=1e-12, max_iters=10000, accept=1e-6):
    """Host-evaluated generic path beyond the dense solver: (J^T J) dx = -J^T r (or = rhs) by CG on the device with J
    (scipy CSR) resident in HBM.  -> (dx, iterations, relative preconditioned residual).

    The reference solves these systems with a sparse LU (pyslam/problem.py:186), which does not care about the
    condition number; Jacobi-preconditioned CG on J^T J does (it squares it).  So the outcome is checked: a solve
    that ran out of iterations with a relative residual above `accept` raises NotConverged (an unconverged step or
    covariance column must not be used silently -- round-2 ADVICE), one that ended between `tol` and `accept` warns."""
    lib = nat.require_gpu()
    J = J.tocsr()
    J.sort_indices()
    Jt = J.T.tocsr()
    Jt.sort_indices()
    m, n = J.shape
    a = [np.ascontiguousarray(x, dtype=t) for x, t in ((J.indptr, np.int32), (J.indices, np.int32), (J.data, np.float64),
                                                        (Jt.indptr, np.int32), (Jt.indices, np.int32), (Jt.data, np.float64))]
    rr = None if r is None else np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
    bb = None if rhs is None else np.ascontiguousarray(rhs, dtype=np.float64).reshape(-1)
    dx = np.zeros(n)
    its, rel = C.c_int32(), C.c_double()
    nat.check(lib.ps_sparse_normal_solve(m, n, nat.i32p(a[0]), nat.i32p(a[1]), nat.f64p(a[2]), nat.i32p(a[3]), nat.i32p(a[4]),
                                         nat.f64p(a[5]), nat.f64p(rr), nat.f64p(bb), float(tol), int(max_iters), nat.f64p(dx),
                                         C.byref(its), C.byref(rel)))
    relres = float(rel.value)
    if not (relres <= max(accept, tol)):
        raise NotConverged('sparse normal equations ({} unknowns): CG stopped after {} iterations at a relative residual of '
                           '{:.2e} (tolerance {:.1e}); the system is too ill-conditioned for Jacobi-preconditioned CG on '
                           'J^T J -- rescale the parameters / stiffnesses, or hold enough parameters constant for the '
                           'dense path (<= 2048 unknowns)'.format(n, int(its.value), relres, tol))
    if relres > 10. * tol:
        import warnings
        warnings.warn('pyslam_amd: sparse normal equations solved to a relative residual of {:.2e} only (tolerance {:.1e}, '
                      '{} iterations)'.format(relres, tol, int(its.value)), RuntimeWarning)
    return dx, int(its.value), relres


DIRECT_GENERIC_LIMIT = 8192       # csrc/ps_sparse.h: PS_SPD_MAXN


def sparse_normal_direct(J, r=None, rhs=None, refine_steps=3, accept=1e-8):
    """Host-evaluated generic path, 2 049 .. 8 192 unknowns (round 5): (J^T J) dx = -J^T r (or = rhs) by a dense blocked
    Cholesky on the device + refinement on the residual of the original system (include/pyslam_hip.h:
    ps_sparse_normal_direct) -- what the reference's sparse LU (pyslam/problem.py:186) is replaced by where the CG of
    sparse_normal_solve would not converge.  -> (dx, refinement steps allowed, ||rhs - J^T J dx|| / ||rhs||).
    Raises NotConverged if the residual stays above `accept` (a normal matrix singular to rounding)."""
    lib = nat.require_gpu()
    J = J.tocsr(copy=True)
    J.sum_duplicates()                # (the device looks entries up by binary search: one entry per (row, column))
    J.sort_indices()
    Jt = J.T.tocsr()
    Jt.sort_indices()
    m, n = J.shape
    a = [np.ascontiguousarray(x, dtype=t) for x, t in ((J.indptr, np.int32), (J.indices, np.int32), (J.data, np.float64),
                                                        (Jt.indptr, np.int32), (Jt.indices, np.int32), (Jt.data, np.float64))]
    rr = None if r is None else np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
    bb = None if rhs is None else np.ascontiguousarray(rhs, dtype=np.float64).reshape(-1)
    dx = np.zeros(n)
    rel = C.c_double()
    nat.check(lib.ps_sparse_normal_direct(m, n, nat.i32p(a[0]), nat.i32p(a[1]), nat.f64p(a[2]), nat.i32p(a[3]), nat.i32p(a[4]),
                                          nat.f64p(a[5]), nat.f64p(rr), nat.f64p(bb), int(refine_steps), nat.f64p(dx),
                                          C.cast(C.byref(rel), nat.c_f64p)))
    relres = float(rel.value)
    if not (relres <= accept):
        raise NotConverged('dense direct solve of the normal equations ({} unknowns): relative residual {:.2e} after {} refinement '
                           'steps -- J^T J is singular to rounding'.format(n, relres, refine_steps))
    return dx, int(refine_steps), relres


class PhotometricDevice:
    """Device side of a Problem whose only block is a PhotometricResidualSE3 (include/pyslam_hip.h:
    ps_photometric_*): the pixel tables live in HBM, one call runs a whole Gauss-Newton iteration.
    Exposes the subset of DeviceProblem's interface that Problem.solve() drives."""

    def __init__(self, block, loss, split_params, stream=None):
        from pyslam_amd.lowering import _loss_id_k
        lib = nat.require_gpu()
        self._lib = lib
        self.split_params = bool(split_params)
        t = block.device_tables()
        d = nat.PhotoDesc()
        self._keep = t
        d.num_pixels = t['pt_ref'].shape[0]
        d.pt_ref, d.im_ref = nat.f64p(t['pt_ref']), nat.f64p(t['im_ref'])
        d.im_jac, d.tri_jac_d = nat.f64p(t['im_jac']), nat.f64p(t['tri_jac_d'])
        d.height, d.width = t['im_track'].shape
        d.im_track = nat.f64p(t['im_track'])
        for k in range(5):
            d.cam[k] = t['cam'][k]
        d.cam_type, d.cam_w, d.cam_h = t['cam_type'], t['cam_w'], t['cam_h']
        d.intensity_covar, d.depth_covar = t['intensity_covar'], t['depth_covar']
        lid, lk = _loss_id_k(loss)
        d.loss_id, d.loss_k = int(lid), float(lk)
        self.num_pixels = d.num_pixels
        self._h = nat.H()
        nat.check(lib.ps_photometric_create(C.byref(d), C.c_void_p(stream or 0), C.byref(self._h)))
        self._keep = None
        self._saved = None

    def close(self):
        if getattr(self, '_h', None):
            self._lib.ps_photometric_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- pose: (R, t) <-> 12 doubles -----------------------------------
    def set_pose(self, R, t):
        row = np.concatenate([np.asarray(R, dtype=float).reshape(9), np.asarray(t, dtype=float).reshape(3)])
        nat.check(self._lib.ps_photometric_set_pose(self._h, nat.f64p(row)))

    def get_pose(self):
        row = np.zeros(12)
        nat.check(self._lib.ps_photometric_get_pose(self._h, nat.f64p(row)))
        return row[:9].reshape(3, 3).copy(), row[9:].copy()

    def snapshot(self):
        self._saved = self.get_pose()

    def restore(self):
        self.set_pose(*self._saved)

    # ---- evaluation ----------------------------------------------------
    def eval_cost(self, include_all_constant=True):
        cost, n = C.c_double(), C.c_int64()
        nat.check(self._lib.ps_photometric_eval_cost(self._h, C.byref(cost), C.byref(n)))
        self.num_valid = n.value
        return cost.value

    def normal_equations(self):
        Hm, b = np.zeros((6, 6)), np.zeros(6)
        cost, n = C.c_double(), C.c_int64()
        nat.check(self._lib.ps_photometric_normal_equations(self._h, nat.f64p(Hm), nat.f64p(b), C.byref(cost), C.byref(n)))
        return Hm, b, cost.value, n.value

    def step(self, linesearch):
        """One iteration in place: (dx in [translation; rotation] order, cost)."""
        dx, cost = np.zeros(6), C.c_double()
        nat.check(self._lib.ps_photometric_iteration(self._h, int(self.split_params), int(bool(linesearch)),
                                                     nat.f64p(dx), C.byref(cost)))
        return dx, cost.value

    def gn_iteration(self, lam, pcg_tol, pcg_max_iters, linesearch):
        """Same tuple as DeviceProblem.gn_iteration: (cost, |dx|, solver iterations, relative residual)."""
        if lam:
            raise ValueError('the photometric device path has no damping (Options.lm_lambda must be 0)')
        dx, cost = self.step(linesearch)
        return cost, float(np.linalg.norm(dx)), 0, 0.0



class DenseTracker:
    """Device side of the dense RGB-D VO pipeline (include/pyslam_hip.h: ps_dense_*; pyslam_amd/pipelines/dense.py drives
    it): a fixed number of frame slots, each with its image pyramid, gradient and depth levels and per-level pixel tables,
    and the coarse-to-fine solve of one frame in one call.  Device memory is fixed at construction."""

    def __init__(self, levels, height, width, num_slots=3, stream=None):
        lib = nat.require_gpu()
        self._lib = lib
        self.levels, self.height, self.width, self.num_slots = int(levels), int(height), int(width), int(num_slots)
        self._pending = []          # host buffers of uploads not yet synchronised (ps_dense_upload does not wait)
        self._h = nat.H()
        nat.check(lib.ps_dense_create(self.levels, self.height, self.width, self.num_slots, C.c_void_p(stream or 0),
                                      C.byref(self._h)))

    def close(self):
        if getattr(self, '_h', None):
            self._lib.ps_dense_destroy(self._h)
            self._h = None
        self._pending = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def level_shape(self, level):
        h, w = C.c_int32(), C.c_int32()
        nat.check(self._lib.ps_dense_level_shape(self._h, int(level), C.byref(h), C.byref(w)))
        return h.value, w.value

    def upload(self, slot, image=None, depth=None):
        """Image (uint8 or float64, height x width) and / or depth (float64) into `slot`; an image rebuilds the pyramid."""
        img = None
        if image is not None:
            img = np.asarray(image)
            if img.dtype not in (np.uint8, np.float64):
                raise TypeError('DenseTracker: uint8 or float64 images only, got {}'.format(img.dtype))
            if img.ndim != 2:
                raise ValueError('DenseTracker: a single-channel image is required, got shape {}'.format(img.shape))
            img = np.ascontiguousarray(img)
        dep = None
        if depth is not None:
            dep = np.ascontiguousarray(np.asarray(depth, dtype=np.float64))
            if img is not None and dep.shape != img.shape:
                raise ValueError('DenseTracker: depth shape {} differs from the image shape {}'.format(dep.shape, img.shape))
        h, w = (img.shape if img is not None else dep.shape)
        self._pending += [a for a in (img, dep) if a is not None]
        nat.check(self._lib.ps_dense_upload(self._h, int(slot), 0 if img is None or img.dtype == np.uint8 else 1, int(h), int(w),
                                            None if img is None else img.ctypes.data_as(C.c_void_p), nat.f64p(dep)))

    def make_tables(self, slot, levels, cams, intensity_covar, depth_covar, min_grad):
        """Pixel tables of `slot` for each level of `levels`, with the camera of the same position in `cams` (RGBDCamera)."""
        lv = np.ascontiguousarray(levels, dtype=np.int32)
        c6 = np.ascontiguousarray([[c.cu, c.cv, c.fu, c.fv, c.w, c.h] for c in cams], dtype=np.float64).reshape(-1, 6)
        if c6.shape[0] != lv.size:
            raise ValueError('one camera per level is required')
        nat.check(self._lib.ps_dense_make_tables(self._h, int(slot), int(lv.size), nat.i32p(lv), nat.f64p(c6),
                                                 float(intensity_covar), float(depth_covar), float(min_grad)))

    def track(self, ref_slot, track_slot, levels, rot_only, options, loss, pose12):
        """Coarse-to-fine solve: -> (pose12, [iterations per level], [cost history per level])."""
        from pyslam_amd.lowering import _loss_id_k
        lv = np.ascontiguousarray(levels, dtype=np.int32)
        ro = np.ascontiguousarray([1 if r else 0 for r in rot_only], dtype=np.int32)
        o = _solve_options(nat.SolveOptions(), options)
        lid, lk = _loss_id_k(loss)
        cap = o.max_iters + 2
        pin = np.ascontiguousarray(pose12, dtype=np.float64).reshape(12)
        pout = np.zeros(12)
        its = np.zeros(max(lv.size, 1), dtype=np.int32)
        hist = np.zeros((max(lv.size, 1), cap))
        try:
            nat.check(self._lib.ps_dense_track(self._h, int(ref_slot), int(track_slot), int(lv.size), nat.i32p(lv), nat.i32p(ro),
                                               C.byref(o), int(lid), float(lk), nat.f64p(pin), nat.f64p(pout), nat.i32p(its),
                                               nat.f64p(hist), cap))
        finally:
            self._pending = []
        return pout, [int(i) for i in its[:lv.size]], [hist[k, :its[k] + 1].copy() for k in range(lv.size)]

    def read_level(self, slot, level, what):
        """'image' (h, w), 'gradient' (2, h, w) or 'depth' (h, w) of a slot's pyramid level."""
        h, w = self.level_shape(level)
        code = {'image': 0, 'gradient': 1, 'depth': 2}[what]
        out = np.zeros((2, h, w) if code == 1 else (h, w))
        nat.check(self._lib.ps_dense_read_level(self._h, int(slot), int(level), code, nat.f64p(out)))
        self._pending = []
        return out

    def num_pixels(self, slot, level):
        n = C.c_int32()
        nat.check(self._lib.ps_dense_num_pixels(self._h, int(slot), int(level), C.byref(n)))
        return n.value

    def read_tables(self, slot, level):
        """The level's pixel tables, named as PhotometricResidualSE3.device_tables() names them."""
        n = self.num_pixels(slot, level)
        t = dict(pt_ref=np.zeros((n, 3)), im_ref=np.zeros(n), im_jac=np.zeros((n, 2)), tri_jac_d=np.zeros((n, 3)))
        nat.check(self._lib.ps_dense_read_tables(self._h, int(slot), int(level), n, nat.f64p(t['pt_ref']), nat.f64p(t['im_ref']),
                                                 nat.f64p(t['im_jac']), nat.f64p(t['tri_jac_d'])))
        self._pending = []
        return t

    def device_bytes(self):
        b = C.c_int64()
        nat.check(self._lib.ps_dense_device_bytes(self._h, C.byref(b)))
        return b.value

_TABLES_F64 = ('obs_uvd', 'cams', 'stiff3', 'obs_groups', 'e_Tobs_inv', 'u_Tobs_inv', 'stiffd', 'edge_groups')
_TABLES_I32 = ('pose_rid', 'point_vid', 'obs_pose', 'obs_point', 'obs_grp', 'e_i', 'e_j', 'e_grp', 'u_i', 'u_grp')


def resident_tables(lp, device='cuda:0', params=True, tables=True):
    """A view of a LoweredProblem whose tables are torch tensors in HBM -- what a torch caller that built its problem on the
    device hands to DeviceProblem (ps_problem_desc.flags = PS_DESC_DEVICE_PARAMS | PS_DESC_DEVICE_TABLES): no host copy of
    the measurement tables is needed on the caller's side."""
    import copy
    import torch
    out = copy.copy(lp)
    if params:
        out.poses = torch.as_tensor(np.ascontiguousarray(lp.poses, dtype=np.float64)).to(device)
        out.points = torch.as_tensor(np.ascontiguousarray(lp.points, dtype=np.float64)).to(device)
    if tables:
        for name in _TABLES_F64:
            setattr(out, name, torch.as_tensor(np.ascontiguousarray(getattr(lp, name), dtype=np.float64)).to(device))
        for name in _TABLES_I32:
            setattr(out, name, torch.as_tensor(np.ascontiguousarray(getattr(lp, name), dtype=np.int32)).to(device))
    return out
