"""Seeded synthetic problems as LoweredProblem tables.

The generators are shared by bench.py, the parity tests and
oracle/gen_golden.py, so the HIP path, the numpy oracle and the verbatim
reference all see byte-identical inputs.  ``to_objects`` rebuilds the
object-graph form (one residual object per block) for any package that
offers the reference's class names -- the reference itself in the authoring
container, or this build's ``pyslam`` shim.
"""
import numpy as np

from pyslam_amd.liegroups import SE2, SE3, SO2, SO3
from pyslam_amd.lowering import (LoweredProblem, pack_pose_matrices,
                                 pose_rows_to_matrices)
from pyslam_amd.utils import invsqrt
from pyslam_amd import losses

STEREO_BA_CAMERA = (640., 480., 1000., 1000., 0.25, 1280, 960)  # reference examples/stereo_ba.py:29


# ---------------------------------------------------------------------------
# batched SE(3) helpers (generation only)
# ---------------------------------------------------------------------------
def _exp_many(xis, group=SE3):
    return np.stack([group.exp(x).as_matrix() for x in np.atleast_2d(xis)])


def _inv_many(Ts):
    n = Ts.shape[1] - 1
    out = np.tile(np.identity(n + 1), (Ts.shape[0], 1, 1))
    Rt = np.transpose(Ts[:, :n, :n], (0, 2, 1))
    out[:, :n, :n] = Rt
    out[:, :n, n] = -np.einsum('nij,nj->ni', Rt, Ts[:, :n, n])
    return out


def _project(cam5, pts_c):
    cu, cv, fu, fv, b = cam5
    iz = 1. / pts_c[:, 2]
    return np.stack([fu * pts_c[:, 0] * iz + cu, fv * pts_c[:, 1] * iz + cv, fu * b * iz], axis=1)


def _triangulate(cam5, uvd):
    cu, cv, fu, fv, b = cam5
    bd = b / uvd[:, 2]
    return np.stack([(uvd[:, 0] - cu) * bd, (uvd[:, 1] - cv) * bd * (fu / fv), fu * bd], axis=1)


def _loss_row(loss):
    return float(loss.LOSS_ID), float(getattr(loss, 'k', 0.))


# ---------------------------------------------------------------------------
# C3 / C4: stereo bundle adjustment
# ---------------------------------------------------------------------------
def stereo_ba(num_kf=200, num_lm=50000, obs_per_lm=10, half_window=20, seed=0,
              loss=None, pose_noise=0.01, point_noise=0.05, const_first_pose=True,
              const_point_fraction=0.0, lm_offset=0, lm_total=None):
    """Stereo BA in the shape of reference examples/stereo_ba.py, scaled up.

    ``lm_offset`` / ``lm_total`` select a contiguous landmark shard of a larger
    problem generated with the same seed (multi-GPU: every rank derives the
    same keyframes and its own landmarks).
    Returns (LoweredProblem, truth dict).
    """
    loss = loss or losses.L2Loss()
    cam5 = np.array(STEREO_BA_CAMERA[:5])
    stiff = invsqrt(np.diagflat([1., 1., 2.]))
    rng = np.random.default_rng(seed)

    k = np.arange(num_kf, dtype=float)
    xi = np.zeros((num_kf, 6))
    xi[:, 0] = 0.05 * k
    xi[:, 5] = 0.002 * k
    T_true = _exp_many(xi)
    T_init = np.einsum('nij,njk->nik', _exp_many(pose_noise * rng.standard_normal((num_kf, 6))), T_true)
    if const_first_pose:
        T_init[0] = T_true[0]

    total = lm_total if lm_total is not None else num_lm
    # per-landmark streams are derived from (seed, landmark id) blocks so a
    # shard reproduces exactly the rows of the full problem
    lrng = np.random.default_rng([seed, 1])
    kc_all = lrng.integers(0, num_kf, size=total)
    pc_all = np.stack([lrng.uniform(-8., 8., total), lrng.uniform(-3., 3., total),
                       lrng.uniform(6., 30., total)], axis=1)
    keys_all = lrng.random((total, 2 * half_window + 1))
    noise_pt_all = point_noise * lrng.standard_normal((total, 3))
    sl = slice(lm_offset, lm_offset + num_lm)
    kc, pc, sel_keys, noise_pt = kc_all[sl], pc_all[sl], keys_all[sl], noise_pt_all[sl]

    T_inv = _inv_many(T_true)
    pts_true = np.einsum('nij,nj->ni', T_inv[kc, :3, :3], pc) + T_inv[kc, :3, 3]
    pts_init = pts_true + noise_pt

    # choose obs_per_lm distinct keyframes in [kc-hw, kc+hw] clipped to [0, K)
    offs = np.arange(-half_window, half_window + 1)
    cand = kc[:, None] + offs[None, :]
    valid = (cand >= 0) & (cand < num_kf)
    sel_keys = np.where(valid, sel_keys, 2.)          # invalid candidates sort last
    n_obs = min(obs_per_lm, int(valid.sum(axis=1).min()))
    pick = np.sort(np.argsort(sel_keys, axis=1)[:, :n_obs], axis=1)
    obs_pose = np.take_along_axis(cand, pick, axis=1).reshape(-1)
    obs_point = np.repeat(np.arange(num_lm), n_obs)

    p_cam = (np.einsum('nij,nj->ni', T_true[obs_pose, :3, :3], pts_true[obs_point])
             + T_true[obs_pose, :3, 3])
    orng = np.random.default_rng([seed, 2, lm_offset])
    uvd = _project(cam5, p_cam) + orng.standard_normal((obs_pose.size, 3)) * np.sqrt([1., 1., 2.])

    rid = np.arange(num_kf, dtype=np.int32)
    if const_first_pose:
        rid = rid - 1          # pose 0 -> -1 (held constant)
    vid = np.arange(num_lm, dtype=np.int32)
    if const_point_fraction > 0.:
        fixed = np.random.default_rng([seed, 3]).random(num_lm) < const_point_fraction
        vid = np.where(fixed, -1, np.cumsum(~fixed) - 1).astype(np.int32)
        pts_init[fixed] = pts_true[fixed]
        # the reference cannot solve with a block whose parameters are ALL constant
        # (problem.py:346-348 leaves e_blocks[ridx] = None and np.bmat raises)
        keep = ~((rid[obs_pose] < 0) & (vid[obs_point] < 0))
        obs_pose, obs_point, uvd = obs_pose[keep], obs_point[keep], uvd[keep]

    lp = LoweredProblem(
        dof=6, poses=pack_pose_matrices(T_init), pose_rid=rid,
        points=pts_init, point_vid=vid,
        obs_pose=obs_pose, obs_point=obs_point, obs_uvd=uvd,
        cams=cam5[None, :], stiff3=stiff.reshape(1, 9),
        obs_groups=np.array([[0., 0., *_loss_row(loss)]]),
        pose_keys=['T_cam{}_w'.format(i) for i in range(num_kf)],
        point_keys=['pt{}_w'.format(j + lm_offset) for j in range(num_lm)]).finalize()
    return lp, {'poses': T_true, 'points': pts_true}


def mono_ba(num_kf=200, num_lm=50000, obs_per_lm=10, half_window=20, seed=0, loss=None, pose_noise=0.01,
            point_noise=0.05, stereo_fraction=0.0):
    """Monocular BA: stereo_ba's scene (same seed, same keyframes, landmarks, observation lists and (u, v) noise) seen by a
    pinhole camera that measures only (u, v) -- cams row b = -2, third coordinate of every observation 0, the 2 x 2
    stiffness (unit pixel noise) in the top-left of a 3 x 3.  The FIRST TWO keyframes are held constant at their true
    poses: monocular BA has seven gauge directions, the baseline between two held poses fixes the scale.
    ``stereo_fraction`` > 0: that share of the observations (seeded) stays stereo, in a second (camera, stiffness) group:
    both kinds of camera on the same landmarks.  Returns (LoweredProblem, truth dict) like stereo_ba."""
    lp, truth = stereo_ba(num_kf=num_kf, num_lm=num_lm, obs_per_lm=obs_per_lm, half_window=half_window, seed=seed, loss=loss,
                          pose_noise=pose_noise, point_noise=point_noise, const_first_pose=True)
    if num_kf < 3:
        raise ValueError('mono_ba: at least three keyframes (two are held constant)')
    lp.poses[1] = pack_pose_matrices(truth['poses'][1:2])[0]
    lp.pose_rid = np.maximum(np.arange(num_kf, dtype=np.int32) - 2, -1)
    cam5 = lp.cams[0].copy()
    mono_cam = cam5.copy()
    mono_cam[4] = -2.
    S2 = np.zeros((3, 3))
    S2[:2, :2] = invsqrt(np.identity(2))
    row = lp.obs_groups[0].copy()
    if stereo_fraction > 0.:
        stereo = np.random.default_rng([seed, 4]).random(lp.num_obs) < stereo_fraction
        lp.cams = np.stack([mono_cam, cam5])
        lp.stiff3 = np.stack([S2.ravel(), lp.stiff3[0]])
        lp.obs_groups = np.array([[0., 0., row[2], row[3]], [1., 1., row[2], row[3]]])
        lp.obs_grp = stereo.astype(np.int32)
        lp.obs_uvd[~stereo, 2] = 0.
    else:
        lp.cams = mono_cam[None, :]
        lp.stiff3 = S2.reshape(1, 9)
        lp.obs_uvd[:, 2] = 0.
    return lp.finalize(), truth


# ---------------------------------------------------------------------------
# C2: SE(3) pose graph;  C1-style: SE(2) pose graph
# ---------------------------------------------------------------------------
def pose_graph(num_poses=10000, num_loops=40001, dof=6, seed=2, loss=None,
               prior_first=True, const_first=False, init_noise=0.02, meas_noise=0.01,
               orientation_loops=False):
    """Noisy helix (SE3) / arc (SE2) with odometry + short-range loop closures.
    orientation_loops (SE3): the loop closures measure the relative ROTATION only
    (reference residuals/pose_to_pose_orientation_residual.py), lowered as lowering.py does."""
    loss = loss if loss is not None else losses.HuberLoss(1.0)
    group = SE3 if dof == 6 else SE2
    rng = np.random.default_rng(seed)
    step = np.array([0.5, 0, 0, 0, 0, 0.05]) if dof == 6 else np.array([0.5, 0, 0.05])
    incs = _exp_many(step + 0.01 * rng.standard_normal((num_poses - 1, dof)), group)
    T_true = [np.identity(dof // 3 + 2)]
    for M in incs:
        T_true.append(M.dot(T_true[-1]))
    T_true = np.stack(T_true)
    T_init = np.einsum('nij,njk->nik',
                       _exp_many(init_noise * rng.standard_normal((num_poses, dof)), group), T_true)

    ei = list(range(num_poses - 1))
    ej = list(range(1, num_poses))
    if num_loops > 0 and num_poses > 3:
        li = rng.integers(0, num_poses - 2, size=num_loops)
        lj = np.minimum(li + rng.integers(2, 31, size=num_loops), num_poses - 1)
        ei += li.tolist()
        ej += lj.tolist()
    ei, ej = np.array(ei), np.array(ej)
    rel = np.einsum('nij,njk->nik', T_true[ej], _inv_many(T_true[ei]))
    meas = np.einsum('nij,njk->nik', _exp_many(meas_noise * rng.standard_normal((ei.size, dof)), group), rel)

    odom = invsqrt(1e-3 * np.identity(dof))
    prior = invsqrt(1e-12 * np.identity(dof))
    rid = np.arange(num_poses, dtype=np.int32)
    if const_first:
        rid = rid - 1
        T_init[0] = T_true[0]
    e_grp = np.zeros(ei.size)
    stiffd = [odom.ravel(), prior.ravel()]
    edge_groups = [[0., *_loss_row(loss)], [1., *_loss_row(losses.L2Loss())]]
    if orientation_loops:
        assert dof == 6
        meas[num_poses - 1:, :3, 3] = 0.           # T_obs = (C_obs, 0)
        S6 = np.zeros((6, 6))
        S6[3:, 3:] = invsqrt(1e-3 * np.identity(3))
        stiffd.append(S6.ravel())
        edge_groups.append([2., *_loss_row(loss)])
        e_grp[num_poses - 1:] = 2
    lp = LoweredProblem(
        dof=dof, poses=pack_pose_matrices(T_init), pose_rid=rid,
        e_i=ei, e_j=ej, e_Tobs_inv=pack_pose_matrices(_inv_many(meas)),
        e_grp=e_grp,
        stiffd=np.stack(stiffd),
        edge_groups=np.array(edge_groups),
        pose_keys=['T_{}_0'.format(i) for i in range(num_poses)])
    if prior_first and not const_first:
        lp.u_i = [0]
        lp.u_Tobs_inv = pack_pose_matrices(_inv_many(T_true[0:1]))
        lp.u_grp = [1]
    return lp.finalize(), {'poses': T_true}


# ---------------------------------------------------------------------------
# C5: sliding-window stereo VO (one pose, N fixed points, robust loss)
# ---------------------------------------------------------------------------
def with_pose_edges(lp, num_loops, seed, loss=None, orientation_loops=False, truth_poses=None):
    """A stereo-BA problem plus the odometry / loop-closure edges and the first-pose prior of a pose graph over the same
    keyframes (mixed visual + relative-pose constraints, as sliding-window VO with odometry would pose them).  Without
    ``truth_poses`` the edge measurements come from ``pose_graph``'s own trajectory and disagree with the visual
    constraints (a valid, if unhappy, problem for single-step parity); with the BA's true poses they are consistent."""
    pg, _ = pose_graph(num_poses=lp.num_poses, num_loops=num_loops, dof=6, seed=seed, loss=loss,
                       orientation_loops=orientation_loops)
    out = lp.copy()
    for name in ('e_i', 'e_j', 'e_Tobs_inv', 'e_grp', 'u_i', 'u_Tobs_inv', 'u_grp', 'stiffd', 'edge_groups'):
        setattr(out, name, getattr(pg, name).copy())
    if truth_poses is not None:
        # measurements of the BA's own true trajectory (+ 1 % noise): visual and relative-pose constraints agree
        T = np.asarray(truth_poses)
        rng = np.random.default_rng([seed, 9])
        rel = np.einsum('nij,njk->nik', T[out.e_j], _inv_many(T[out.e_i]))
        meas = np.einsum('nij,njk->nik', _exp_many(0.01 * rng.standard_normal((out.e_i.size, 6))), rel)
        meas[out.e_grp == 2, :3, 3] = 0.               # rotation-only loop closures: T_obs = (C_obs, 0)
        out.e_Tobs_inv = pack_pose_matrices(_inv_many(meas)) if out.e_i.size else out.e_Tobs_inv
        if out.u_i.size:
            out.u_Tobs_inv = pack_pose_matrices(_inv_many(T[out.u_i]))
    out.validate()
    return out


def motion_only(num_pts=256, seed=3, loss=None, outlier_fraction=0.2):
    loss = loss if loss is not None else losses.CauchyLoss(3.0)
    cam5 = np.array(STEREO_BA_CAMERA[:5])
    stiff = invsqrt(np.diagflat([1., 1., 2.]))
    rng = np.random.default_rng(seed)
    T21 = SE3.exp(np.array([0.3, -0.05, 0.1, 0.01, -0.02, 0.03])).as_matrix()
    p1 = np.stack([rng.uniform(-8, 8, num_pts), rng.uniform(-3, 3, num_pts),
                   rng.uniform(6, 30, num_pts)], axis=1)
    sig = np.sqrt([1., 1., 2.])
    obs1 = _project(cam5, p1) + 0.1 * rng.standard_normal((num_pts, 3)) * sig
    p2 = p1.dot(T21[:3, :3].T) + T21[:3, 3]
    obs2 = _project(cam5, p2) + rng.standard_normal((num_pts, 3)) * sig
    bad = rng.random(num_pts) < outlier_fraction
    obs2[bad, :2] += rng.uniform(20, 60, (int(bad.sum()), 2)) * rng.choice([-1., 1.], (int(bad.sum()), 2))
    lp = LoweredProblem(
        dof=6, poses=pack_pose_matrices(np.identity(4)[None]), pose_rid=[0],
        points=_triangulate(cam5, obs1), point_vid=-np.ones(num_pts),
        obs_pose=np.zeros(num_pts), obs_point=np.arange(num_pts), obs_uvd=obs2,
        cams=cam5[None, :], stiff3=stiff.reshape(1, 9),
        obs_groups=np.array([[0., 0., *_loss_row(loss)]]),
        pose_keys=['T_2_1'], point_keys=[]).finalize()
    return lp, {'poses': T21[None], 'obs_1': obs1, 'obs_2': obs2}


# ---------------------------------------------------------------------------
# LoweredProblem -> object graph (reference-style API)
# ---------------------------------------------------------------------------
_LOSS_NAMES = ['L2Loss', 'L1Loss', 'CauchyLoss', 'HuberLoss', 'TukeyLoss', 'TDistributionLoss']


def make_loss(ns, loss_id, k):
    cls = getattr(ns, _LOSS_NAMES[int(loss_id)])
    return cls() if int(loss_id) < 2 else cls(k)


def pose_objects(rows, dof, ns):
    out = []
    for M in pose_rows_to_matrices(rows, dof):
        if dof == 6:
            out.append(ns.SE3(ns.SO3(M[:3, :3].copy()), M[:3, 3].copy()))
        else:
            out.append(ns.SE2(ns.SO2(M[:2, :2].copy()), M[:2, 2].copy()))
    return out


def to_objects(lp, ns, options=None, points_first=True):
    """Build ``ns.Problem`` from tables.  ``ns`` exposes the reference's public
    names: Problem, Options, StereoCamera, the residual and loss classes and
    the liegroups types.  Parameters are inserted landmarks-first by default,
    like reference examples/stereo_ba.py:53-62."""
    problem = ns.Problem(options if options is not None else ns.Options())
    poses = pose_objects(lp.poses, lp.dof, ns)
    pkeys = lp.pose_keys or ['T{}'.format(i) for i in range(lp.num_poses)]
    lkeys = list(lp.point_keys) + ['_fixed_pt{}'.format(i)
                                   for i in range(lp.num_points - len(lp.point_keys))]

    # (cams row b = -2: a monocular camera -- ns.MonoCamera, 2-vector observations, the 2 x 2 corner of the stiffness)
    cams = [ns.MonoCamera(*row[:4], 1280, 960) if row[4] == -2. else ns.StereoCamera(*row, 1280, 960) for row in lp.cams]
    st3 = [row.reshape(3, 3) for row in lp.stiff3]
    std = [row.reshape(lp.dof, lp.dof) for row in lp.stiffd]
    og = [(cams[int(g[0])], st3[int(g[1])], make_loss(ns, g[2], g[3])) for g in lp.obs_groups]
    eg = [(std[int(g[0])], make_loss(ns, g[1], g[2])) for g in lp.edge_groups]

    for i, Tinv, g in zip(lp.u_i, pose_objects(lp.u_Tobs_inv, lp.dof, ns), lp.u_grp):
        problem.add_residual_block(ns.PoseResidual(Tinv.inv(), eg[g][0]), [pkeys[i]], eg[g][1])
    for i, j, Tinv, g in zip(lp.e_i, lp.e_j, pose_objects(lp.e_Tobs_inv, lp.dof, ns), lp.e_grp):
        S = eg[g][0]
        if lp.dof == 6 and not S[:3, :].any() and not S[:, :3].any():
            # rotation-only edge (lowering.py: 3x3 stiffness embedded in the rotational corner)
            block = ns.PoseToPoseOrientationResidual(Tinv.inv().rot, S[3:, 3:].copy())
        else:
            block = ns.PoseToPoseResidual(Tinv.inv(), S)
        problem.add_residual_block(block, [pkeys[i], pkeys[j]], eg[g][1])
    mono_stiff = {}
    for i, j, uvd, g in zip(lp.obs_pose, lp.obs_point, lp.obs_uvd, lp.obs_grp):
        cam, S, loss = og[g]
        if getattr(cam, 'CAMERA_ID', None) == 2:
            S2 = mono_stiff.get(id(S))
            if S2 is None:
                S2 = mono_stiff[id(S)] = S[:2, :2].copy()
            problem.add_residual_block(ns.ReprojectionResidual(cam, uvd[:2].copy(), S2), [pkeys[i], lkeys[j]], loss)
            continue
        problem.add_residual_block(ns.ReprojectionResidual(cam, uvd.copy(), S),
                                   [pkeys[i], lkeys[j]], loss)

    params = {}
    pt_items = [(k, p.copy()) for k, p in zip(lkeys, lp.points)]
    pose_items = list(zip(pkeys, poses))
    for k, v in (pt_items + pose_items) if points_first else (pose_items + pt_items):
        params[k] = v
    problem.initialize_params(params)
    const = [k for k, r in zip(pkeys, lp.pose_rid) if r < 0] + \
            [k for k, v in zip(lkeys, lp.point_vid) if v < 0]
    if const:
        problem.set_parameters_constant(const)
    return problem


def photometric_scene(h=48, w=64, seed=5, xi_true=(0.03, -0.02, 0.04, 0.01, -0.015, 0.02), rgbd=False,
                      noise=0.0, fu=None):
    """A textured plane seen from two poses, rendered EXACTLY (no warping): the intensity is a smooth function of
    the 3-D point, the plane n.P = c is given in the reference frame, and every tracking-image pixel is the
    intensity at the intersection of its ray with that plane.

    Returns camera parameters ``cam`` = (cu, cv, fu, fv, b, w, h) (b = 0 and depth instead of disparity when
    ``rgbd``), ``im_ref`` (h, w), ``depth_ref`` (disparity or depth, (h, w)), ``im_track`` (h, w), ``im_jac``
    (2, h, w) central-difference gradient of im_ref, and ``T_true`` (4 x 4, track <- ref).
    The inputs of the reference's PhotometricResidualSE3 (photometric_residual.py:44-46)."""
    rng = np.random.default_rng(seed)
    fu = float(fu if fu is not None else 0.9 * w)
    cu, cv, fv, b = 0.5 * w - 0.5, 0.5 * h - 0.5, fu, 0.25
    n = np.array([0.15, -0.1, 1.0]); n /= np.linalg.norm(n)
    c = 4.0
    freq = rng.uniform(0.6, 2.2, size=(6, 3)) * rng.choice([-1., 1.], size=(6, 3))
    phase = rng.uniform(0, 2 * np.pi, 6)
    amp = rng.uniform(10., 30., 6)

    def intensity(P):
        return 100. + np.sum(amp * np.sin(P @ freq.T + phase), axis=-1)

    u, v = np.meshgrid(np.arange(w, dtype=float), np.arange(h, dtype=float), indexing='xy')
    rays = np.stack([(u - cu) / fu, (v - cv) / fv, np.ones_like(u)], axis=-1)
    # reference view: P = s d with n.P = c
    s_ref = c / (rays @ n)
    P_ref = rays * s_ref[..., None]
    im_ref = intensity(P_ref)
    z_ref = P_ref[..., 2]
    depth_ref = z_ref if rgbd else fu * b / z_ref
    # tracking view: P_ref = R^T (s d' - t)
    T = SE3.exp(np.asarray(xi_true, dtype=float))
    R, t = T.rot.as_matrix(), np.asarray(T.trans, dtype=float)
    Rt_n = R @ n                                   # n . R^T x = (R n) . x
    s_trk = (c + Rt_n @ t) / (rays @ Rt_n)
    P_in_ref = (rays * s_trk[..., None] - t) @ R    # rows: R^T (s d' - t)
    im_track = intensity(P_in_ref)
    if noise:
        im_ref = im_ref + noise * rng.standard_normal(im_ref.shape)
        im_track = im_track + noise * rng.standard_normal(im_track.shape)
    gy, gx = np.gradient(im_ref)
    cam = (cu, cv, fu, fv, 0. if rgbd else b, w, h)
    return dict(cam=cam, im_ref=im_ref, depth_ref=depth_ref, im_track=im_track, im_jac=np.stack([gx, gy]),
                T_true=T.as_matrix(), rgbd=rgbd)


def rgbd_sequence(h=96, w=128, n_frames=8, seed=0, step=(0.02, -0.01, 0.04, 0.012, 0.015, -0.006), hole_fraction=0.01,
                  texture=1.0):
    """An RGB-D sequence of an exactly rendered textured scene (three planes: a back wall, a floor and a slanted side
    wall, so the depth has edges) seen along a smooth trajectory, rendered as photometric_scene renders its plane: every
    pixel is the intensity of the 3-D point its ray meets first, with no warping or resampling.

    The camera starts at the world origin and moves by about ``step`` (translation, rotation; per frame) with a slow
    sinusoidal wobble.  Intensities are smooth functions of the world point, quantised to uint8; ``texture`` scales the
    spatial frequencies (1.0: a few pixels per intensity step at every size).  Depth is the camera z in metres with
    ``hole_fraction`` of the pixels NaN and as many 0 (invalid measurements).

    Returns ``images`` (n, h, w) uint8, ``depth`` (n, h, w) float64, ``cam`` = (cu, cv, fu, fv, w, h) and ``T_c_w``
    (n, 4, 4) world-to-camera poses."""
    rng = np.random.default_rng(seed)
    fu = fv = 0.9 * w
    cu, cv = 0.5 * w - 0.5, 0.5 * h - 0.5
    planes = [(np.array([0., 0., 1.]), 5.0),                                    # back wall z = 5
              (np.array([0., 1., 0.]), 1.0),                                    # floor y = 1 (y points down)
              (np.array([1., 0., 0.35]) / np.linalg.norm([1., 0., 0.35]), -1.2)]  # slanted wall on the left
    k = fu / 100. * texture
    freq = rng.uniform(0.8, 2.6, size=(6, 3)) * rng.choice([-1., 1.], size=(6, 3)) * k
    phase = rng.uniform(0, 2 * np.pi, 6)
    amp = rng.uniform(12., 22., 6)

    def intensity(P):
        return 128. + np.sum(amp * np.sin(P @ freq.T + phase), axis=-1)

    u, v = np.meshgrid(np.arange(w, dtype=float), np.arange(h, dtype=float), indexing='xy')
    rays = np.stack([(u - cu) / fu, (v - cv) / fv, np.ones_like(u)], axis=-1)
    step = np.asarray(step, dtype=float)
    images = np.zeros((n_frames, h, w), dtype=np.uint8)
    depth = np.zeros((n_frames, h, w))
    T_c_w = np.zeros((n_frames, 4, 4))
    for f in range(n_frames):
        xi = step * f + 0.3 * step * np.sin(0.7 * f)
        T = SE3.exp(xi)
        R, t = T.rot.as_matrix(), np.asarray(T.trans, dtype=float)
        s_best = np.full((h, w), np.inf)
        for n, c in planes:
            Rn = R @ n                                   # n . P_w = c with P_w = R^T (s d - t)
            with np.errstate(divide='ignore', invalid='ignore'):
                s = (c + Rn @ t) / (rays @ Rn)
            s_best = np.where((s > 0.05) & (s < s_best), s, s_best)
        P_c = rays * s_best[..., None]
        P_w = (P_c - t) @ R                              # rows: R^T (P_c - t)
        images[f] = np.clip(np.round(intensity(P_w)), 0, 255).astype(np.uint8)
        d = s_best.copy()
        holes = rng.random((h, w))
        d[holes < hole_fraction] = np.nan
        d[(holes >= hole_fraction) & (holes < 2 * hole_fraction)] = 0.
        depth[f] = d
        T_c_w[f] = T.as_matrix()
    return dict(images=images, depth=depth, cam=(cu, cv, fu, fv, w, h), T_c_w=T_c_w)



def stereo_sequence(h=96, w=128, n_frames=8, seed=0, step=(0.02, -0.01, 0.04, 0.012, 0.015, -0.006), baseline=0.12,
                    cell=0.16, edge=0.):
    """A stereo sequence of the scene of rgbd_sequence (back wall, floor, slanted side wall), rendered the same exact
    way (every pixel is the intensity of the point its ray meets first) from a left camera on rgbd_sequence's
    trajectory and a right camera ``baseline`` metres along the left camera's x axis.

    The texture has corners: each plane carries a seeded random piecewise-constant pattern, squares of ``cell`` metres
    in the plane's own coordinates (the smooth sinusoids of rgbd_sequence give a corner detector nothing to find).
    With ``edge`` = 0 the cells have step edges: point-sampled, every edge then falls on a whole pixel in each image and
    the images hold no sub-pixel edge position.  With ``edge`` > 0 the last ``edge`` of every cell ramps linearly into
    its neighbour (an edge of finite width, as a camera's blur gives), still evaluated exactly at the ray's point.

    Returns ``left``, ``right`` (n, h, w) uint8, ``depth`` (n, h, w) float64 (true camera z of every left pixel, no
    holes), ``cam`` = (cu, cv, fu, fv, b, w, h) and ``T_c_w`` (n, 4, 4) world-to-left-camera poses; with the depth and
    the poses ``stereo_correspondence`` gives the true position of every left pixel in the other images."""
    rng = np.random.default_rng(seed)
    fu = fv = 0.9 * w
    cu, cv = 0.5 * w - 0.5, 0.5 * h - 0.5
    n2 = np.array([1., 0., 0.35]) / np.linalg.norm([1., 0., 0.35])
    planes = [(np.array([0., 0., 1.]), 5.0, np.array([1., 0., 0.]), np.array([0., 1., 0.])),
              (np.array([0., 1., 0.]), 1.0, np.array([1., 0., 0.]), np.array([0., 0., 1.])),
              (n2, -1.2, np.array([0., 1., 0.]), np.cross(n2, [0., 1., 0.]))]
    N = 64
    tables = rng.integers(30, 226, size=(len(planes), N, N))
    u, v = np.meshgrid(np.arange(w, dtype=float), np.arange(h, dtype=float), indexing='xy')
    rays = np.stack([(u - cu) / fu, (v - cv) / fv, np.ones_like(u)], axis=-1)
    step = np.asarray(step, dtype=float)

    def render(R, t):
        s_best = np.full((h, w), np.inf)
        which = np.zeros((h, w), dtype=int)
        for k, (n, c, _, _) in enumerate(planes):
            Rn = R @ n
            with np.errstate(divide='ignore', invalid='ignore'):
                s = (c + Rn @ t) / (rays @ Rn)
            hit = (s > 0.05) & (s < s_best)
            s_best = np.where(hit, s, s_best)
            which = np.where(hit, k, which)
        P_w = (rays * s_best[..., None] - t) @ R
        img = np.zeros((h, w), dtype=np.uint8)
        for k, (_, _, e1, e2) in enumerate(planes):
            a, b = P_w @ e1 / cell, P_w @ e2 / cell
            i, j = np.floor(a).astype(np.int64), np.floor(b).astype(np.int64)
            if edge > 0:                                 # the last `edge` of a cell ramps linearly into its neighbour
                sa, sb = np.clip((a - i - (1. - edge)) / edge, 0., 1.), np.clip((b - j - (1. - edge)) / edge, 0., 1.)
            else:
                sa = sb = np.zeros_like(a)
            t = tables[k]
            val = ((1. - sa) * (1. - sb) * t[i % N, j % N] + sa * (1. - sb) * t[(i + 1) % N, j % N] +
                   (1. - sa) * sb * t[i % N, (j + 1) % N] + sa * sb * t[(i + 1) % N, (j + 1) % N])
            img = np.where(which == k, np.round(val), img).astype(np.uint8)
        return img, s_best

    left = np.zeros((n_frames, h, w), dtype=np.uint8)
    right = np.zeros((n_frames, h, w), dtype=np.uint8)
    depth = np.zeros((n_frames, h, w))
    T_c_w = np.zeros((n_frames, 4, 4))
    for f in range(n_frames):
        xi = step * f + 0.3 * step * np.sin(0.7 * f)
        T = SE3.exp(xi)
        R, t = T.rot.as_matrix(), np.asarray(T.trans, dtype=float)
        left[f], depth[f] = render(R, t)
        right[f], _ = render(R, t - np.array([baseline, 0., 0.]))
        T_c_w[f] = T.as_matrix()
    return dict(left=left, right=right, depth=depth, cam=(cu, cv, fu, fv, baseline, w, h), T_c_w=T_c_w)


def mono_sequence(h=96, w=128, n_frames=8, seed=0, **kw):
    """The left camera of ``stereo_sequence`` (same arguments) as a monocular sequence: ``images`` (n, h, w) uint8, ``depth``
    (n, h, w) true camera z of every pixel, ``T_c_w`` (n, 4, 4) and ``cam`` = (cu, cv, fu, fv, w, h)."""
    seq = stereo_sequence(h, w, n_frames, seed=seed, **kw)
    cu, cv, fu, fv = seq['cam'][:4]
    return dict(images=seq['left'], depth=seq['depth'], T_c_w=seq['T_c_w'], cam=(cu, cv, fu, fv, w, h))


def stereo_correspondence(seq, f0, f1, uv):
    """True positions of the left pixels ``uv`` (n, 2; integer) of frame f0 of a stereo_sequence in the other images:
    (n, 8) with the columns u1p v1p u2p v2p u1c v1c u2c v2c (1 left, 2 right; p frame f0, c frame f1)."""
    cu, cv, fu, fv, b = seq['cam'][:5]
    uv = np.asarray(uv)
    ui, vi = uv[:, 0].astype(int), uv[:, 1].astype(int)
    z = seq['depth'][f0][vi, ui]
    P = np.stack([(ui - cu) * z / fu, (vi - cv) * z / fv, z], axis=1)
    T = seq['T_c_w'][f1] @ np.linalg.inv(seq['T_c_w'][f0])
    Q = P @ T[:3, :3].T + T[:3, 3]
    u1c, v1c = fu * Q[:, 0] / Q[:, 2] + cu, fv * Q[:, 1] / Q[:, 2] + cv
    return np.stack([ui, vi, ui - fu * b / z, vi, u1c, v1c, u1c - fu * b / Q[:, 2], v1c], axis=1).astype(float)

# ---------------------------------------------------------------------------
# user-defined residual blocks (no KIND: no typed device kernel), as a user of Problem writes them -- the blocks
# Options.hybrid_blocks evaluates on the host beside the typed tables (tools/gen_hybrid_golden.py, tests)
# ---------------------------------------------------------------------------
class TranslationPrior:
    """r = S (t - t_obs) on one SE(3) / SE(2) pose (a GPS / position prior).  Jacobian in the pose's perturbation
    (T <- exp(xi) T, xi = [rho | phi]): d t = rho + phi x t, i.e. S [I | -t^] (SE2: S [I | (-t_y, t_x)])."""

    def __init__(self, t_obs, stiffness):
        self.t_obs = np.asarray(t_obs, dtype=float)
        self.stiffness = np.asarray(stiffness, dtype=float)

    def evaluate(self, params, compute_jacobians=None):
        T = params[0]
        residual = self.stiffness.dot(T.trans - self.t_obs)
        if not compute_jacobians:
            return residual
        jacobians = [None]
        if compute_jacobians[0]:
            jacobians[0] = self.stiffness.dot(type(T).odot(T.trans).reshape(T.trans.size, -1))
        return residual, jacobians


class TranslationSmoothness:
    """r = S (t_0 - 2 t_1 + t_2) on three poses (a constant-velocity smoothness factor)."""

    def __init__(self, stiffness):
        self.stiffness = np.asarray(stiffness, dtype=float)

    def evaluate(self, params, compute_jacobians=None):
        T0, T1, T2 = params
        residual = self.stiffness.dot(T0.trans - 2. * T1.trans + T2.trans)
        if not compute_jacobians:
            return residual
        jacobians = [None, None, None]
        for k, (T, c) in enumerate(zip(params, (1., -2., 1.))):
            if compute_jacobians[k]:
                jacobians[k] = c * self.stiffness.dot(type(T).odot(T.trans).reshape(T.trans.size, -1))
        return residual, jacobians


class Untyped:
    """Delegates evaluate() to a typed block but carries no KIND: the same residual as a user-defined block."""

    def __init__(self, inner):
        self.inner = inner

    def evaluate(self, params, compute_jacobians=None):
        return self.inner.evaluate(params, compute_jacobians)


def add_user_blocks(problem, lp, ns, kinds, poses, t_obs, stiffness, loss_rows):
    """Add the user blocks of a table spec to `problem` (built by to_objects from `lp`): per block its kind (0:
    TranslationPrior on poses[b, 0], 1: TranslationSmoothness on poses[b, :3]), t_obs (first 3 | 2 entries), the n x n
    stiffness (row-major) and the loss row (loss id, k).  -> the blocks, in order."""
    keys = lp.pose_keys or ['T{}'.format(i) for i in range(lp.num_poses)]
    n = 3 if lp.dof == 6 else 2
    out = []
    for kind, p, t, S, lr in zip(kinds, poses, t_obs, stiffness, loss_rows):
        S = np.asarray(S, dtype=float)[:n * n].reshape(n, n)
        if int(kind) == 0:
            block, bkeys = TranslationPrior(np.asarray(t, dtype=float)[:n], S), [keys[int(p[0])]]
        else:
            block, bkeys = TranslationSmoothness(S), [keys[int(q)] for q in p[:3]]
        problem.add_residual_block(block, bkeys, make_loss(ns, lr[0], lr[1]))
        out.append(block)
    return out


# ---------------------------------------------------------------------------
# two monocular views of one scene: correspondences with outliers (pipelines/twoview.py)
# ---------------------------------------------------------------------------
TWO_VIEW_CAMERA = (320., 240., 500., 500., 640, 480)


def two_view(num_pts=192, seed=11, outlier_fraction=0.3, pixel_noise=0.5, rotvec=(0.02, -0.05, 0.03), t=(0.5, -0.05, 0.1)):
    """Two pinhole views of ``num_pts`` points uniform in [-3, 3] x [-2, 2] x [4, 12] m (frame of camera 1), camera
    (cu, cv, fu, fv) = (320, 240, 500, 500) at 640 x 480, second pose p_2 = R p_1 + t with R = exp(rotvec).  Gaussian pixel noise
    on both images; the first ``outlier_fraction * num_pts`` rows of obs_2 are replaced by uniform pixels.
    -> (obs_1 (N, 2), obs_2 (N, 2), T_21 (4, 4) truth, outlier mask (N,) bool); the true points: two_view_points."""
    pts, T = _two_view_scene(num_pts, seed, rotvec, t)
    cu, cv, fu, fv, w, h = TWO_VIEW_CAMERA
    rng = np.random.default_rng([seed, 1])
    p2 = pts @ T[:3, :3].T + T[:3, 3]
    obs_1 = np.stack([fu * pts[:, 0] / pts[:, 2] + cu, fv * pts[:, 1] / pts[:, 2] + cv], axis=1)
    obs_2 = np.stack([fu * p2[:, 0] / p2[:, 2] + cu, fv * p2[:, 1] / p2[:, 2] + cv], axis=1)
    obs_1 = obs_1 + pixel_noise * rng.standard_normal(obs_1.shape)
    obs_2 = obs_2 + pixel_noise * rng.standard_normal(obs_2.shape)
    n_out = int(outlier_fraction * num_pts)
    outlier = np.arange(num_pts) < n_out
    obs_2[:n_out] = rng.uniform([0., 0.], [w, h], size=(n_out, 2))
    return obs_1, obs_2, T, outlier


def _two_view_scene(num_pts, seed, rotvec, t):
    rng = np.random.default_rng([seed, 0])
    pts = np.stack([rng.uniform(-3., 3., num_pts), rng.uniform(-2., 2., num_pts), rng.uniform(4., 12., num_pts)], axis=1)
    T = np.identity(4)
    T[:3, :3] = SO3.exp(np.asarray(rotvec, dtype=np.float64)).as_matrix()
    T[:3, 3] = t
    return pts, T


def two_view_points(num_pts=192, seed=11, rotvec=(0.02, -0.05, 0.03), t=(0.5, -0.05, 0.1)):
    """The true points (N, 3) of two_view's scene, in the frame of camera 1."""
    return _two_view_scene(num_pts, seed, rotvec, t)[0]


# ---------------------------------------------------------------------------
# a third monocular view of two_view's scene: 2-D - 3-D correspondences with outliers (pipelines/pnp.py)
# ---------------------------------------------------------------------------
def pnp_scene(num_pts=192, seed=11, outlier_fraction=0.3, pixel_noise=0.5, rotvec=(-0.03, 0.08, -0.02), t=(-0.6, 0.1, 0.3)):
    """A third pinhole view of two_view_points(num_pts, seed), TWO_VIEW_CAMERA, at the pose p_3 = R p_1 + t with R = exp(rotvec)
    (another pose than two_view's second).  Gaussian pixel noise; the LAST ``outlier_fraction * num_pts`` rows of obs are replaced
    by uniform pixels (two_view replaces the first rows: the two outlier sets are disjoint up to 50 %).
    -> (pts_w (N, 3) the true points in the frame of camera 1, obs (N, 2), T_cw (4, 4) truth, outlier mask (N,) bool)."""
    pts, T = _two_view_scene(num_pts, seed, rotvec, t)
    cu, cv, fu, fv, w, h = TWO_VIEW_CAMERA
    rng = np.random.default_rng([seed, 2])
    p3 = pts @ T[:3, :3].T + T[:3, 3]
    obs = np.stack([fu * p3[:, 0] / p3[:, 2] + cu, fv * p3[:, 1] / p3[:, 2] + cv], axis=1)
    obs = obs + pixel_noise * rng.standard_normal(obs.shape)
    n_out = int(outlier_fraction * num_pts)
    outlier = np.arange(num_pts) >= num_pts - n_out
    if n_out:
        obs[num_pts - n_out:] = rng.uniform([0., 0.], [w, h], size=(n_out, 2))
    return pts, obs, T, outlier


# ---------------------------------------------------------------------------
# two monocular maps of two_view's scene whose scales are unrelated: 3-D - 3-D correspondences with outliers (pipelines/sim3.py)
# ---------------------------------------------------------------------------
def sim3_scene(num_pts=192, seed=11, scale=2.5, outlier_fraction=0.3, point_noise=0.005, pixel_noise=0.5,
               rotvec=(0.04, -0.3, 0.06), t=(1.5, -0.2, 0.8)):
    """The points of _two_view_scene(num_pts, seed) as two maps: pts_1 in the frame of camera 1 at the scene's own scale, pts_2 in
    the frame of camera 2 (p = R p_1 + t, R = exp(rotvec)) in a map ``scale`` times as large, so p_2 = scale R p_1 + scale t.  Each
    map's points carry relative depth noise along their ray (``point_noise``), each camera's pixels (TWO_VIEW_CAMERA) Gaussian noise.
    The first ``outlier_fraction * num_pts`` rows of pts_2 and obs_2 are rotated by one place among themselves: wrong matches between
    real points.  -> (pts_1 (N, 3), pts_2 (N, 3), obs_1 (N, 2), obs_2 (N, 2), scale, T_21 (4, 4) = [R | scale t], outlier mask (N,))."""
    pts, T = _two_view_scene(num_pts, seed, rotvec, t)
    cu, cv, fu, fv, w, h = TWO_VIEW_CAMERA
    rng = np.random.default_rng([seed, 3])
    q = pts @ T[:3, :3].T + T[:3, 3]
    obs_1 = np.stack([fu * pts[:, 0] / pts[:, 2] + cu, fv * pts[:, 1] / pts[:, 2] + cv], axis=1)
    obs_2 = np.stack([fu * q[:, 0] / q[:, 2] + cu, fv * q[:, 1] / q[:, 2] + cv], axis=1)
    obs_1 = obs_1 + pixel_noise * rng.standard_normal(obs_1.shape)
    obs_2 = obs_2 + pixel_noise * rng.standard_normal(obs_2.shape)
    pts_1 = pts * (1. + point_noise * rng.standard_normal(num_pts))[:, None]
    pts_2 = scale * q * (1. + point_noise * rng.standard_normal(num_pts))[:, None]
    n_out = int(outlier_fraction * num_pts)
    outlier = np.arange(num_pts) < n_out
    if n_out:
        pts_2[:n_out], obs_2[:n_out] = np.roll(pts_2[:n_out], 1, axis=0), np.roll(obs_2[:n_out], 1, axis=0)
    T_21 = T.copy()
    T_21[:3, 3] = scale * T[:3, 3]
    return pts_1, pts_2, obs_1, obs_2, float(scale), T_21, outlier


# ---------------------------------------------------------------------------
# Sim(3) pose graphs (pipelines/posegraph.py, pipelines/simgraph.py)
# ---------------------------------------------------------------------------
def sim3_graph(num_vertices=12, num_chords=2, seed=0, perturbation=0.05):
    """A consistent ring graph of similarities: vertex k is a true similarity on a circle of radius 3 with a rotation about a
    tilted axis and the scale exp(0.4 sin(2 pi k / N)); one edge k -> k + 1 (mod N) and ``num_chords`` chords, from every 5th vertex
    to the vertex a third of the ring ahead; every edge is exact (S_j S_i^-1 of the truth).  The start is exp(xi) S_true with
    xi ~ N(0, perturbation^2) per component, except the held vertex 0.
    -> (truth: list of Sim3, start: list of Sim3, held (N,) bool, edges: list of (i, j, S_ji, None))."""
    from pyslam_amd.liegroups import Sim3
    N = int(num_vertices)
    if N < 3:
        raise ValueError("sim3_graph: a ring needs at least 3 vertices")
    rng = np.random.default_rng([seed, 7])
    axis = np.array([0.2, 1.0, -0.3]) / np.linalg.norm([0.2, 1.0, -0.3])
    truth = []
    for k in range(N):
        a = 2. * np.pi * k / N
        R = SO3.exp(a * axis + 0.1 * rng.standard_normal(3))
        t = np.array([3. * np.cos(a), 0.5 * np.sin(2. * a), 3. * np.sin(a)]) + 0.2 * rng.standard_normal(3)
        truth.append(Sim3(R, t, np.exp(0.4 * np.sin(a))))
    pairs = [(k, (k + 1) % N) for k in range(N)]
    pairs += [((5 * c) % N, (5 * c + N // 3) % N) for c in range(int(num_chords))]
    edges = [(i, j, truth[j].dot(truth[i].inv()), None) for i, j in pairs if i != j]
    held = np.arange(N) == 0
    start = [truth[0]] + [Sim3.exp(perturbation * rng.standard_normal(7)).dot(S) for S in truth[1:]]
    return truth, start, held, edges


def sim3_drift_loop(num_keyframes=40, scale_drift=0.01, rot_noise=0.002, seed=0, points_per_keyframe=4):
    """A monocular map that has drifted around a loop.  True poses: ``num_keyframes`` cameras on 97 % of a circle of radius 10,
    looking along the direction of travel.  Estimates: the true relative motions chained from the true first pose, each step's
    translation times (1 + scale_drift)^k -- the local scale of the map grows by ``scale_drift`` per keyframe -- and each step's
    rotation perturbed by ``rot_noise`` rad per axis.  One exact closure between the last keyframe and the first, in
    ``detect_loop``'s convention (entry 0, keyframe K - 1, scale, T_21: p_last = scale R p_first + t, each in its own keyframe's
    local map scale).  Landmarks are owned by keyframes: ``points_per_keyframe`` points in front of each, placed in the estimated map
    at their owner's local scale.
    -> dict: poses_true, poses_est (K, 4, 4 world-to-camera), closure, owner (L,), points_true, points_est (L, 3), scales (K,)."""
    K = int(num_keyframes)
    if K < 3:
        raise ValueError("sim3_drift_loop: at least 3 keyframes")
    rng = np.random.default_rng([seed, 8])
    true = np.zeros((K, 4, 4))
    for k in range(K):
        a = 0.97 * 2. * np.pi * k / K
        R_wc = SO3.roty(-a).as_matrix()                       # camera axes in the world: z along the tangent of the circle
        c = np.array([10. * np.cos(a), 0., 10. * np.sin(a)])
        R_wc = R_wc @ SO3.roty(0.5 * np.pi).as_matrix().T
        true[k] = np.identity(4)
        true[k, :3, :3] = R_wc.T
        true[k, :3, 3] = -R_wc.T @ c
    scales = (1. + scale_drift) ** np.arange(K)
    est = np.zeros_like(true)
    est[0] = true[0]
    for k in range(K - 1):
        rel = true[k + 1] @ np.linalg.inv(true[k])
        rel[:3, :3] = SO3.exp(rot_noise * rng.standard_normal(3)).as_matrix() @ rel[:3, :3]
        rel[:3, 3] *= scales[k + 1]
        est[k + 1] = rel @ est[k]
    rel = true[K - 1] @ np.linalg.inv(true[0])
    T_21 = rel.copy()
    T_21[:3, 3] *= scales[K - 1]
    m = int(points_per_keyframe)
    owner = np.repeat(np.arange(K), m)
    p_c = np.stack([rng.uniform(-2., 2., K * m), rng.uniform(-1., 1., K * m), rng.uniform(3., 8., K * m)], axis=1)
    inv_true, inv_est = np.linalg.inv(true), np.linalg.inv(est)
    points_true = np.einsum('nij,nj->ni', inv_true[owner, :3, :3], p_c) + inv_true[owner, :3, 3]
    p_local = scales[owner][:, None] * p_c
    points_est = np.einsum('nij,nj->ni', inv_est[owner, :3, :3], p_local) + inv_est[owner, :3, 3]
    return dict(poses_true=true, poses_est=est, closure=(0, K - 1, float(scales[K - 1]), T_21), owner=owner, points_true=points_true,
                points_est=points_est, scales=scales)
