"""Sim(3) pose graph on the device: what consumes a verified loop constraint (``loop.detect_loop``,
``SparseMonoPipeline.loop_closures``) and corrects the map.

``Sim3PoseGraph`` is the graph itself: vertices are similarities (``liegroups.Sim3``), an edge (i, j, S_ji) says S_j S_i^-1 = S_ji,
at least one vertex is held, and ``solve`` runs the whole Gauss-Newton loop in one call into the HIP core (ps_sim3pg_solve: the
edge kernel, the dense assembly, the blocked Cholesky chain; csrc/ps_k_sim3pg.h, ps_host_sim3pg.h).  There is no CPU path; the
numpy restatement of the same definition, pipelines/simgraph.py, is what the tests hold the device against.  The system is dense:
at most 1170 free vertices (7 unknowns each, 8192 in all) -- keyframe graphs; a larger graph is an error.

``correct_loop`` is the map correction built on it: keyframe poses as vertices at scale 1, odometry and covisibility edges measured
from the current estimates, one edge per closure, and afterwards every pose and every landmark moved by its keyframe's correction."""
import ctypes as C

import numpy as np

from pyslam_amd import _native as nat
from pyslam_amd.liegroups import SE3, SO3, Sim3

__all__ = ['Sim3PoseGraph', 'correct_loop', 'loop_graph', 'apply_correction', 'DeviceSim3Graph', 'debug_explog', 'MAX_FREE_VERTICES']

MAX_FREE_VERTICES = 8192 // 7


def pack13(S):
    return np.concatenate([S.rot.mat.reshape(9), S.trans, [S.scale]])


def unpack13(row):
    return Sim3(SO3(np.array(row[0:9]).reshape(3, 3)), np.array(row[9:12]), float(row[12]))


def _as_sim3(S):
    if isinstance(S, Sim3):
        return S
    if isinstance(S, SE3):
        return Sim3.from_se3(S)
    M = np.asarray(S, dtype=np.float64)
    if M.shape != (4, 4):
        raise ValueError("a vertex or measurement must be a Sim3, an SE3 or a 4 x 4 similarity matrix")
    return Sim3.from_matrix(M, normalize=True)


def _loss_id_k(loss):
    if loss is None:
        return 0, 0.
    from pyslam_amd.lowering import _loss_id_k as lowered, NotLowerable
    try:
        lid, k = lowered(loss)
    except NotLowerable as err:
        raise ValueError("Sim3PoseGraph: {} (only the built-in losses run on the device)".format(err))
    return int(lid), float(k)


class DeviceSim3Graph:
    """The handle (ps_sim3pg) of a graph given as tables: vertices (N, 13), held (N,), edges i, j (E,), measurements (E, 13),
    stiffness (E, 7, 7) or None.  What ``Sim3PoseGraph`` and the tests drive."""

    def __init__(self, vertices13, held, edge_i, edge_j, edge_obs13, stiffness=None, loss=None):
        nat.require_gpu()
        self.lib = nat.load()
        V = np.ascontiguousarray(vertices13, dtype=np.float64).reshape(-1, 13)
        self.held = np.ascontiguousarray(np.asarray(held, dtype=bool).reshape(V.shape[0]), dtype=np.uint8)
        ei, ej = np.ascontiguousarray(edge_i, dtype=np.int32).ravel(), np.ascontiguousarray(edge_j, dtype=np.int32).ravel()
        obs = np.ascontiguousarray(edge_obs13, dtype=np.float64).reshape(-1, 13)
        W = None if stiffness is None else np.ascontiguousarray(stiffness, dtype=np.float64).reshape(-1, 49)
        if ei.size != ej.size or obs.shape[0] != ei.size or (W is not None and W.shape[0] != ei.size):
            raise ValueError("the edge tables must hold one row per edge")
        self.num_vertices, self.num_edges = V.shape[0], int(ei.size)
        self.n = 7 * int((self.held == 0).sum())
        lid, k = _loss_id_k(loss)
        self.h = nat.H()
        nat.check(self.lib.ps_sim3pg_create(self.num_vertices, nat.f64p(V), self.held.ctypes.data_as(nat.c_u8p), self.num_edges,
                                            nat.i32p(ei), nat.i32p(ej), nat.f64p(obs), nat.f64p(W), lid, k, None, C.byref(self.h)))

    def close(self):
        if getattr(self, 'h', None):
            self.lib.ps_sim3pg_destroy(self.h)
            self.h = None

    __del__ = close

    def set_vertices(self, vertices13):
        V = np.ascontiguousarray(vertices13, dtype=np.float64).reshape(self.num_vertices, 13)
        nat.check(self.lib.ps_sim3pg_set_vertices(self.h, nat.f64p(V)))

    def get_vertices(self):
        V = np.zeros((self.num_vertices, 13))
        nat.check(self.lib.ps_sim3pg_get_vertices(self.h, nat.f64p(V)))
        return V

    def eval_cost(self):
        c = np.zeros(1)
        nat.check(self.lib.ps_sim3pg_eval_cost(self.h, nat.f64p(c)))
        return float(c[0])

    def linearize(self, lam=0.):
        """(H with its diagonal times 1 + lam, g, cost)."""
        H, g, c = np.zeros((self.n, self.n)), np.zeros(self.n), np.zeros(1)
        nat.check(self.lib.ps_sim3pg_linearize(self.h, float(lam), nat.f64p(H), nat.f64p(g), nat.f64p(c)))
        return H, g, float(c[0])

    def iteration(self, lam=0.):
        """One iteration -> (cost after the step, ||dx||, relative residual of the linear solve)."""
        o = np.zeros(3)
        nat.check(self.lib.ps_sim3pg_iteration(self.h, float(lam), nat.f64p(o[0:1]), nat.f64p(o[1:2]), nat.f64p(o[2:3])))
        return float(o[0]), float(o[1]), float(o[2])

    def solve(self, options=None):
        """-> (cost history, iterations, last ||dx||)."""
        from pyslam_amd.device import _solve_options
        from pyslam_amd.problem import Options
        o = _solve_options(nat.SolveOptions(), options if options is not None else Options(), True)
        cap = o.max_iters + 2
        hist, n, its, dxn = np.zeros(cap), C.c_int32(0), C.c_int32(0), C.c_double(0.)
        nat.check(self.lib.ps_sim3pg_solve(self.h, C.byref(o), nat.f64p(hist), cap, C.byref(n), C.byref(its), C.byref(dxn)))
        return hist[:n.value].copy(), int(its.value), float(dxn.value)

    def debug_edges(self):
        """(r~ (E, 7), J~_i (E, 7, 7), J~_j (E, 7, 7)) of the edge kernel at the current vertices."""
        tap = np.zeros((self.num_edges, 105))
        nat.check(self.lib.ps_sim3pg_debug_edges(self.h, nat.f64p(tap)))
        return tap[:, :7].copy(), tap[:, 7:56].reshape(-1, 7, 7).copy(), tap[:, 56:].reshape(-1, 7, 7).copy()

    def profile(self, enable=True):
        ms = np.zeros(5)
        nat.check(self.lib.ps_sim3pg_profile(self.h, int(bool(enable)), nat.f64p(ms)))
        return dict(zip(('edges', 'assemble', 'factor', 'substitute_refine', 'retract_cost'), ms.tolist()))


def debug_explog(xi):
    """The device's exp, log and adjoint on a table (n, 7) of tangent vectors -> (S (n, 13), log(exp(xi)) (n, 7), Ad (n, 7, 7))."""
    nat.require_gpu()
    xi = np.ascontiguousarray(xi, dtype=np.float64).reshape(-1, 7)
    n = xi.shape[0]
    S, back, adj = np.zeros((n, 13)), np.zeros((n, 7)), np.zeros((n, 49))
    nat.check(nat.load().ps_sim3pg_debug_explog(n, nat.f64p(xi), nat.f64p(S), nat.f64p(back), nat.f64p(adj)))
    return S, back, adj.reshape(n, 7, 7)


class Sim3PoseGraph:
    def __init__(self):
        self.vertices = []
        """The vertices (Sim3); replaced by the solved ones"""
        self.held = []
        self.edges = []
        """(i, j, S_ji, stiffness or None) per edge: S_j S_i^-1 = S_ji"""
        self.loss = None
        """None (L2) or one of pyslam's built-in loss objects, applied per residual component"""
        self.cost_history = []
        self.iterations = 0

    def add_vertex(self, S, held=False):
        self.vertices.append(_as_sim3(S))
        self.held.append(bool(held))
        return len(self.vertices) - 1

    def add_edge(self, i, j, S_ji, stiffness=None):
        i, j, n = int(i), int(j), len(self.vertices)
        if not (0 <= i < n and 0 <= j < n):
            raise ValueError("Sim3PoseGraph.add_edge: vertex index out of range ({}, {} of {})".format(i, j, n))
        if i == j:
            raise ValueError("Sim3PoseGraph.add_edge: an edge joins two different vertices")
        W = None
        if stiffness is not None:
            W = np.asarray(stiffness, dtype=np.float64)
            if W.shape != (7, 7):
                raise ValueError("Sim3PoseGraph.add_edge: the stiffness must be a 7 x 7 matrix")
        self.edges.append((i, j, _as_sim3(S_ji), W))

    def tables(self):
        """(vertices (N, 13), held (N,), edge_i, edge_j, measurements (E, 13), stiffness (E, 7, 7) or None)."""
        V = np.array([pack13(S) for S in self.vertices]).reshape(-1, 13)
        E = len(self.edges)
        obs = np.array([pack13(e[2]) for e in self.edges]).reshape(-1, 13)
        W = None
        if any(e[3] is not None for e in self.edges):
            W = np.stack([np.identity(7) if e[3] is None else e[3] for e in self.edges])
        return (V, np.array(self.held, dtype=bool), np.array([e[0] for e in self.edges], dtype=np.int32).reshape(E),
                np.array([e[1] for e in self.edges], dtype=np.int32).reshape(E), obs, W)

    def _check(self):
        if not self.vertices:
            raise ValueError("Sim3PoseGraph: the graph has no vertex")
        if not any(self.held):
            raise ValueError("Sim3PoseGraph: at least one vertex must be held (the gauge of the graph is free otherwise)")
        free = len(self.held) - sum(self.held)
        if free > MAX_FREE_VERTICES:
            raise ValueError("Sim3PoseGraph: {} free vertices, the dense solve takes at most {} (8192 unknowns)".format(free, MAX_FREE_VERTICES))

    def solve(self, options=None):
        """Run the loop on the device; the vertices are replaced by the solved ones and returned (list of Sim3)."""
        self._check()
        if all(self.held):
            self.cost_history, self.iterations = [], 0
            return self.vertices
        dev = DeviceSim3Graph(*self.tables(), loss=self.loss)
        try:
            hist, its, _ = dev.solve(options)
            V = dev.get_vertices()
        finally:
            dev.close()
        self.cost_history, self.iterations = hist.tolist(), its
        self.vertices = [unpack13(row) for row in V]
        return self.vertices


def _pose_matrix(T):
    return T.as_matrix() if hasattr(T, 'as_matrix') else np.asarray(T, dtype=np.float64)


def loop_graph(poses_cw, closures, extra_edges=(), held=(0,), stiffness=None, loss=None):
    """The graph ``correct_loop`` solves (a ``Sim3PoseGraph``): usable with the restatement as well (``tables`` / ``edges``)."""
    P = [_pose_matrix(T) for T in poses_cw]
    K = len(P)
    if K < 2:
        raise ValueError("correct_loop: at least two keyframes are needed")
    held = set(int(h) for h in held)
    if not held or not all(0 <= h < K for h in held):
        raise ValueError("correct_loop: held must name at least one keyframe of the {} given".format(K))
    graph = Sim3PoseGraph()
    graph.loss = loss
    for k in range(K):
        graph.add_vertex(Sim3.from_se3(P[k]), held=k in held)
    V = graph.vertices
    for k in range(K - 1):                                     # odometry: measured from the current estimates
        graph.add_edge(k, k + 1, V[k + 1].dot(V[k].inv()), stiffness)
    for i, j in extra_edges:                                   # covisibility: likewise
        i, j = int(i), int(j)
        if not (0 <= i < K and 0 <= j < K) or i == j:
            raise ValueError("correct_loop: extra edge ({}, {}) does not join two different keyframes".format(i, j))
        if abs(i - j) > 1:
            graph.add_edge(i, j, V[j].dot(V[i].inv()), stiffness)
    if not closures:
        raise ValueError("correct_loop: no closure given")
    for entry, keyframe, scale, T_21 in closures:              # p_keyframe = scale R p_entry + t
        entry, keyframe = int(entry), int(keyframe)
        if not (0 <= entry < K and 0 <= keyframe < K) or entry == keyframe:
            raise ValueError("correct_loop: closure ({}, {}) does not join two different keyframes".format(entry, keyframe))
        graph.add_edge(entry, keyframe, Sim3.from_se3(_pose_matrix(T_21), float(scale)), stiffness)
    return graph


def apply_correction(old, new, poses_cw, landmark_owner=None, points_w=None):
    """Poses and points after the graph moved its vertices from ``old`` to ``new`` (lists of Sim3): the pose of keyframe k is
    ``to_se3()`` of its vertex, a point moves by its owner's correction p' = S_new^-1 S_old p (its coordinates in the owner's camera
    frame keep their direction and scale with the map).  -> (poses as given: list of SE3 or (K, 4, 4); scales (K,); points or None)."""
    objects = len(poses_cw) > 0 and hasattr(poses_cw[0], 'as_matrix')
    poses = [S.to_se3() for S in new]
    if not objects:
        poses = np.stack([T.as_matrix() for T in poses])
    scales = np.array([S.scale for S in new])
    pts = None
    if points_w is not None:
        pts = np.array(points_w, dtype=np.float64).reshape(-1, 3)
        owner = np.asarray(landmark_owner, dtype=np.int64).reshape(-1)
        if owner.size != pts.shape[0]:
            raise ValueError("correct_loop: landmark_owner must name one keyframe per point")
        if owner.size and (owner.min() < 0 or owner.max() >= len(new)):
            raise ValueError("correct_loop: a landmark's owner is not a keyframe")
        for k in np.unique(owner):
            sel = owner == k
            pts[sel] = np.atleast_2d(new[k].inv().dot(old[k]).dot(pts[sel]))
    return poses, scales, pts


def correct_loop(poses_cw, closures, extra_edges=(), held=(0,), landmark_owner=None, points_w=None, stiffness=None, loss=None,
                 options=None):
    """Correct a keyframe map for its detected loops.  ``poses_cw``: world-to-camera poses of the keyframes (SE3 or 4 x 4);
    ``closures``: (entry, keyframe, scale, T_21) in ``detect_loop``'s convention p_keyframe = scale R p_entry + t;
    ``extra_edges``: further keyframe pairs (covisibility), measured like the odometry edges from the current estimates;
    ``landmark_owner`` / ``points_w``: one keyframe per point, and the points.  ``loss``: None (L2) or a built-in loss, per residual
    component; under ``L1Loss`` the IRLS weight is 1 / max(|r_k|, 1e-8) -- the odometry and covisibility edges start at zero residual,
    where the plain 1 / |r_k| is undefined.  -> (poses_cw_new, scales, points_w_new); the graph
    that ran stays in ``correct_loop.last_graph``."""
    graph = loop_graph(poses_cw, closures, extra_edges, held, stiffness, loss)
    old = list(graph.vertices)
    new = graph.solve(options)
    correct_loop.last_graph = graph
    return apply_correction(old, new, poses_cw, landmark_owner, points_w)


correct_loop.last_graph = None
