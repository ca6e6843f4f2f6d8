"""Sim(3) pose graph, host side: ``liegroups.Sim3`` against scipy's matrix exponential and logarithm on every branch, the
restatement (pyslam_amd/pipelines/simgraph.py) -- Jacobians, convergence, the drift scene --, ``correct_loop``'s bookkeeping with the
restatement standing in for the device, argument errors, exports and the source layout.  No device."""
import os
import re

import numpy as np
import pytest
import scipy.linalg as sl

import sim3graph_scenes as gs
from pyslam_amd import synthetic
from pyslam_amd.liegroups import SE3, SO3, Sim3
from pyslam_amd.pipelines import posegraph as pg
from pyslam_amd.pipelines import simgraph as sg
from pyslam_amd.problem import Options

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exp_and_log_against_scipy_on_every_branch():
    xis = gs.tangents()
    assert xis.shape[0] > 150
    worst_exp = worst_log = worst_pi = worst_round = 0.
    for xi in xis:
        S = Sim3.exp(xi)
        M = sl.expm(Sim3.wedge(xi))
        worst_exp = max(worst_exp, np.abs(S.as_matrix() - M).max() / max(1., np.abs(M).max()))
        back = S.log()
        worst_round = max(worst_round, np.abs(back - xi).max())
        L = np.real(sl.logm(S.as_matrix()))
        gap = np.abs(Sim3.vee(L) - back).max() / max(1., np.abs(xi).max())
        if np.linalg.norm(xi[3:6]) > 3.:
            worst_pi = max(worst_pi, gap)
        else:
            worst_log = max(worst_log, gap)
    print('Sim3 over {} tangent vectors: exp against expm {:.2e}, log against logm {:.2e} ({:.2e} at |phi| = 3.1), log(exp) {:.2e}'.format(
        xis.shape[0], worst_exp, worst_log, worst_pi, worst_round))
    assert worst_exp <= gs.TOL_EXPM and worst_log <= gs.TOL_LOGM and 0. < worst_pi <= gs.TOL_LOGM_NEAR_PI
    assert worst_round <= gs.TOL_LOGM
    # the exact zeros
    I = Sim3.exp(np.zeros(7))
    assert np.array_equal(I.as_matrix(), np.identity(4)) and not Sim3.identity().log().any()
    only_rho = Sim3.exp([1., -2., 3., 0., 0., 0., 0.])
    assert np.array_equal(only_rho.trans, [1., -2., 3.]) and only_rho.scale == 1.


def test_the_two_branches_of_w_agree_around_the_series_radius():
    """Series and closed form are the same function: where both are well conditioned (|z| between 0.7 and 1.0) they agree to
    rounding, whichever of theta and sigma carries the magnitude."""
    from pyslam_amd.liegroups.sim3 import w_closed, w_coefficients, w_series
    worst = 0.
    for radius in (0.7, 0.9, 1.0):
        for ang in np.linspace(0., 0.5 * np.pi, 9):
            for sign in (1., -1.):
                th, s = radius * np.sin(ang), sign * radius * np.cos(ang)
                worst = max(worst, np.abs(np.array(w_series(th, s)) - np.array(w_closed(th, s))).max())
    print('W coefficients, series against closed form around |z| = 1: {:.2e}'.format(worst))
    assert worst <= 64 * np.finfo(float).eps                  # sums of ~20 terms of size <= 1, and quotients conditioned <= 30
    assert w_coefficients(0.6, 0.8) == w_series(0.6, 0.8) and w_coefficients(0.6, 0.8 + 1e-9) == w_closed(0.6, 0.8 + 1e-9)
    assert w_coefficients(0., 0.) == (1., 0.5, 1. / 6.) or np.abs(np.array(w_coefficients(0., 0.)) - [1., 0.5, 1. / 6.]).max() <= 1e-16


def test_round_trips_inverse_product_and_adjoint():
    rng = np.random.default_rng(1)
    for _ in range(20):
        xi, x = rng.standard_normal(7) * [2., 2., 2., 0.8, 0.8, 0.8, 0.5], rng.standard_normal(7)
        S, T = Sim3.exp(xi), Sim3.exp(0.7 * rng.standard_normal(7))
        assert np.abs(S.log() - xi).max() <= 1e-13
        assert np.abs(Sim3.exp(S.log()).as_matrix() - S.as_matrix()).max() <= 1e-13
        M = S.as_matrix()
        assert np.abs(S.inv().as_matrix() - np.linalg.inv(M)).max() <= 1e-13
        assert np.abs(S.dot(S.inv()).as_matrix() - np.identity(4)).max() <= 1e-14
        assert np.abs(S.dot(T).as_matrix() - M @ T.as_matrix()).max() <= 1e-13
        p = rng.standard_normal((5, 3))
        assert np.abs(S.dot(p) - (S.scale * p @ S.rot.mat.T + S.trans)).max() <= 1e-14
        assert np.abs(S.dot(p[0]) - (M @ np.append(p[0], 1.))[:3]).max() <= 1e-14
        assert np.abs(S.dot(np.append(p[0], 1.)) - M @ np.append(p[0], 1.)).max() <= 1e-14
        # Ad(S) x = vee(S x^ S^-1)
        assert np.abs(Sim3.vee(M @ Sim3.wedge(x) @ np.linalg.inv(M)) - S.adjoint() @ x).max() <= 1e-13
        assert np.abs(Sim3.vee(Sim3.wedge(x)) - x).max() <= 1e-15    # (sigma comes back as a third of the trace)
        Q = Sim3.from_matrix(M)
        assert abs(Q.scale - S.scale) <= 1e-14 * S.scale and np.abs(Q.as_matrix() - M).max() <= 1e-13
        P = Sim3.exp(xi)
        P.perturb(x)
        assert np.abs(P.as_matrix() - Sim3.exp(x).as_matrix() @ M).max() <= 1e-13
    assert Sim3.dof == 7 and Sim3.wedge(np.zeros((3, 7))).shape == (3, 4, 4) and Sim3.vee(np.zeros((3, 4, 4))).shape == (3, 7)


def test_to_se3_is_the_camera_in_the_rescaled_map():
    rng = np.random.default_rng(2)
    T = SE3.exp(rng.standard_normal(6))
    S = Sim3.from_se3(T, 2.5)
    assert S.scale == 2.5 and np.array_equal(S.rot.mat, T.rot.mat) and np.array_equal(S.trans, T.trans)
    p = rng.standard_normal((6, 3))
    rigid = S.to_se3()
    assert isinstance(rigid, SE3) and np.abs(rigid.dot(p) * S.scale - S.dot(p)).max() <= 1e-14     # same rays, depths over the scale
    assert np.array_equal(Sim3.from_se3(T).to_se3().as_matrix(), T.as_matrix())
    assert np.array_equal(Sim3.from_se3(T.as_matrix()).as_matrix(), T.as_matrix())


def test_the_restatements_jacobians_at_zero_residual():
    """The first-order form J_i = -W Ad(S_j S_i^-1), J_j = W drops the inverse left Jacobian of the logarithm: it is exact only
    where the residual is zero, so the central differences are taken there."""
    V, held, edges = gs.random_graph(4, [(0, 1), (2, 1), (1, 3)], (0,), 4, stiffness=True, noise=0.)
    assert np.abs(sg.residuals(V, edges)).max() <= 1e-14
    eps = 1e-6
    for e in edges:
        _, J1, J2, _ = sg.scaled_edge(V, e)
        for which, J in ((e[0], J1), (e[1], J2)):
            num = np.zeros((7, 7))
            for k in range(7):
                d = np.zeros(7)
                d[k] = eps
                plus, minus = list(V), list(V)
                plus[which], minus[which] = Sim3.exp(d).dot(V[which]), Sim3.exp(-d).dot(V[which])
                num[:, k] = (sg.residuals(plus, [e])[0] - sg.residuals(minus, [e])[0]) / (2. * eps)
            assert np.abs(num - J).max() <= 1e-8 * max(1., np.abs(J).max()), np.abs(num - J).max()
    # away from zero the form is first order only
    Vn, _, en = gs.random_graph(4, [(0, 1)], (0,), 4, noise=0.3)
    assert np.abs(sg.residuals(Vn, en)).max() > 0.1


def test_linearise_handles_held_vertices_losses_and_absent_rows():
    from pyslam_amd.losses import HuberLoss
    cases = gs.linearise_cases()
    V, held, edges, _ = cases['held_pair']
    H, g, c = sg.linearise(V, edges, held)
    assert H.shape == (28, 28) and np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
    only_free = [e for e in edges if not (held[e[0]] and held[e[1]])]
    H2, g2, c2 = sg.linearise(V, only_free, held)
    assert np.array_equal(H, H2) and np.array_equal(g, g2) and c > c2 > 0.      # an edge between two held vertices: cost only
    V, held, edges, _ = cases['stiffness']
    rs, J1, J2, _ = sg.scaled_edge(V, edges[2])
    assert rs[4] == 0. and not J1[4].any() and not J2[4].any() and J1[3].any()
    V, held, edges, loss = cases['huber']
    r = sg.residuals(V, edges)
    assert (np.abs(r) > loss.k).any() and (np.abs(r) < loss.k).any()
    assert abs(sg.cost(V, edges, loss) - HuberLoss(loss.k).loss(r).sum()) <= 1e-12
    H, g, c = sg.linearise(V, edges, held, loss)
    Hl2 = sg.linearise(V, edges, held)[0]
    assert np.trace(H) < np.trace(Hl2)
    with pytest.raises(ValueError, match='at least one vertex must be held'):
        sg.linearise(V, edges, np.zeros(len(V), dtype=bool))
    for name, (V, held, edges, loss) in cases.items():
        H = sg.linearise(V, edges, held, loss)[0]
        assert H.shape[0] == 7 * int((~held).sum()) and np.linalg.eigvalsh(H).min() > 0., name


def test_the_restatement_converges_to_the_truth():
    for case, (N, p) in enumerate(gs.SOLVE_CASES):
        truth, start, held, edges, V, hist, its = gs.solve_reference(case)
        assert len(edges) == N + N // 5 and held.tolist() == [True] + [False] * (N - 1)
        assert max(np.abs(sg.residuals(truth, edges)).max(), sg.cost(truth, edges)) <= 1e-13      # every edge is exact
        gap, gap0 = gs.vertex_gap(V, truth), gs.vertex_gap(start, truth)
        cond = np.linalg.cond(sg.linearise(truth, edges, held)[0])
        print('{} vertices, perturbation {}: {} iterations, truth to {:.2e} (start {:.2e}), cond(H) {:.2e}, costs {}'.format(
            N, p, its, gap, gap0, cond, ['{:.2e}'.format(c) for c in hist]))
        assert its <= 8 and gap <= 1e-10 and gap0 > 0.5 * p and len(hist) == its + 1
    again = synthetic.sim3_graph(12, 2, 0, 0.05)
    assert gs.vertex_gap(again[1], gs.solve_reference(0)[1]) == 0.                                  # the generator is deterministic
    assert len({round(S.scale, 6) for S in again[0]}) > 6                                         # varying scale


def test_the_drift_scene_is_corrected_by_the_restatement_alone():
    d, graph, old, new, poses, scales, points, hist, its = gs.drift_reference()
    K = gs.DRIFT['num_keyframes']
    assert d['poses_est'].shape == (K, 4, 4) and len(graph.edges) == K and graph.held == [True] + [False] * (K - 1)
    e, k, s, T_21 = d['closure']
    assert (e, k) == (0, K - 1) and abs(s - 1.01 ** (K - 1)) <= 1e-12
    # the closure is exact: the true poses at their local scales satisfy it
    true = [Sim3.from_se3(T, sc) for T, sc in zip(d['poses_true'], d['scales'])]
    true = [Sim3(S.rot, S.trans * S.scale, S.scale) for S in true]       # camera frame k in units of its local map
    assert np.abs(true[k].dot(true[e].inv()).as_matrix() - Sim3.from_se3(T_21, s).as_matrix()).max() <= 1e-12
    before, after = gs.centre_rmse(d['poses_est'], d['poses_true']), gs.centre_rmse(poses, d['poses_true'])
    p_before = float(np.sqrt(((d['points_est'] - d['points_true']) ** 2).sum(axis=1).mean()))
    p_after = float(np.sqrt(((points - d['points_true']) ** 2).sum(axis=1).mean()))
    print('drift loop, {} keyframes: centre RMSE {:.3f} -> {:.3f} ({:.1f}x), landmark RMSE {:.3f} -> {:.3f}, {} iterations, costs {}'.format(
        K, before, after, before / after, p_before, p_after, its, ['{:.3e}'.format(c) for c in hist]))
    assert before / after >= 5. and p_before / p_after >= 5.
    assert abs(scales[0] - 1.) == 0. and scales[-1] > 1.3                  # the last vertex took up the drift


def stand_in(monkeypatch):
    """``Sim3PoseGraph.solve`` with the restatement in place of the device call (the device path: tests/test_gpu_sim3graph.py)."""
    def solve(self, options=None):
        self._check()
        V, hist, its = sg.solve(self.vertices, self.edges, np.array(self.held), self.loss, options)
        self.vertices, self.cost_history, self.iterations = V, hist, its
        return V
    monkeypatch.setattr(pg.Sim3PoseGraph, 'solve', solve)


def test_correct_loop_leaves_a_consistent_map_alone_and_moves_points_with_their_owner(monkeypatch):
    stand_in(monkeypatch)
    d = synthetic.sim3_drift_loop(num_keyframes=12, seed=3)
    P = d['poses_est']
    consistent = (0, 11, 1.0, P[11] @ np.linalg.inv(P[0]))     # scale 1, T_21 the actual relative pose
    poses, scales, pts = pg.correct_loop(P, [consistent], extra_edges=[(0, 5), (3, 9), (4, 5)], landmark_owner=d['owner'],
                                         points_w=d['points_est'])
    assert pg.correct_loop.last_graph.iterations >= 1 and len(pg.correct_loop.last_graph.edges) == 11 + 2 + 1
    assert np.abs(poses - P).max() <= 1e-9 and np.abs(scales - 1.).max() <= 1e-9 and np.abs(pts - d['points_est']).max() <= 1e-9
    # the real closure: every point keeps its coordinates in its owner's camera frame, up to the owner's scale
    as_objects = [SE3.from_matrix(T, normalize=True) for T in P]
    poses, scales, pts = pg.correct_loop(as_objects, [d['closure']], landmark_owner=d['owner'], points_w=d['points_est'])
    assert isinstance(poses[0], SE3) and scales[-1] > 1.05 and np.abs(pts - d['points_est']).max() > 0.1
    for k in (1, 6, 11):
        sel = d['owner'] == k
        before = d['points_est'][sel] @ P[k][:3, :3].T + P[k][:3, 3]
        after = poses[k].dot(pts[sel])
        assert np.abs(after * scales[k] - before).max() <= 1e-10
    only_poses = pg.correct_loop(P, [d['closure']])
    assert only_poses[2] is None and np.abs(only_poses[0] - np.stack([T.as_matrix() for T in poses])).max() <= 1e-12


def test_argument_errors_exports_and_shims(monkeypatch):
    import liegroups
    import pyslam.pipelines
    import pyslam.pipelines.posegraph as shim
    import pyslam_amd.liegroups as lg
    import pyslam_amd.pipelines as pp
    assert liegroups.Sim3 is Sim3 is lg.Sim3 and 'Sim3' in lg.__all__ and 'Sim3' in liegroups.__all__
    assert shim.Sim3PoseGraph is pg.Sim3PoseGraph is pp.Sim3PoseGraph and shim.correct_loop is pg.correct_loop is pp.correct_loop
    assert pyslam.pipelines.Sim3PoseGraph is pg.Sim3PoseGraph
    assert {'Sim3PoseGraph', 'correct_loop'} <= set(pg.__all__)
    with pytest.raises(ValueError, match='scale must be positive'):
        Sim3(SO3.identity(), np.zeros(3), 0.)
    with pytest.raises(ValueError, match='Invalid similarity matrix'):
        Sim3.from_matrix(np.ones((4, 4)))
    g = pg.Sim3PoseGraph()
    with pytest.raises(ValueError, match='no vertex'):
        g.solve()
    a, b = g.add_vertex(Sim3.identity()), g.add_vertex(SE3.identity())
    assert (a, b) == (0, 1) and isinstance(g.vertices[1], Sim3)
    with pytest.raises(ValueError, match='index out of range'):
        g.add_edge(0, 2, Sim3.identity())
    with pytest.raises(ValueError, match='two different vertices'):
        g.add_edge(1, 1, Sim3.identity())
    with pytest.raises(ValueError, match='7 x 7'):
        g.add_edge(0, 1, Sim3.identity(), stiffness=np.identity(6))
    with pytest.raises(ValueError, match='Sim3, an SE3 or a 4 x 4'):
        g.add_vertex(np.identity(3))
    g.add_edge(0, 1, np.identity(4))
    with pytest.raises(ValueError, match='at least one vertex must be held'):
        g.solve()
    big = pg.Sim3PoseGraph()
    big.vertices, big.held = [Sim3.identity()] * (pg.MAX_FREE_VERTICES + 2), [True] + [False] * (pg.MAX_FREE_VERTICES + 1)
    with pytest.raises(ValueError, match='8192 unknowns'):
        big.solve()
    V, held, i, j, obs, W = g.tables()
    assert V.shape == (2, 13) and obs.shape == (1, 13) and W is None and i.dtype == np.int32 and V[0, 12] == 1.

    class Mine:
        LOSS_ID, k = 3, 1.
    g.held[0], g.loss = True, Mine()
    with pytest.raises(ValueError, match='only the built-in losses'):
        pg._loss_id_k(g.loss)
    P = np.tile(np.identity(4), (3, 1, 1))
    for kw, match in ((dict(closures=[]), 'no closure'), (dict(closures=[(0, 3, 1., np.identity(4))]), 'does not join'),
                      (dict(closures=[(0, 2, 1., np.identity(4))], held=()), 'held must name'),
                      (dict(closures=[(0, 2, 1., np.identity(4))], extra_edges=[(1, 1)]), 'extra edge')):
        with pytest.raises(ValueError, match=match):
            pg.correct_loop(P, **kw)
    with pytest.raises(ValueError, match='at least two keyframes'):
        pg.correct_loop(P[:1], [(0, 0, 1., np.identity(4))])
    stand_in(monkeypatch)
    with pytest.raises(ValueError, match='one keyframe per point'):
        pg.correct_loop(P, [(0, 2, 1., np.identity(4))], landmark_owner=[0], points_w=np.zeros((2, 3)))


def test_the_pipeline_switch_defaults_to_off():
    from pyslam_amd.pipelines.mono import SparseMonoPipeline
    src = open(os.path.join(REPO, 'pyslam_amd', 'pipelines', 'mono.py')).read()
    assert 'self.loop_correction = False' in src and 'self.loop_corrections = []' in src and 'self.loop_min_shared' in src
    assert callable(SparseMonoPipeline.correct_loop_closure) and callable(SparseMonoPipeline.covisibility_edges)


def test_the_c_abi_and_the_source_layout():
    from pyslam_amd import _native as nat
    names = ('ps_sim3pg_create', 'ps_sim3pg_destroy', 'ps_sim3pg_set_vertices', 'ps_sim3pg_get_vertices', 'ps_sim3pg_eval_cost',
             'ps_sim3pg_linearize', 'ps_sim3pg_iteration', 'ps_sim3pg_solve', 'ps_sim3pg_debug_edges', 'ps_sim3pg_debug_explog',
             'ps_sim3pg_profile')
    header = open(os.path.join(REPO, 'include', 'pyslam_hip.h')).read()
    src = open(os.path.join(REPO, 'pyslam_amd', 'csrc', 'ps_abi_sim3pg.h')).read()
    for name in names:
        decl = re.search(r'\bint ' + name + r'\((.*?)\);', header, re.S).group(1)
        defn = re.search(r'\nint ' + name + r'\((.*?)\) \{', src, re.S).group(1)
        assert name in nat.SIGNATURES, name
        assert len(decl.split(',')) == len(defn.split(',')) == len(nat.SIGNATURES[name][1]), name
        assert re.sub(r'\s+', ' ', decl) == re.sub(r'\s+', ' ', defn), name
    core = open(os.path.join(REPO, 'pyslam_amd', 'csrc', 'ps_core.hip')).read()
    assert core.index('#include "ps_k_sim3.h"') < core.index('#include "ps_k_sim3pg.h"')
    assert core.index('#include "ps_abi_sim3.h"') < core.index('#include "ps_host_sim3pg.h"') < core.index('#include "ps_abi_sim3pg.h"')
    import __graft_entry__ as g
    assert {'ps_k_sim3pg.h', 'ps_host_sim3pg.h', 'ps_abi_sim3pg.h'} <= set(os.listdir(os.path.dirname(g.SRC)))   # the build hash covers csrc/
    kern = open(os.path.join(REPO, 'pyslam_amd', 'csrc', 'ps_k_sim3pg.h')).read()
    assert re.search(r'atomic\w*\s*\(', kern, re.I) is None     # no atomic call: every sum in a fixed order
    for k in ('k_s3g_edges', 'k_s3g_assemble', 'k_s3g_retract', 'k_s3g_sum'):
        assert re.search(r'__global__ __launch_bounds__\(256\) void ' + k + r'\(', kern), k
    for fn in ('sim3_exp(', 'sim3_log(', 'sim3_adj('):
        assert 'PS_DEV' in kern and fn in kern, fn
    host = open(os.path.join(REPO, 'pyslam_amd', 'csrc', 'ps_host_sim3pg.h')).read()
    for call in ('bchol_chain(', 'BCHOL_FACTOR', 'k_spd_subst', 'k_spd_residual', 'k_spd_axpy'):
        assert call in host, call
    assert 'ps_stop_step(' in src and 'PS_SPD_MAXN' in src
