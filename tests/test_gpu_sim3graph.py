"""Sim(3) pose graph on the device (csrc/ps_k_sim3pg.h, ps_host_sim3pg.h, ps_abi_sim3pg.h; pyslam_amd/pipelines/posegraph.py) against
its numpy restatement (pyslam_amd/pipelines/simgraph.py, pyslam_amd/liegroups/sim3.py).

Bounds.  Blocks (r~, J~), the normal equations (H, g), the cost and the first step carry the margins tests/test_gpu_parity.py
already uses for them: TOL_BLOCK 1e-12, TOL_COST 1e-10 (with its rounding term in units of the previous cost, over the entries
above 1e-9 of the start cost) and TOL_DX 1e-8.  New here: the device's exp / log / adjoint against ``Sim3`` over
sim3graph_scenes.tangents() -- observed on an MI355X: exp 4.44e-16, log(exp) 1.36e-15, adjoint 7.25e-16 (relative to max(1, largest
entry)); bound: 8 x those (sim3graph_scenes.EXPLOG_OBSERVED, EXPLOG_FACTOR).  Observed beside the borrowed margins, the largest over
all cases: r~ 7.6e-15, J~ 8.1e-16, H 1.7e-15, g 1.6e-14, cost 1.6e-15 (against 1e-12 / 1e-10); step 7.9e-13 at lambda 0 and 8.7e-14 at
1e-3, relative residual of the linear solve 6.2e-15 (against 1e-8 / 1e-12); cost histories 1.0e-12 (against 1e-10); the drift scene's
poses, scales and points 1.2e-14 (against 1e-9); the truth of the three solve cases to 2.9e-15 (against the issue's 1e-10)."""
import numpy as np
import pytest

import sim3graph_scenes as gs
from conftest import rel_err
from test_gpu_parity import TOL_BLOCK, TOL_COST, TOL_DX
from pyslam_amd import _native as nat
from pyslam_amd.liegroups import SE3, Sim3
from pyslam_amd.pipelines import posegraph as pg
from pyslam_amd.pipelines import simgraph as sg
from pyslam_amd.problem import Options

pytestmark = pytest.mark.gpu


def device(V, held, edges, loss=None):
    return pg.DeviceSim3Graph(*gs.tables(V, held, edges), loss=loss)


def history_close(hist, ref):
    """tests/test_gpu_parity.py's rule for a cost history."""
    hist, ref = np.asarray(hist), np.asarray(ref)
    big = ref > 1e-9 * ref[0]
    prev = np.concatenate([[ref[0]], ref[:-1]])
    gap = np.abs(hist - ref)
    assert np.all(gap[big] <= TOL_COST * np.abs(ref[big]) + 1e-15 * prev[big]), gap / np.abs(ref)
    assert np.all(hist[~big] <= 1e-9 * ref[0])
    return float((gap[big] / np.abs(ref[big])).max())


def test_exp_log_and_adjoint_of_the_device():
    xis = gs.tangents()
    S13, back, adj = pg.debug_explog(xis)
    worst = dict(exp=0., log=0., adj=0.)
    for xi, row, b, a in zip(xis, S13, back, adj):
        S = Sim3.exp(xi)
        ref = pg.pack13(S)
        worst['exp'] = max(worst['exp'], np.abs(row - ref).max() / max(1., np.abs(ref).max()))
        worst['log'] = max(worst['log'], np.abs(b - S.log()).max() / max(1., np.abs(xi).max()))
        A = S.adjoint()
        worst['adj'] = max(worst['adj'], np.abs(a - A).max() / max(1., np.abs(A).max()))
    print('device exp / log / adjoint against Sim3 over {} tangent vectors: {}'.format(
        xis.shape[0], {k: '{:.2e}'.format(v) for k, v in worst.items()}))
    for k, v in worst.items():
        assert v <= gs.EXPLOG_FACTOR * gs.EXPLOG_OBSERVED[k], (k, v)
    # the zeros are exact
    S0, b0, a0 = pg.debug_explog(np.zeros((1, 7)))
    assert np.array_equal(S0[0], pg.pack13(Sim3.identity())) and not b0.any() and np.array_equal(a0[0], np.identity(7))


@pytest.mark.parametrize('name', sorted(gs.linearise_cases()))
def test_tap_normal_equations_and_cost(name):
    V, held, edges, loss = gs.linearise_cases()[name]
    dev = device(V, held, edges, loss)
    try:
        r, J1, J2 = dev.debug_edges()
        ref = [sg.scaled_edge(V, e, loss) for e in edges]
        fig = dict(r=rel_err(r, np.array([x[0] for x in ref])), J1=rel_err(J1, np.array([x[1] for x in ref])),
                   J2=rel_err(J2, np.array([x[2] for x in ref])))
        H, g, c = dev.linearize(0.)
        Ho, go, co = sg.linearise(V, edges, held, loss)
        fig.update(H=rel_err(H, Ho), g=rel_err(g, go), cost=abs(c - co) / co)
        print('{} ({} edges, n = {}): {}'.format(name, len(edges), dev.n, {k: '{:.2e}'.format(v) for k, v in fig.items()}))
        assert max(fig['r'], fig['J1'], fig['J2'], fig['H'], fig['g']) < TOL_BLOCK and fig['cost'] <= TOL_COST
        assert np.array_equal(H, H.T)                                    # mirrored in the same order: symmetric to the bit
        assert dev.eval_cost() == c                                      # the same fixed-order sum
        lam = 1e-3
        Hd, gd, _ = dev.linearize(lam)
        assert np.array_equal(gd, g) and np.array_equal(Hd - np.diag(np.diag(Hd)), H - np.diag(np.diag(H)))
        assert np.array_equal(np.diag(Hd), np.diag(H) * (1. + lam))
        for lam in (0., 1e-3):                                           # one step against the restatement's system
            dev.set_vertices(gs.tables(V, held, edges)[0])
            cost_after, dxn, relres = dev.iteration(lam)
            new, dx, c_ref = sg.iterate(V, edges, held, loss, lam)
            got = gs.unpack(dev.get_vertices())
            step = np.concatenate([S.dot(O.inv()).log() for S, O, h in zip(got, V, held) if not h])
            err = rel_err(step, dx)
            print('    lambda {}: step {:.2e}, ||dx|| {:.2e}, relres {:.1e}, cost after {:.2e}'.format(
                lam, err, abs(dxn - np.linalg.norm(dx)) / np.linalg.norm(dx), relres, abs(cost_after - c_ref) / c_ref))
            assert err < TOL_DX and abs(dxn - np.linalg.norm(dx)) <= TOL_DX * np.linalg.norm(dx) and relres <= 1e-12      # (the core's own tolerance for a linear solve)
            assert abs(cost_after - c_ref) <= TOL_COST * c_ref + 1e-15 * c
            assert all(np.array_equal(pg.pack13(a), pg.pack13(b)) for a, b, h in zip(got, V, held) if h)      # held vertices stay
    finally:
        dev.close()


@pytest.mark.parametrize('case', range(len(gs.SOLVE_CASES)))
def test_solve_reaches_the_truth_as_the_restatement_does(case):
    truth, start, held, edges, V_ref, hist_ref, its_ref = gs.solve_reference(case)
    dev = device(start, held, edges)
    try:
        hist, its, dxn = dev.solve(gs.solve_options())
        V = gs.unpack(dev.get_vertices())
        gap = gs.vertex_gap(V, truth)
        print('{}: {} iterations (restatement {}), truth to {:.2e}, costs {}'.format(gs.SOLVE_CASES[case], its, its_ref, gap,
                                                                                    ['{:.2e}'.format(c) for c in hist]))
        assert its == its_ref and len(hist) == len(hist_ref) and gap <= 1e-10
        print('    cost history against the restatement: {:.2e}'.format(history_close(hist, hist_ref)))
        # the same solve again: bit-identical
        dev.set_vertices(gs.tables(start, held, edges)[0])
        hist2, its2, _ = dev.solve(gs.solve_options())
        assert its2 == its and np.array_equal(hist2, hist) and np.array_equal(dev.get_vertices(), np.array([pg.pack13(S) for S in V]))
    finally:
        dev.close()


def test_the_drift_scene_as_the_restatement_corrects_it():
    d, graph, old, new_ref, poses_ref, scales_ref, points_ref, hist_ref, its_ref = gs.drift_reference()
    poses, scales, points = pg.correct_loop(d['poses_est'], [d['closure']], landmark_owner=d['owner'], points_w=d['points_est'])
    run = pg.correct_loop.last_graph
    gap = max(np.abs(poses - poses_ref).max(), np.abs(scales - scales_ref).max(), np.abs(points - points_ref).max())
    print('drift loop on the device: {} iterations (restatement {}), poses, scales and points against the restatement {:.2e}, '
          'centre RMSE {:.3f} -> {:.3f}'.format(run.iterations, its_ref, gap, gs.centre_rmse(d['poses_est'], d['poses_true']),
                                                gs.centre_rmse(poses, d['poses_true'])))
    assert run.iterations == its_ref and gap <= 1e-9                    # SURVEY 8d's margin for final poses and landmarks
    history_close(run.cost_history, hist_ref)
    assert gs.centre_rmse(d['poses_est'], d['poses_true']) >= 5. * gs.centre_rmse(poses, d['poses_true'])


def test_errors_leave_a_handle_that_can_be_destroyed():
    V, held, edges, _ = gs.linearise_cases()['held_middle']
    tabs = gs.tables(V, held, edges)
    with pytest.raises(nat.NativeError, match='no held vertex'):
        pg.DeviceSim3Graph(tabs[0], np.zeros(len(V), dtype=bool), *tabs[2:])
    bad = tabs[2].copy()
    bad[1] = len(V)
    with pytest.raises(nat.NativeError, match='out of range'):
        pg.DeviceSim3Graph(tabs[0], tabs[1], bad, *tabs[3:])
    with pytest.raises(nat.NativeError, match='i == j'):
        pg.DeviceSim3Graph(tabs[0], tabs[1], tabs[3], tabs[3], tabs[4])
    nan = tabs[0].copy()
    nan[1, 10] = np.nan
    with pytest.raises(nat.NativeError, match='not finite'):
        pg.DeviceSim3Graph(nan, *tabs[1:])
    many = np.tile(tabs[0][:1], (pg.MAX_FREE_VERTICES + 2, 1))
    with pytest.raises(nat.NativeError, match='at most 8192'):
        pg.DeviceSim3Graph(many, np.arange(many.shape[0]) == 0, tabs[2], tabs[3], tabs[4])
    # an indefinite system: every edge on free vertex 4 carries a zero stiffness
    W = np.stack([np.zeros((7, 7)) if 4 in (e[0], e[1]) else np.identity(7) for e in edges])
    dev = pg.DeviceSim3Graph(*tabs[:5], stiffness=W)
    try:
        before = dev.get_vertices()
        with pytest.raises(nat.NativeError, match='not positive definite to rounding'):
            dev.iteration(0.)
        assert np.array_equal(dev.get_vertices(), before)              # nothing moved
        with pytest.raises(nat.NativeError, match='not positive definite to rounding'):
            dev.solve()
        assert np.isfinite(dev.eval_cost())                            # the handle still answers
    finally:
        dev.close()
    with pytest.raises(nat.NativeError, match='null'):
        nat.check(nat.load().ps_sim3pg_eval_cost(None, None))


def test_the_public_graph_and_correct_loop():
    truth, start, held, edges, V_ref, hist_ref, its_ref = gs.solve_reference(0)
    g = pg.Sim3PoseGraph()
    for S, h in zip(start, held):
        g.add_vertex(S, held=bool(h))
    for e in edges:
        g.add_edge(*e)
    V = g.solve(gs.solve_options())
    assert V is g.vertices and isinstance(V[0], Sim3) and g.iterations == its_ref and len(g.cost_history) == its_ref + 1
    assert gs.vertex_gap(V, truth) <= 1e-10
    # the default options stop earlier, by the cost threshold
    g2 = pg.Sim3PoseGraph()
    for S, h in zip(start, held):
        g2.add_vertex(S, held=bool(h))
    for e in edges:
        g2.add_edge(*e)
    from pyslam_amd.losses import HuberLoss
    g2.loss = HuberLoss(1.0)
    g2.solve()
    assert 1 <= g2.iterations <= its_ref and g2.cost_history[-1] < Options().min_cost and gs.vertex_gap(g2.vertices, truth) <= 1e-5
    # a closure the map already satisfies moves nothing
    from pyslam_amd import synthetic
    d = synthetic.sim3_drift_loop(num_keyframes=12, seed=3)
    P = d['poses_est']
    poses, scales, pts = pg.correct_loop(P, [(0, 11, 1.0, P[11] @ np.linalg.inv(P[0]))], extra_edges=[(0, 5), (3, 9)],
                                         landmark_owner=d['owner'], points_w=d['points_est'])
    assert np.abs(poses - P).max() <= 1e-9 and np.abs(scales - 1.).max() <= 1e-9 and np.abs(pts - d['points_est']).max() <= 1e-9


def test_the_monocular_pipeline_with_loop_correction():
    import loop_scenes as ls
    import mono_scenes as ms
    from pyslam_amd.pipelines.mono import SparseMonoPipeline
    images = ls.out_and_back()                                 # the sequence of tests/test_gpu_loop.py: queries, no closure

    def run(correction):
        p = SparseMonoPipeline(ms.camera(ms.sequence()['cam']))
        p.local_ba = False
        p.loop_detection, p.loop_correction, p.loop_gap = True, correction, ls.LOOP_GAP
        np.random.seed(ms.PIPELINE_SEED)
        for im in images:
            p.track(im)
        return p
    on, off = run(True), run(False)
    try:
        # no closure on this short sequence: the switch changes nothing, bit for bit
        assert on.loop_closures == [] and on.loop_corrections == [] and len(on.keyframes) == len(off.keyframes) >= 4
        assert len(on.loop_queries) == len(off.loop_queries) > 0
        for a, b in zip(on.T_c_w, off.T_c_w):
            assert (a is None) == (b is None) and (a is None or a.as_matrix().tobytes() == b.as_matrix().tobytes())
        for a, b in zip(on.keyframes, off.keyframes):
            assert a.T_c_w.as_matrix().tobytes() == b.T_c_w.as_matrix().tobytes() and np.array_equal(a.landmark, b.landmark)
        assert on.points_w.tobytes() == off.points_w.tobytes() and np.array_equal(on.alive, off.alive)
        assert on.keyframe_frames == off.keyframe_frames and len(on.keyframe_frames) == len(on.keyframes)
        K = len(on.keyframes)
        assert all(np.array_equal(on.keyframes[k].image, images[f]) for k, f in enumerate(on.keyframe_frames))
        extra = on.covisibility_edges()
        assert extra and all(0 <= i < j < K for i, j in extra)
        owner = on.landmark_owners()
        assert owner.shape == (on.points_w.shape[0],) and owner.min() == 0 and owner.max() < K
        # a fabricated closure the map already satisfies: nothing moves
        T = [kf.T_c_w.as_matrix() for kf in on.keyframes]
        frames_before = [None if t is None else t.as_matrix() for t in on.T_c_w]
        pts_before = on.points_w.copy()
        rel = SE3.from_matrix(T[K - 1] @ np.linalg.inv(T[0]), normalize=True)
        on.correct_loop_closure(dict(keyframe=K - 1, entry=0, scale=1.0, T_21=rel))
        rec = on.loop_corrections[-1]
        gap = max(np.abs(kf.T_c_w.as_matrix() - t).max() for kf, t in zip(on.keyframes, T))
        gap = max(gap, np.abs(on.points_w - pts_before).max(),
                  max(np.abs(a.as_matrix() - b).max() for a, b in zip(on.T_c_w, frames_before) if b is not None))
        print('consistent closure over {} keyframes, {} edges ({} covisibility): everything stays to {:.2e}'.format(
            K, rec['edges'], rec['covisibility'], gap))
        assert gap <= 1e-9 and np.abs(rec['scales'] - 1.).max() <= 1e-9 and rec['edges'] >= K
        # a closure that asks for the scale 1.1: the closing keyframe's vertex moves towards it
        rel2 = SE3.from_matrix(T[K - 1] @ np.linalg.inv(T[0]), normalize=True)
        rel2.trans = 1.1 * rel2.trans
        on.correct_loop_closure(dict(keyframe=K - 1, entry=0, scale=1.1, T_21=rel2))
        rec = on.loop_corrections[-1]
        print('closure scale 1.1: vertex scales {}, {} iterations'.format(np.round(rec['scales'], 4).tolist(), rec['iterations']))
        assert len(on.loop_corrections) == 2 and rec['keyframe'] == K - 1 and rec['entry'] == 0 and rec['iterations'] >= 1
        assert rec['scales'][0] == 1. and 1.0 < rec['scales'][-1] <= 1.1 + 1e-9 and rec['cost_history'][-1] < rec['cost_history'][0]
        assert np.abs(on.points_w - pts_before).max() > 1e-6 and all(isinstance(t, SE3) for t in on.T_c_w if t is not None)
    finally:
        on.matcher.close()
        off.matcher.close()
