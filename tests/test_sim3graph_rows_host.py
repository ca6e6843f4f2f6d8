"""CPU side of the per-row Sim(3) pose-graph tests: the long-double definition (tests/longdouble_sim3graph.py) against mpmath, its fp64
twin against the restatement (pyslam_amd/pipelines/simgraph.py, pyslam_amd/liegroups/sim3.py), what the scenes
(tests/sim3graph_row_scenes.py) claim, the reference's own error e64 per scene, and L1's capped weight on the restatement.

e64 by the reference alone (fp64 twin against long double on the same input, over the scene and its one-ulp copies; the device's bound
is max(1e-12, 8 e64)).  Every scene sits on the floor (8 e64 <= 1e-12) except, with the reason:
  angles      r~ 1.1e-12, g 4.2e-13: the edge at 3.1415 rad.  vee(R - R^T) has the length 2 sin(theta) = 1.9e-4 there and carries the
              2^-53 of the product S_j S_i^-1 S_ji^-1 absolutely: 2^-53 / sin(theta) = 1.2e-12 of the direction of phi.
  l1_zero     r~ 4.2e-12, g 4.1e-12: the capped L1 rows.  r is rounding noise (1e-15 of translations of 10), s = sqrt(1e8) = 1e4
              hands it to r~ at 1e-11, beside a rounding scale u of 10.
  many_edges  g 9.2e-14 (on the floor, the nearest to it): a vector of g sums 4 000 edges of one sign pattern.
The rows under L1 away from zero (rows-L1-*) reach 2e-14 (J~) and 4e-14 (H): 1 / |r_k| hands a component's relative error to its row.
map_scales was narrowed for its cost (sim3graph_row_scenes._map_scales)."""
import numpy as np
import pytest

import longdouble_sim3graph as ld
import sim3graph_row_scenes as rs
import sim3graph_scenes as gs
from pyslam_amd import losses
from pyslam_amd.liegroups import Sim3
from pyslam_amd.pipelines import posegraph as pg
from pyslam_amd.pipelines import simgraph as sg
from pyslam_amd.problem import Options

pytestmark = pytest.mark.skipif(not ld.LONGDOUBLE_OK, reason=ld.LONGDOUBLE_SKIP)

LD = ld.LD
U64 = 2. ** -64
EPS = ld.EPS
# where the reference alone leaves the 1e-12 floor (module docstring): scene -> quantities
OFF_FLOOR = dict(angles=('rt', 'g'), l1_zero=('rt', 'g'))


def loss_object(g):
    if g.loss_id == ld.L2:
        return None
    cls = (None, losses.L1Loss, losses.CauchyLoss, losses.HuberLoss, losses.TukeyLoss, losses.TDistributionLoss)[g.loss_id]
    return cls() if g.loss_id == ld.L1 else cls(g.loss_k)


def as_objects(g):
    """(vertices, edges) of a Graph as simgraph takes them."""
    V = [pg.unpack13(row) for row in g.V13]
    edges = [(int(i), int(j), pg.unpack13(o), None if g.stiffness is None else g.stiffness[e])
             for e, (i, j, o) in enumerate(zip(g.ei, g.ej, g.obs13))]
    return V, edges


# ---------------------------------------------------------------------------
# 1. the long-double definition against mpmath
# ---------------------------------------------------------------------------
THETAS = (0., 1e-12, 1e-10, 0.9e-8, 1.1e-8, 1e-6, 1e-4, 1e-2, 0.3, 0.999, 1.0, 1.001, 2., 3., 3.14159)
SIGMAS = (0.,) + tuple(s * v for v in (1e-12, 1e-9, 1e-5, 1e-2, 0.3, 0.999, 1.0, 1.001, 3., 20.) for s in (1., -1.))


def test_the_long_double_coefficients_exp_and_log_against_mpmath():
    """A, B, C over THETAS x SIGMAS, exp over gs.tangents() and the scenes' angles against mpmath at 50 digits (the coefficients from
    f = (e^z - 1) / z formed at 120 digits; exp from mpmath.expm of the 4 x 4 generator), log as the inverse of that exp.

    Bound: 4 x 2^-64 relative for the coefficients, plus the small branch's own truncation where theta <= 1e-8 lies OUTSIDE the
    unit circle: there the definition says h1 = 1, h2 = 1 / 2 for sin(theta) / theta = 1 - theta^2 / 6 + ... and (1 - cos(theta)) /
    theta^2 = 1 / 2 - theta^2 / 24 + ..., which moves B by at most (|sigma| E theta^2 / 6 + E theta^4 / 24) / |z|^2 and C by at most
    (|sigma| E theta^2 / 24 + E theta^2 / 6) / |z|^2, E = e^sigma (7.7e-17 of C at theta = 0.9e-8, sigma = -1.001).  exp: 4 x 2^-64
    of max(1, its largest entry) per entry plus theta^3 / 6 (R) and the same coefficient terms times |rho| (t).  log(exp(xi)) = xi
    to 8 x 2^-64 max(1, |xi|), plus the same truncation terms; beyond pi / 2 divided by sin(theta) (3.1415: 9.3e-5): the direction of
    phi is read from vee(R - R^T), whose length 2 sin(theta) carries the rounding of R absolutely."""
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 50

    def exact(x):                                  # a long double as an mpf, exactly
        hi = float(x)
        return mp.mpf(hi) + mp.mpf(float(x - LD.type(hi)))

    def coefficients(th, sg_):
        with mp.workdps(120):
            th, s = mp.mpf(th), mp.mpf(sg_)
            A = mp.expm1(s) / s if s != 0 else mp.mpf(1)
            if th == 0:
                if s == 0:
                    return A, mp.mpf(1) / 2, mp.mpf(1) / 6
                E = mp.exp(s)
                return A, (E * (s - 1) + 1) / s ** 2, (E * (s * s - 2 * s + 2) - 2) / (2 * s ** 3)
            z = mp.mpc(s, th)
            f = mp.expm1(z) / z
            return A, f.imag / th, (A - f.real) / th ** 2

    grid = [(t, s) for t in THETAS for s in SIGMAS]
    th, sg_ = np.array([g[0] for g in grid]), np.array([g[1] for g in grid])
    (A, B, C), table = ld.two_pass(lambda dt, p: ld.w_coefficients(th.astype(dt), sg_.astype(dt), p, 'w'), LD)
    assert table['w/w_series'].any() and not table['w/w_series'].all() and table['w/closed/h12'].any()
    worst = 0.
    for k, (t, s) in enumerate(grid):
        ref = coefficients(t, s)
        trunc = [0., 0., 0.]
        if t <= 1e-8 and s * s + t * t > 1.:
            E, z2 = np.exp(s), s * s + t * t
            trunc = [0., (abs(s) * E * t * t / 6 + E * t ** 4 / 24) / z2, (abs(s) * E * t * t / 24 + E * t * t / 6) / z2]
        for name, got, r, tr in zip('ABC', (A[k], B[k], C[k]), ref, trunc):
            err = float(abs(exact(got) - r))
            worst = max(worst, (err - tr) / float(abs(r)))
            assert err <= 4 * U64 * float(abs(r)) + tr, (name, t, s, err / float(abs(r)), tr)
    print('A, B, C over {} points: {:.2f} x 2^-64 beyond the truncation term at the worst point'.format(len(grid), worst / U64))

    rng = np.random.default_rng(3)
    xis = np.vstack([gs.tangents()] + [np.hstack([rng.standard_normal(3), a * rs.direction(rng)[0], 0.05]) for a in rs.ANGLES])
    (S13, back, _), table = ld.two_pass(lambda dt, p: (lambda S: (ld.pack(S), ld.log(S, p, 'l'), None))(ld.exp(xis.astype(dt), p, 'x')), LD)
    w_exp, w_log = 0., 0.
    for k, xi in enumerate(xis):
        G = mp.zeros(4, 4)
        x, y, z = (mp.mpf(v) for v in xi[3:6])
        for (r, c), v in {(0, 1): -z, (0, 2): y, (1, 0): z, (1, 2): -x, (2, 0): -y, (2, 1): x}.items():
            G[r, c] = v
        for d in range(3):
            G[d, d] = mp.mpf(xi[6])
            G[d, 3] = mp.mpf(xi[d])
        with mp.workdps(80):
            M = mp.expm(G, method='taylor')
            s = mp.exp(mp.mpf(xi[6]))
        theta, sigma, rho = float(np.linalg.norm(xi[3:6])), float(xi[6]), float(np.abs(xi[:3]).sum())
        ref = [M[r, c] / s for r in range(3) for c in range(3)] + [M[r, 3] for r in range(3)] + [s]
        scale = max(1., max(float(abs(v)) for v in ref))
        trunc_R = theta ** 3 / 6 if theta <= 1e-8 else 0.
        trunc_t = 0.
        if theta <= 1e-8 and sigma * sigma + theta * theta > 1.:
            E, z2 = np.exp(sigma), sigma * sigma + theta * theta
            trunc_t = rho * (theta * (abs(sigma) * E * theta ** 2 / 6 + E * theta ** 4 / 24) / z2
                             + theta ** 2 * (abs(sigma) * E * theta ** 2 / 24 + E * theta ** 2 / 6) / z2)
        for n, (got, r) in enumerate(zip(S13[k], ref)):
            err = float(abs(exact(got) - r))
            w_exp = max(w_exp, err / scale)
            assert err <= 4 * U64 * scale + (trunc_R if n < 9 else trunc_t), (k, n, xi, err)
        if theta >= np.pi:
            continue
        cond = 1. / np.sin(theta) if theta > 0.5 * np.pi else 1.
        err = float(np.abs(back[k] - xi.astype(LD)).max()) / max(1., float(np.abs(xi).max()))
        w_log = max(w_log, err / cond)
        assert err <= 8 * U64 * cond + trunc_R + trunc_t, (k, xi, err)
    print('exp over {} tangent vectors: {:.2f} x 2^-64; log(exp) - xi: {:.2f} x 2^-64 / sin(theta)'.format(len(xis), w_exp / U64, w_log / U64))


# ---------------------------------------------------------------------------
# 2. the fp64 twin against the restatement
# ---------------------------------------------------------------------------
def test_the_twin_group_functions_against_sim3():
    xis = gs.tangents()
    S13, back, adj = ld.explog(xis, np.float64)
    for xi, row, b, a in zip(xis, S13, back, adj):
        S = Sim3.exp(xi)
        ref = pg.pack13(S)
        assert np.abs(row - ref).max() <= 1e-13 * max(1., np.abs(ref).max())
        cond = 1. / np.sin(np.linalg.norm(xi[3:6])) if np.linalg.norm(xi[3:6]) > 3. else 1.
        assert np.abs(b - S.log()).max() <= 1e-13 * cond * max(1., np.abs(xi).max()), xi
        assert np.abs(a - S.adjoint()).max() <= 1e-13 * max(1., np.abs(a).max())


@pytest.mark.parametrize('name', [n for n in rs.ROW_SCENES if n != 'many_edges'])
def test_the_twin_against_the_restatement_per_row(name):
    """1e-13 per row, in the tests' measure; where the reference's own error exceeds that (OFF_FLOOR), two fp64 evaluations of the
    same definition lie within 2 e64 of each other."""
    g, _ = rs.scene(name)
    twin = rs.edge_pairs(name)[0][1]
    e64 = rs.e64(name)
    V, edges = as_objects(g)
    loss = loss_object(g)
    ref = [sg.scaled_edge(V, e, loss) for e in edges]
    u = ld.edge_scale(g)
    for key, rows in rs.classes(twin).items():
        for n, what in enumerate(('rt', 'J1', 'J2')):
            err = ld.row_err(np.array([ref[e][n] for e in rows]), getattr(twin, what)[rows], u[rows])
            assert err <= max(1e-13, 2 * e64[what, key]), (name, what, key, err)
    H, gv, c = sg.linearise(V, edges, g.held, loss)
    Ht, gt, _ = twin.assemble(0.)
    eH, eg = ld.err_system((H, gv), (Ht, gt), twin)
    assert eH <= max(1e-13, 2 * e64['H', 0.]) and eg <= max(1e-13, 2 * e64['g', 0.]), (name, eH, eg)
    if name != 'exact':
        assert abs(c - twin.cost()) <= max(1e-13, 2 * e64['cost']) * c
    assert np.array_equal(np.isfinite(H), np.ones_like(H, dtype=bool))


# ---------------------------------------------------------------------------
# 3. what the scenes claim
# ---------------------------------------------------------------------------
def test_angles_scales_and_units_reach_their_branches():
    g, info = rs.scene('angles')
    ed = rs.edge_pairs('angles')[0][0]
    case = info['case_edges']
    got = np.sqrt((ed.xi[case, 3:6].astype(float) ** 2).sum(axis=1))
    assert np.all(np.abs(got - info['angle']) <= 1e-15 + 2e-12 * info['angle']), got - info['angle']
    assert np.array_equal(ed.small[case], info['angle'] <= 1e-8) and ed.small[case].sum() == 3
    assert np.all(np.abs(ed.xi[case, 6].astype(float) - 0.05) <= 1e-15)
    assert np.all(np.abs(np.sqrt((ed.xi[case, :3].astype(float) ** 2).sum(axis=1)) - 1.) <= 1e-12)

    g, info = rs.scene('scales')
    ed = rs.edge_pairs('scales')[0][0]
    case = info['case_edges']
    assert np.all(np.abs(ed.xi[case, 6].astype(float) - info['sigma']) <= 1e-15 * np.maximum(1., np.abs(info['sigma'])))
    inside = info['sigma'] ** 2 + info['angle'] ** 2 <= 1.
    assert np.array_equal(ed.series[case], inside) and 20 <= inside.sum() <= 40
    tiny = ed.table['edge/log/closed/h12'][case]                    # theta <= 1e-8 outside the circle: the closed forms' small branch
    assert (tiny & ~inside).sum() >= 12 and (~tiny & ~inside).sum() >= 12 and (ed.small[case] & inside).sum() >= 6
    for s in (0.999, -0.999, 1.001, -1.001):
        assert np.array_equal(inside[(info['sigma'] == s) & (info['angle'] <= 1e-8)], [abs(s) < 1.] * 2)

    for name, unit in (('km', 1e3), ('mm', 1e-3)):
        g, info = rs.scene(name)
        ed = rs.edge_pairs(name)[0][0]
        t = np.abs(g.V13[:, 9:12]).max(axis=1)
        assert np.all(t >= 0.05 * unit) and np.all(t <= 20 * unit) and np.all(np.abs(g.obs13[:, 9:12]).max(axis=1) <= 50 * unit)
        assert np.array_equal(ed.small[info['case_edges']], info['angle'] <= 1e-8)
        u = ld.edge_scale(g)
        assert np.all(u >= min(1., unit)) and np.all(u <= 100 * max(1., unit))
    g, info = rs.scene('map_scales')
    ratio = g.V13[g.ej, 12] / g.V13[g.ei, 12]
    assert ratio.max() == 1e6 and ratio.min() == 1e-6 and g.V13[:, 12].min() == 1e-3 and g.V13[:, 12].max() == 1e3
    assert np.abs(g.V13[:, 9:12]).max() <= 10.


def test_the_rounding_scale_holds_the_far_scenes_on_the_floor():
    """u (longdouble_sim3graph.edge_scale; the definition is in tests/test_gpu_sim3graph_rows.py's docstring) is what makes the row
    measure a count of roundings: with it the fp64 twin's rows lie within 64 x 2^-53 on km, mm and map_scales; with a floor of 1 in its
    place the rows of km and map_scales whose residual is mostly cancellation do not."""
    for name in ('km', 'mm', 'map_scales'):
        e = rs.e64(name)
        worst = max(v for k, v in e.items() if isinstance(k, tuple) and k[0] in ('rt', 'J1', 'J2', 'H', 'g'))
        assert worst <= 64 * EPS, (name, worst)
    for name in ('km', 'map_scales'):
        r, t = rs.edge_pairs(name)[0]
        assert ld.row_err(t.rt, r.rt, 1.) > 8 * ld.row_err(t.rt, r.rt, ld.edge_scale(r.g)), name


def test_exact_rows_l1_zero_and_the_workgroup_scenes_are_what_they_say():
    g, _ = rs.scene('exact')
    ed = rs.edge_pairs('exact')[0][0]
    assert float((np.abs(ed.rt).max(axis=1) / ld.edge_scale(g)).max()) <= 32 * EPS         # the inputs' own rounding, nothing else
    # rows: 28 of 140 components beyond k, at most two per edge; Tukey's zero weights are exactly those
    for loss in range(6):
        ed = rs.edge_pairs('rows-{}-identity'.format(ld.LOSS_NAMES[loss]))[0][0]
        beyond = np.abs(ed.r.astype(float)) > rs.K_LOSS
        assert beyond.sum() == 28 and beyond.sum(axis=1).max() <= 2 and np.array_equal(beyond, np.abs(rs.rows_errors()) > rs.K_LOSS)
        if loss in (ld.HUBER, ld.TUKEY):
            assert np.array_equal(ed.inside_k, ~beyond)
        if loss == ld.TUKEY:
            assert np.array_equal(ed.s == 0, beyond) and np.all(ed.J2[beyond] == 0) and np.all(ed.J1[beyond] == 0)
    for kind, rows in (('rotation_only', [3, 4, 5]), ('scale_only', [6]), ('translation_only', [0, 1, 2])):
        ed = rs.edge_pairs('rows-Huber-{}'.format(kind))[0][0]
        assert np.array_equal(np.flatnonzero(ed.present[0]), rows) and np.all(ed.rt[~ed.present] == 0) and np.all(ed.J1[~ed.present] == 0)
        assert rs.definite('rows-L2-{}'.format(kind)) == (kind == 'translation_only')      # (its rows of Ad(S_j S_i^-1) reach all seven columns)
    K = rs.scene('rows-L2-diagonal')[0].stiffness
    assert K[0].diagonal().min() == 1e-3 and K[0].diagonal().max() == 1e3
    # l1_zero: every odometry component at zero (capped), the closure's not
    g, _ = rs.scene('l1_zero')
    ed = rs.edge_pairs('l1_zero')[0][0]
    assert g.E == 12 and np.abs(ed.r[:11].astype(float)).max() <= 2e-14 and ed.l1_capped[:11].all() and not ed.l1_capped[11].all()
    assert np.all(np.isfinite(ed.assemble(0.)[0].astype(float)))
    # wg64: 64 edges, reversed, duplicate and held-ended edges, absent rows at the boundaries of a wave's share, both sides of k
    g, _ = rs.scene('wg64')
    ed = rs.edge_pairs('wg64')[0][0]
    pairs = list(zip(g.ei.tolist(), g.ej.tolist()))
    assert g.E == 64 and any(i > j for i, j in pairs) and len(set(pairs)) < 64 and any((j, i) in pairs for i, j in pairs)
    assert any(g.held[i] and g.held[j] for i, j in pairs) and any(g.held[i] != g.held[j] for i, j in pairs)
    assert sorted(np.flatnonzero(~ed.present.all(axis=1)).tolist()) == list(rs.WG64_ABSENT)
    assert 0.2 <= ed.inside_k[ed.present].mean() <= 0.8
    g, _ = rs.scene('E65')
    assert g.E == 65
    g, _ = rs.scene('many_edges')
    assert g.E == 16448 and -(-g.E // 64) == 257 and g.nfree == 7
    assert np.bincount(np.concatenate([g.rid[g.ei], g.rid[g.ej]]) + 1)[1:].min() > 3000       # items of every diagonal slot
    ed = rs.edge_pairs('many_edges')[0][0]
    assert 0.2 <= ed.inside_k.mean() <= 0.8


def test_hang257_and_noisy_loop():
    g, info = rs.scene('hang257')
    ed = rs.edge_pairs('hang257')[0][0]
    H, gv, _ = ed.assemble(0.)
    assert g.nfree == 257 and 7 * g.nfree == 1799 and np.array_equal(H, np.identity(1799, dtype=LD)) and np.array_equal(gv, -ed.rt.reshape(-1))
    angle = np.sqrt((info['xi'][:, 3:6] ** 2).sum(axis=1))
    assert angle.max() > 3.09 and angle[angle > 0].min() == pytest.approx(1e-9) and len(set(map(tuple, info['xi']))) == gs.tangents().shape[0]
    assert ed.series.any() and not ed.series.all() and ed.small.any() and not ed.small.all()
    assert np.abs(ed.xi.astype(float) - info['xi']).max() <= 1e-10                          # (3.1 rad: 2^-53 / sin(3.1) and the cofactors)
    _, table = ld.retract(g, -ed.rt.astype(float))
    assert table['retract/exp/w_series'].any() and not table['retract/exp/w_series'].all()
    assert table['retract/exp/h12'].any() and table['retract/exp/closed/h12'].any()
    # noisy_loop: under the stopping rule the steps become non-decreasing, and what is restored is not the last iterate
    g, _ = rs.scene('noisy_loop')
    V, edges = as_objects(g)
    for nd, its in ((1, 3), (2, 4), (3, 5)):
        opt = Options()
        opt.allow_nondecreasing_steps, opt.max_nondecreasing_steps = True, nd
        Vs, hist, n = sg.solve(V, edges, g.held, None, opt)
        assert n == its and len(hist) == its + 1 and hist[-1] > 0.05 and hist[3] >= opt.min_cost_decrease * hist[2]
        last = V
        for _ in range(its):
            last = sg.iterate(last, edges, g.held)[0]
        same = all(np.array_equal(pg.pack13(a), pg.pack13(b)) for a, b in zip(Vs, last))
        assert same == (nd == 1), nd


def test_every_step_scene_is_definite():
    for name in rs.STEP_SCENES:
        assert rs.definite(name), name
        if name != 'hang257':
            assert rs.definite(name, 1e-3), name


# ---------------------------------------------------------------------------
# 4. the reference's own error
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', rs.ROW_SCENES)
def test_e64_by_scene(name):
    e = rs.e64(name)
    worst = {}
    for k, v in e.items():
        kk = k[0] if isinstance(k, tuple) else k
        worst[kk] = max(worst.get(kk, 0.), v)
    print('{:28s} e64: {}'.format(name, '  '.join('{} {:.1e}'.format(k, v) for k, v in worst.items())))
    for what in ('rt', 'J1', 'J2', 'H', 'g'):
        if what in OFF_FLOOR.get(name, ()):
            assert rs.TOL_ROW < rs.FACTOR * worst[what] <= 1e-10, (name, what, worst[what])      # (recorded: it is off the floor, and why)
        else:
            assert rs.FACTOR * worst[what] <= rs.TOL_ROW, (name, what, worst[what])
    if name != 'exact':
        assert rs.FACTOR * worst['cost'] <= rs.TOL_COST, (name, worst['cost'])


# ---------------------------------------------------------------------------
# 5. L1 at zero residuals
# ---------------------------------------------------------------------------
def test_l1_takes_its_first_step_from_zero_residuals():
    """loop_graph measures odometry from the estimates: under L1 every such component is zero, where L1Loss.weight is NaN.  The graph's
    rule 1 / max(|r_k|, 1e-8) keeps H finite and definite; the first step lowers the cost, and the restatement's whole solve ends
    nearer the truth than it started."""
    g, info = rs.scene('l1_zero')
    d = info['scene']
    graph = pg.loop_graph(d['poses_est'], [d['closure']], loss=losses.L1Loss())
    V, held = list(graph.vertices), np.array(graph.held)
    assert np.isnan(losses.L1Loss().weight(np.zeros(1))[0])                     # the loss itself is unchanged
    r = sg.residuals(V, graph.edges)
    assert np.abs(r[:11]).max() <= 2e-14
    H, gv, c0 = sg.linearise(V, graph.edges, held, graph.loss)
    assert np.all(np.isfinite(H)) and np.all(np.isfinite(gv)) and np.linalg.eigvalsh(H)[0] > 0.
    rho, w = sg._rho_weight(losses.L1Loss(), np.array([0., 1e-9, -2e-8, 0.5]))
    assert np.array_equal(w, [1e8, 1e8, 1. / 2e-8, 2.]) and np.array_equal(rho, [0., 1e-9, 2e-8, 0.5])
    new, dx, c1 = sg.iterate(V, graph.edges, held, graph.loss)
    assert np.linalg.norm(dx) > 0. and c1 < c0
    Vs, hist, its = sg.solve(V, graph.edges, held, graph.loss, Options())
    poses, _, _ = pg.apply_correction(V, Vs, d['poses_est'])
    before, after = gs.centre_rmse(d['poses_est'], d['poses_true']), gs.centre_rmse(poses, d['poses_true'])
    print('L1 loop correction by the restatement: {} iterations, cost {:.3e} -> {:.3e}, centre RMSE {:.4f} -> {:.4f}'.format(
        its, hist[0], hist[-1], before, after))
    assert its >= 1 and np.all(np.isfinite(hist)) and after < before
