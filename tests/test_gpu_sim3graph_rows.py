"""The Sim(3) pose-graph kernels on the device (csrc/ps_k_sim3pg.h, ps_host_sim3pg.h, ps_abi_sim3pg.h) per edge, per block and per
vertex against a long-double definition (tests/longdouble_sim3graph.py, written apart from the restatement and held against mpmath
by tests/test_sim3graph_rows_host.py), on scenes built from a wanted error transform (tests/sim3graph_row_scenes.py).  Kernels:
k_s3g_edges (with sim3_log, sim3_w_coef, sim3_adj and the losses), k_s3g_assemble, k_s3g_sum, k_s3g_retract (sim3_exp), and the keep /
restore exchange of ps_sim3pg_solve.  The older tests (tests/test_gpu_sim3graph.py) stay as they are.

Measure.  Per row of r~, J~_1, J~_2 (one row per edge), per 7 x 7 block of H, per 7-vector of g and per vertex: the largest absolute
difference from the long-double reference over max(the row's own largest reference entry, u).  u is the row's ROUNDING SCALE, the size
of the numbers whose rounded products the row was formed from (one rounding of the row is 2^-53 u): for an edge the infinity norm
of its stiffness times the largest magnitude among the summands that form the error transform's translation through S_j S_i^-1 S_ji^-1
-- |t_j|, (s_j / s_i) |t_i|, (s_j / (s_i s_ji)) |t_ji| -- floored at 1 (longdouble_sim3graph.edge_scale); for a block of H or a
vector of g the largest u_e max(|J~_e|, u_e) among the edges that touch it (system_floors); for a vertex 1.
tests/test_sim3graph_rows_host.py checks the definition on km, mm and map_scales by e64.

Bounds.  Rows, blocks, vectors and vertices: max(1e-12, 8 e64), e64 the fp64 twin's distance from the long-double pass on the same input
over the scene and its one-ulp copies, r~ / J~ per (loss, branch) class.  Cost: 1e-10.  The whole step: max(1e-8, 8 e_ref) against
longdouble_sim3graph.accurate_solve of the long-double system, e_ref a dense fp64 solve of the twin's system against the same.  No
bound comes from the device's output.  `exact` is held absolutely as well: 32 x 2^-53 of the rounding scale.  Exact statements
beside the bounds: absent rows and rows under a zero Tukey weight are 0, blocks no edge touches are 0, H is symmetric to the bit,
eval_cost is the linearisation's cost to the bit, held vertices keep their bits, two handles on the same tables give the same bits.

The logarithm's branch.  Under L2 and the identity stiffness r~ is xi; where the two branches of sim3_log's `sn <= 1e-8` differ by more
than 64 x 2^-53 in an edge's rotation part, the device must lie nearer the fp64 twin forced into the branch the predicate takes than
the twin forced into the other.  Beside rotation entries of size 1 the branches lie that far apart only from 3.5e-5 rad on (they
differ by theta^3 / 6); the scene `bare` (vertex 0 and every measurement the identity: the error transform is S_v to the bit, no product
is rounded) is judged relative to |phi| instead, from 2e-7 rad on -- the edges at 3e-7 and 9e-7 rad are what sees a small branch taken
up to 1e-6.

The step.  The device does not return dx; it is read back as log(S_new S_old^-1) in long double from the vertices before and after
(exact inputs).  On hang257 H = I and dx = g to the bit (the factor of I is I, the refinement adds zero), so there the retraction
is held per vertex against the long-double exp(g) S: two workgroups of k_s3g_retract, both branches of sim3_w_coef and of
s3g_h12, steps of 3.1 rad and of 1e-9.

By the reference alone every scene sits on the 1e-12 floor except angles (the edge at 3.1415 rad) and l1_zero (the capped rows):
tests/test_sim3graph_rows_host.py has the figures and the reasons.

Observed on an MI355X, one run, "device / e64" (the bound is max(1e-12, 8 e64)); per scene the entry with the least margin over its
classes and both dampings; dx: device / e_ref; cost: relative; rows = the 22 variants of the `rows` graph (six losses x identity, four
losses x four stiffness kinds), L1 apart.  tests/parity_margins.py prints every scene on its own:

  scene                                 r~                J~                 H                 g                dx          vertices      cost
  angles                   5.3e-13/1.1e-12   2.3e-16/2.9e-16   3.7e-16/6.8e-16   2.1e-13/4.2e-13   5.9e-13/2.1e-13                 -   8.2e-15
  bare                     2.7e-16/2.6e-16   9.3e-17/1.9e-16   1.1e-16/1.1e-16   2.7e-16/4.4e-16   5.4e-16/3.7e-16                 -         0
  scales                   4.0e-16/5.6e-16   3.0e-16/4.6e-16   5.1e-16/5.4e-16   2.6e-16/5.9e-16   2.9e-12/2.2e-12                 -         0
  km                       2.1e-16/4.6e-16   1.9e-16/3.7e-16   5.1e-16/6.3e-16   2.3e-16/6.4e-16   2.0e-09/2.4e-09                 -   3.5e-16
  mm                       2.0e-16/2.5e-16   2.0e-16/3.1e-16   3.8e-16/5.1e-16   2.9e-16/3.9e-16   3.9e-16/3.2e-16                 -   5.5e-16
  map_scales               2.7e-16/3.4e-16   2.3e-16/3.5e-16   3.4e-16/7.0e-16   1.6e-16/4.9e-16   1.3e-04/2.1e-04                 -   1.6e-14
  exact                    2.8e-16/4.1e-16   1.7e-16/4.1e-16   4.2e-16/5.2e-16   2.5e-16/4.4e-16                 -                 -         -
  wg64                     3.0e-16/3.9e-16   1.6e-15/1.5e-15   6.5e-16/1.2e-15   1.3e-16/4.2e-16   4.3e-15/7.4e-15                 -   2.2e-16
  E65                      2.3e-16/5.5e-16   1.8e-15/2.5e-15   7.7e-16/1.9e-15   7.6e-17/2.2e-16   2.3e-15/2.8e-15                 -         0
  many_edges               6.0e-16/7.3e-16   1.1e-14/1.9e-14   7.2e-15/1.0e-14   6.2e-14/9.2e-14   2.3e-13/6.2e-14                 -   1.2e-16
  hang257                  2.2e-15/2.9e-15   2.6e-16/3.9e-16   1.1e-16/1.1e-16   7.3e-16/1.2e-15   2.9e-15/2.2e-15   7.7e-16/6.8e-16         0
  noisy_loop               3.0e-16/3.9e-16   2.5e-16/3.7e-16   4.6e-16/5.5e-16   3.6e-16/4.8e-16   1.4e-14/1.6e-13                 -   7.6e-16
  rows (identity)          6.6e-16/8.6e-16   2.1e-15/4.7e-15   2.2e-15/4.8e-15   4.3e-16/9.4e-16   7.3e-15/7.3e-15                 -   3.7e-16
  rows (identity, L1)      5.7e-16/9.0e-16   9.4e-15/2.1e-14   1.5e-14/4.1e-14   4.1e-17/4.1e-17   4.6e-15/2.0e-15                 -   1.1e-16
  rows (stiffness)         3.3e-16/4.2e-16   2.1e-15/4.7e-15   2.4e-15/4.9e-15   2.9e-16/4.9e-16   7.1e-13/6.8e-12                 -   6.5e-16
  rows (stiffness, L1)     5.7e-16/9.0e-16   9.4e-15/2.1e-14   1.5e-14/4.1e-14   3.6e-17/4.1e-17   4.7e-15/4.7e-12                 -   5.4e-16
  l1_zero                  1.7e-12/4.2e-12   2.5e-14/2.8e-14   5.3e-16/1.0e-15   1.7e-12/4.1e-12   3.2e-10/1.3e-10                 -   2.7e-15

exact: |r~| 3.4e-16 of u, |g| 9.5e-17 of its scale (bound 3.6e-15), |dx| 1.3e-15 absolutely (bound 2.5e-11 behind H^-1); the costs after
the step of exact, bare and hang257 are rounding noise and are held absolutely.  map_scales' step: cond(H) = 2e12.  The branch of
sim3_log was judged on 18 of 24 (angles), 5 of 8 (bare: 3e-7, 9e-7, 1e-5, 1e-3, 0.3), 90 of 120 (scales), 155 of 257 (hang257) edges.
noisy_loop: 3, 4, 5 iterations for max_nondecreasing_steps 1, 2, 3, the table kept after iteration 3 restored each time, the
restatement's vertices to 1.3e-15.  correct_loop under L1 on the 12-keyframe drift scene: 1 iteration as the restatement (the default
rule stops a step that lowers the cost by less than 10 %), cost 1.700963 -> 1.700877, centre RMSE lower in its fifth digit.  No defect
beyond L1's weight at zero was found.

That the checks can fail (each change made in a scratch copy of the kernels, built apart, one run, not kept; "old" = the 24 tests of
tests/test_gpu_sim3graph.py): (a) sim3_log's small branch up to 1e-6 fails test_edge_rows[bare] in the branch check alone (edge at 3e-7:
4e-21 from the other branch's twin, 0 from its own) -- old pass; (b) k_s3g_sum over its first 256 partials fails
test_normal_equations_and_cost[many_edges] (cost off by 3.7e-3) and test_step[many_edges] -- old pass; (c) k_s3g_retract ignoring its
second workgroup fails test_hang257_retraction_per_vertex (dx off by 0.64) -- old pass; (d) ps_sim3pg_solve without the exchange fails
test_solve_keeps_and_restores_what_the_rule_says[2] and [3] -- old pass; (e) ps_loss_weight's NaN for L1 fails test_edge_rows[l1_zero],
test_normal_equations_and_cost[l1_zero], test_l1_takes_its_first_step_from_zero_residuals and
test_correct_loop_under_l1_ends_nearer_the_truth -- old pass; (f) `present` ignored under a non-L2 loss changes NO output now (the row of
the stiffness is zero, so r_k = 0 and s_k times a zero row is zero under every loss, L1's weight at zero being finite): all 99 and the
old pass -- an equivalent mutant, named here so that nobody counts on a test for it; (g) phase 2 reading its wave's first scale fails 54
of the 99 (every scene with a robust loss) and old [huber], [cauchy]."""
import numpy as np
import pytest

import longdouble_sim3graph as ld
import sim3graph_row_scenes as rs
from pyslam_amd import _native as nat
from pyslam_amd.pipelines import posegraph as pg
from pyslam_amd.problem import Options, StopRule

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ld.LONGDOUBLE_OK, reason=ld.LONGDOUBLE_SKIP)]

LD = ld.LD
EPS = ld.EPS


def loss_object(g):
    from pyslam_amd import losses
    if g.loss_id == ld.L2:
        return None
    cls = (None, losses.L1Loss, losses.CauchyLoss, losses.HuberLoss, losses.TukeyLoss, losses.TDistributionLoss)[g.loss_id]
    return cls() if g.loss_id == ld.L1 else cls(g.loss_k)


def device(g):
    return pg.DeviceSim3Graph(*g.device_args(), loss=loss_object(g))


def report(name, what, err, e64, limit):
    print('{:28s} {:30s} device {:.2e}   e64 {:.2e}   bound {:.2e}'.format(name, what, err, e64, limit))


def check(name, what, err, e64, floor=rs.TOL_ROW):
    limit = rs.bound(e64, floor)
    report(name, what, err, e64, limit)
    assert err <= limit, (name, what, err, e64, limit)


def plain(g):
    return g.loss_id == ld.L2 and g.stiffness is None


# ---------------------------------------------------------------------------
# 1. the tap: r~, J~_1, J~_2 per edge
# ---------------------------------------------------------------------------
def rows(name):
    g, info = rs.scene(name)
    ref = rs.edge_pairs(name)[0][0]
    e64 = rs.e64(name)
    u = ld.edge_scale(g)
    dev = device(g)
    try:
        got = dict(zip(('rt', 'J1', 'J2'), dev.debug_edges()))
    finally:
        dev.close()
    assert all(np.all(np.isfinite(a)) for a in got.values())
    zero = ~ref.present | (ref.s == 0)                                   # absent rows, and rows under a zero Tukey weight
    assert np.all(got['rt'][zero] == 0.) and np.all(got['J1'][zero] == 0.) and np.all(got['J2'][zero] == 0.)
    if name.startswith('rows-Tukey') or name == 'wg64':
        assert zero.any()
    if name == 'exact':
        worst = float((np.abs(got['rt']).max(axis=1) / u).max())
        print('{:28s} {:30s} device {:.2e}   bound {:.2e} (absolute, over u)'.format(name, '|r~|', worst, 32 * EPS))
        assert worst <= 32 * EPS, worst
    for key, edges in sorted(rs.classes(ref).items()):
        for what in ('rt', 'J1', 'J2'):
            check(name, '{} {} {}'.format(what, *key), ld.row_err(got[what][edges], getattr(ref, what)[edges], u[edges]), e64[what, key])
    if plain(g):
        forced = {b: ld.Edges(g, np.float64, force={'log_small': b}).rt[:, 3:6] for b in (True, False)}
        # (an edge of exact products -- the scene `bare` -- carries no rounding of a rotation entry: there the two branches are told apart
        #  relative to |phi|; elsewhere absolutely, beside rotation entries of size 1)
        size = np.where(info.get('bare', np.zeros(g.E, dtype=bool)), np.abs(ref.xi[:, 3:6].astype(float)).max(axis=1), 1.)
        with np.errstate(invalid='ignore'):
            apart = np.abs(forced[True] - forced[False]).max(axis=1)
            judged = np.flatnonzero(np.isfinite(apart) & (apart > 64 * EPS * size))
        for e in judged:
            mine, other = forced[bool(ref.small[e])][e], forced[not ref.small[e]][e]
            d_mine, d_other = np.abs(got['rt'][e, 3:6] - mine).max(), np.abs(got['rt'][e, 3:6] - other).max()
            assert d_mine < d_other, (name, 'edge {} took the other branch of sim3_log'.format(e), d_mine, d_other)
        print('{:28s} branch of sim3_log judged on {} of {} edges'.format(name, len(judged), g.E))
        if name == 'bare':                      # ... among them edges between 1e-7 and 1e-6 that belong to the logarithm
            assert np.sum((info['angle'][judged] > 1e-7) & (info['angle'][judged] < 1e-6)) == 2, info['angle'][judged]


@pytest.mark.parametrize('name', rs.ROW_SCENES)
def test_edge_rows(name):
    rows(name)


# ---------------------------------------------------------------------------
# 2. H, g and the cost
# ---------------------------------------------------------------------------
def system(name):
    g, _ = rs.scene(name)
    ref = rs.edge_pairs(name)[0][0]
    e64 = rs.e64(name)
    dev, twin_dev = device(g), device(g)
    try:
        cost = None
        for lam in rs.LAMBDAS:
            Hr, gr, touched = rs.system_pairs(name, lam)[0][0]
            H, gv, c = dev.linearize(lam)
            assert np.all(np.isfinite(H)) and np.all(np.isfinite(gv)) and np.isfinite(c)
            eH, eg = ld.err_system((H, gv), (Hr, gr), ref)
            check(name, 'H lambda={}'.format(lam), eH, e64['H', lam])
            check(name, 'g lambda={}'.format(lam), eg, e64['g', lam])
            quiet = ~np.repeat(np.repeat(touched, 7, axis=0), 7, axis=1)
            assert np.all(H[quiet] == 0.) and np.array_equal(H, H.T)
            assert cost is None or c == cost
            cost = c
            H2, g2, c2 = twin_dev.linearize(lam)
            assert np.array_equal(H2, H) and np.array_equal(g2, gv) and c2 == c
        assert dev.eval_cost() == cost and twin_dev.eval_cost() == cost
        if name == 'exact':
            fg = ld.system_floors(ref)[1]
            count = np.bincount(np.concatenate([g.rid[g.ei], g.rid[g.ej]]) + 1, minlength=g.nfree + 1)[1:]
            worst = float((np.abs(gv).reshape(-1, 7).max(axis=1) / (fg * count)).max())
            print('{:28s} {:30s} device {:.2e}   bound {:.2e} (absolute, over the scale)'.format(name, '|g|', worst, 32 * EPS))
            assert worst <= 32 * EPS
            # cost: 7 E components of at most 32 x 2^-53 u each
            assert cost <= 0.5 * 7 * g.E * (32 * EPS * ld.edge_scale(g).max()) ** 2
        else:
            err = rs.cost_err(cost, ref.cost())
            report(name, 'cost', err, e64['cost'], rs.TOL_COST)
            assert err <= rs.TOL_COST, (name, err)
    finally:
        dev.close()
        twin_dev.close()


@pytest.mark.parametrize('name', rs.ROW_SCENES)
def test_normal_equations_and_cost(name):
    system(name)


# ---------------------------------------------------------------------------
# 3. one iteration: the step, the retraction, the cost after it
# ---------------------------------------------------------------------------
def read_step(g, before, after):
    """dx (nf, 7) in long double: log(S_new S_old^-1) of the free vertices, from the two vertex tables."""
    free = np.flatnonzero(~g.held)
    return ld.two_pass(lambda dt, p: ld.log(ld.mul(ld.unpack(after[free], dt), ld.inv(ld.unpack(before[free], dt))), p, 'step'), LD)[0]


def step(name, lam=0.):
    g, _ = rs.scene(name)
    dev = device(g)
    try:
        H, gv, c0 = dev.linearize(lam)
        cost_after, dxn, relres = dev.iteration(lam)
        V = dev.get_vertices()
        assert np.array_equal(V[g.held], g.V13[g.held])                           # held vertices keep their bits
        assert np.all(np.isfinite(V)) and np.isfinite(cost_after) and np.isfinite(relres)
        dx = read_step(g, g.V13, V)
        ref, e_ref = rs.step_reference(name, lam)
        if name == 'exact':
            # the step is rounding noise: |g| <= 32 x 2^-53 of its scale per edge that touches the vertex, behind the reference's H^-1
            fg = ld.system_floors(rs.edge_pairs(name)[0][0])[1]
            count = np.bincount(np.concatenate([g.rid[g.ei], g.rid[g.ej]]) + 1, minlength=g.nfree + 1)[1:]
            Hinv = np.linalg.inv(rs.system_pairs(name, lam)[0][0][0].astype(float))
            limit = float(np.abs(Hinv).sum(axis=1).max() * (32 * EPS * fg * count).max())
            worst = float(np.abs(dx).max())
            print('{:28s} {:30s} device {:.2e}   bound {:.2e} (absolute)'.format(name, '|dx| lambda={}'.format(lam), worst, limit))
            assert worst <= limit
        else:
            err = float(np.abs(dx.reshape(-1) - ref).max() / np.abs(ref).max())
            check(name, 'dx lambda={}'.format(lam), err, e_ref, rs.TOL_DX)
            norm = float(np.sqrt((ref * ref).sum()))
            assert abs(dxn - norm) <= rs.bound(e_ref, rs.TOL_DX) * norm
        # the cost after the step is the cost AT the device's new vertices (exact inputs again); where the step removes the whole
        # residual (exact, bare, hang257) that cost is rounding noise: 7 E components of at most 64 x 2^-53 u each
        want = ld.Edges(g.with_vertices(V), LD).cost()
        noise = 0.5 * 7 * g.E * (64 * EPS * ld.edge_scale(g).max()) ** 2
        report(name, 'cost after the step', abs(cost_after - want) / max(want, noise), 0., rs.TOL_COST)
        assert abs(cost_after - want) <= rs.TOL_COST * want + noise, (name, cost_after, want)
        assert dev.eval_cost() == cost_after
        return V, gv
    finally:
        dev.close()


@pytest.mark.parametrize('name', [n for n in rs.STEP_SCENES if n not in ('hang257', 'l1_zero')])
def test_step(name):
    step(name, 0.)
    if name in ('angles', 'wg64', 'rows-Huber-identity'):
        step(name, 1e-3)


def test_hang257_retraction_per_vertex():
    """H = I, so dx is g (the factor of I is I, the refinement adds zero), and every vertex is exp(g_v) S_v."""
    name = 'hang257'
    g, info = rs.scene(name)
    V, gv = step(name, 0.)
    dx = gv.reshape(-1, 7)
    want, table = ld.retract(g, dx, LD)
    assert table['retract/exp/w_series'].any() and not table['retract/exp/w_series'].all() and table['retract/exp/h12'].any()
    angle = np.sqrt((dx[:, 3:6] ** 2).sum(axis=1))
    assert angle.max() > 3.09 and 0 < angle[angle > 0].min() < 2e-9
    errs = ld.row_errs(V, want, ld.vertex_floor(want))
    e64 = rs.e64_retract(name, dx)
    check(name, 'vertices after exp(dx) S', float(errs.max()), e64)
    check(name, '... of the second workgroup', float(errs[257:].max()), e64)          # vertex 257 = free vertex 256
    assert np.array_equal(V[0], g.V13[0])


# ---------------------------------------------------------------------------
# 4. the solve loop's kept and restored vertices
# ---------------------------------------------------------------------------
def history_close(hist, ref):
    """tests/test_gpu_sim3graph.py's rule for a cost history."""
    hist, ref = np.asarray(hist), np.asarray(ref)
    big = ref > 1e-9 * ref[0]
    prev = np.concatenate([[ref[0]], ref[:-1]])
    gap = np.abs(hist - ref)
    assert np.all(gap[big] <= rs.TOL_COST * np.abs(ref[big]) + 1e-15 * prev[big]), gap / np.abs(ref)
    assert np.all(hist[~big] <= 1e-9 * ref[0])


@pytest.mark.parametrize('max_nd', (1, 2, 3))
def test_solve_keeps_and_restores_what_the_rule_says(max_nd):
    from pyslam_amd.pipelines import simgraph as sg
    g, _ = rs.scene('noisy_loop')
    opt = Options()
    opt.allow_nondecreasing_steps, opt.max_nondecreasing_steps = True, max_nd
    dev = device(g)
    try:
        # the replay: single iterations, the Python rule on their costs and step norms
        hist = [dev.eval_cost()]
        rule = StopRule(opt, hist[0])
        best, kept_at, restored = None, None, False
        while True:
            c, dxn, _ = dev.iteration(opt.lm_lambda)
            hist.append(c)
            f = rule.step(c, dxn)
            if f & StopRule.KEEP_BEST:
                best, kept_at = dev.get_vertices(), rule.iters
            if f & StopRule.RESTORE_BEST:
                restored = True
            if f & StopRule.DONE:
                break
        last = dev.get_vertices()
        want = best if restored else last
        assert restored and kept_at is not None and (kept_at < rule.iters) == (max_nd > 1)
        assert np.array_equal(want, last) == (max_nd == 1)                         # beyond 1 the restored table is not the last iterate
        # the loop in the core, from the same start
        dev.set_vertices(g.V13)
        h1, its1, dxn1 = dev.solve(opt)
        V1 = dev.get_vertices()
        assert its1 == rule.iters and np.array_equal(h1, hist) and np.array_equal(V1, want)
        # again on the same handle, after the two tables were exchanged
        dev.set_vertices(g.V13)
        h2, its2, dxn2 = dev.solve(opt)
        assert its2 == its1 and dxn2 == dxn1 and np.array_equal(h2, h1) and np.array_equal(dev.get_vertices(), V1)
        assert dev.eval_cost() == hist[kept_at]                                    # the cost of what was restored
        # the restatement, by the existing history rule
        V, edges = [pg.unpack13(r) for r in g.V13], [(int(i), int(j), pg.unpack13(o), None) for i, j, o in zip(g.ei, g.ej, g.obs13)]
        Vs, hist_ref, its_ref = sg.solve(V, edges, g.held, None, opt)
        assert its_ref == its1 and len(hist_ref) == len(h1)
        history_close(h1, hist_ref)
        gap = max(np.abs(pg.pack13(a) - b).max() for a, b in zip(Vs, V1))
        print('noisy_loop, max_nondecreasing_steps {}: {} iterations, kept after {}, restatement to {:.2e}'.format(max_nd, its1, kept_at, gap))
        assert gap <= 1e-9
    finally:
        dev.close()


# ---------------------------------------------------------------------------
# 5. L1 from zero residuals
# ---------------------------------------------------------------------------
def test_l1_takes_its_first_step_from_zero_residuals():
    """The loop graph under L1: every odometry component starts at zero.  With ps_loss_weight's NaN there H was NaN and the
    factorisation reported "not positive definite"; with the graph's rule 1 / max(|r_k|, 1e-8) H is finite, a step is taken and the cost
    falls."""
    name = 'l1_zero'
    g, info = rs.scene(name)
    dev = device(g)
    try:
        H, gv, c0 = dev.linearize(0.)
        assert np.all(np.isfinite(H)) and np.all(np.isfinite(gv))
    finally:
        dev.close()
    V, _ = step(name, 0.)
    assert not np.array_equal(V, g.V13)
    dev = device(g)
    try:
        c1, dxn, _ = dev.iteration(0.)
        assert dxn > 0. and c1 < c0
    finally:
        dev.close()


def test_correct_loop_under_l1_ends_nearer_the_truth():
    import sim3graph_scenes as gs
    from pyslam_amd import losses
    from pyslam_amd.pipelines import simgraph as sg
    d = rs.scene('l1_zero')[1]['scene']
    poses, scales, _ = pg.correct_loop(d['poses_est'], [d['closure']], loss=losses.L1Loss())
    run = pg.correct_loop.last_graph
    before, after = gs.centre_rmse(d['poses_est'], d['poses_true']), gs.centre_rmse(poses, d['poses_true'])
    graph = pg.loop_graph(d['poses_est'], [d['closure']], loss=losses.L1Loss())
    Vs, hist_ref, its_ref = sg.solve(list(graph.vertices), graph.edges, np.array(graph.held), graph.loss, Options())
    poses_ref, _, _ = pg.apply_correction(list(graph.vertices), Vs, d['poses_est'])
    after_ref = gs.centre_rmse(poses_ref, d['poses_true'])
    print('L1 loop correction: {} iterations (restatement {}), cost {:.6e} -> {:.6e} (restatement {:.6e}), centre RMSE {:.4f} -> {:.4f} '
          '(restatement {:.4f})'.format(run.iterations, its_ref, run.cost_history[0], run.cost_history[-1], hist_ref[-1], before, after, after_ref))
    assert run.iterations >= 1 and np.all(np.isfinite(run.cost_history)) and np.all(np.isfinite(poses))
    assert after < before and after_ref < before


# ---------------------------------------------------------------------------
# 6. a handle with no edges
# ---------------------------------------------------------------------------
def test_a_graph_without_edges():
    g, _ = rs.scene('exact')
    none = np.zeros(0, dtype=np.int32)
    dev = pg.DeviceSim3Graph(g.V13, g.held, none, none, np.zeros((0, 13)))
    try:
        assert dev.eval_cost() == 0.
        H, gv, c = dev.linearize(0.)
        assert not H.any() and not gv.any() and c == 0.                            # the system it reports: all zero, indefinite
        for call in (lambda: dev.iteration(0.), lambda: dev.solve()):
            with pytest.raises(nat.NativeError, match='not positive definite to rounding'):
                call()
            assert np.array_equal(dev.get_vertices(), g.V13)                       # nothing moved
        assert dev.eval_cost() == 0.
        r, J1, J2 = dev.debug_edges()
        assert r.shape == (0, 7)
    finally:
        dev.close()


def margins(name):
    """What tests/parity_margins.py prints for a scene: every figure of rows / system / step with its e64 and bound."""
    rows(name)
    system(name)
    if name in rs.STEP_SCENES:
        step(name, 0.)
