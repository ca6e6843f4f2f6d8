"""The bundle-adjustment linearisation on the device outside the box synthetic.stereo_ba draws from, against a long-double reference
(tests/longdouble_schur.py) and the oracle -- never against another device variant; the bit-for-bit claims between variants are
asserted beside that, separately.  Scenes: tests/offbox_scenes.py (landmarks at 0.5-2.4 m, 6-30 m, 60-300 m, 600-3000 m, all of these
in one wave, millimetres, three camera types under four losses in every wave, group ids up to 254, one stiffness per observation).
Kernels: k_landmark_pass_packed / k_landmark_pass, k_pose_pass / k_pose_pass_pf, k_schur_pairs_db (tiled and untiled pair list),
k_backsub_packed, the cost kernels (csrc/ps_k_packed.h, ps_k_linearize.h, ps_k_schur2.h, ps_k_tail.h).  Counterpart of reference
pyslam/problem.py:338-360 (J~, r~ per block), :332-333 (J~^T J~) and :186 (the solve).

Measure: per row of a table (per observation's block, per landmark's factor, per 6 x 6 block of S, per 6-vector of g or of the step)
the largest absolute difference over that row's own largest reference entry; the maximum over rows (longdouble_schur.row_err).
conftest.rel_err divides by the norm of the whole table and hides a wrong far row behind a near one.

Bounds.  e64 is the distance of an fp64 evaluation from the long-double evaluation OF THE SAME INPUT, in the same measure: orc.eval_reproj
in fp64 + the fp64 twin of the elimination against the same code in long double.  It is sampled on the scene's tables and on DRAWS = 8
copies of them with every pose entry, coordinate and observation one ulp away (longdouble_schur.one_ulp_away) -- each copy's fp64 result
against THAT copy's long-double result, so the sample holds fp64 evaluation error only, never the scene's sensitivity to its input --
and e64 is the largest of the nine.  (The issue's e64 is the first of the nine alone.  Under L1's weight 1 / |r| the evaluation error is
heavy-tailed: on S of mixed_wave at lambda = 1e-3 the nine range from 6.4e-13 to 5.9e-12, the scene's own draw being 6.6e-13; one
draw is no bound for another's.  The 512-row case keeps the single twin.)  No bound comes from the device's output.
  r~, J~p, J~l    max(TOL_BLOCK, 8 e64), the rows of each loss apart.  TOL_BLOCK (1e-12) alone holds for J~ under L2 everywhere; it fails
                  ON THE REFERENCE for r~ and under the robust losses: r cancels pixel coordinates of ~1e3 down to a residual that is all
                  noise in these scenes, so fp64 leaves ~3e-13 px -- 2e-12 .. 4e-12 of the row whose largest component is 0.01 .. 0.03
                  px -- and L1's weight 1 / |r| (Huber's tail, Cauchy) passes the relative error of r on to J~.  For the same reason the
                  reference blocks are the oracle's evaluated in long double, not its fp64 blocks cast.
  cost            TOL_COST (1e-10)
  C^-1, c, S, g, the landmark part of the step given the device's pose part
                  max(TOL_BLOCK, 8 e64) per scene, quantity and damping (the factor 8: tests/test_gpu_bchol_kernels.py,
                  sim3graph_scenes.EXPLOG_FACTOR).  "C^-1" is the inverse Cholesky factor the handle keeps (ps_get_landmark_factors).
  whole dx        max(TOL_DX, 8 e_ref), e_ref the distance of the oracle's spsolve step from test_gpu_parity.accurate_solve

Observed on an MI355X, "device / e64" (the bound is max(1e-12, 8 e64); the worst variant of each quantity; the whole dx against its
arbiter: device / e_ref; cost: the worst of eval_cost(True), eval_cost(False) and the cost after a whole iteration).  lambda = 0:

  scene                         r~               J~             C^-1                c                S                g             dx_l               dx             cost
  near             1.7e-12/4.6e-12  5.4e-16/8.7e-16  7.4e-15/6.4e-15  9.0e-13/2.6e-12  1.3e-15/2.5e-15  8.5e-13/2.2e-12  1.5e-12/5.6e-12  9.3e-14/1.8e-14          5.0e-15
  base             2.1e-12/3.1e-12  4.6e-16/6.8e-16  5.9e-13/7.2e-13  1.0e-12/2.8e-12  3.0e-14/1.0e-13  3.2e-13/2.6e-12  2.1e-11/2.7e-11  3.8e-13/8.6e-13          2.2e-15
  far10            2.7e-12/3.9e-12  4.8e-16/8.0e-16  5.0e-11/6.2e-11  4.2e-11/6.3e-11  2.4e-12/1.4e-11  1.5e-11/4.3e-11  1.0e-10/1.7e-10  3.1e-11/1.0e-10          1.7e-15
  far100           1.4e-12/3.8e-12  4.4e-16/6.8e-16  5.3e-09/5.7e-09  5.3e-09/5.7e-09  1.9e-10/8.4e-10  1.8e-09/4.1e-09  1.1e-08/1.0e-08  3.7e-09/1.0e-08          5.2e-15
  mm               1.3e-13/3.8e-13  4.2e-16/6.3e-16  5.3e-13/5.4e-13  2.8e-13/2.6e-13  2.5e-14/1.1e-13  2.6e-15/2.6e-14  1.8e-12/7.8e-12  2.9e-13/1.0e-12          1.4e-15
  mixed_depth      2.7e-12/3.8e-12  5.0e-16/6.8e-16  4.4e-09/5.5e-09  4.4e-09/4.7e-09  1.3e-10/2.9e-10  7.3e-10/1.3e-09  8.4e-09/1.0e-08  4.2e-09/6.5e-09          3.3e-15
  mixed_wave       1.1e-12/1.6e-12  1.5e-13/3.9e-13  3.8e-12/5.3e-12  2.5e-12/7.0e-12  6.0e-12/6.5e-12  7.0e-13/3.0e-12  7.6e-12/1.2e-11  1.4e-12/1.5e-11          2.5e-15
  high_group_ids   1.1e-12/1.6e-12  1.5e-13/3.9e-13  3.8e-12/5.3e-12  2.5e-12/7.0e-12  6.0e-12/6.5e-12  7.0e-13/3.0e-12  7.6e-12/1.2e-11  1.4e-12/1.5e-11          2.5e-15
  wide_mixed       1.1e-12/1.6e-12  1.4e-13/3.9e-13  3.9e-12/1.1e-11  3.4e-12/1.2e-11  6.6e-12/6.3e-12  5.5e-13/3.8e-12  1.2e-11/2.9e-11  1.4e-12/4.0e-11          5.6e-15

  lambda = 1e-3               C^-1                c                S                g
  near             7.1e-15/8.9e-15  9.1e-13/2.6e-12  8.0e-16/3.1e-15  8.5e-13/2.3e-12
  base             1.8e-13/2.1e-13  1.0e-12/3.1e-12  2.0e-14/3.8e-14  2.9e-13/2.7e-12
  far10            2.7e-13/2.6e-13  4.8e-12/5.7e-12  1.8e-15/2.6e-14  4.8e-13/1.8e-12
  far100           3.2e-13/2.5e-13  4.6e-12/7.5e-12  3.0e-16/3.0e-14  5.3e-13/2.3e-12
  mm               1.3e-13/1.7e-13  7.9e-14/1.1e-13  1.9e-14/4.8e-14  2.3e-15/1.2e-14
  mixed_depth      2.2e-13/2.6e-13  1.8e-12/7.5e-12  5.4e-15/2.7e-14  1.0e-12/8.6e-13
  mixed_wave       2.9e-12/5.4e-12  2.3e-12/7.0e-12  5.9e-12/5.9e-12  4.5e-13/2.3e-12
  high_group_ids   2.9e-12/5.4e-12  2.3e-12/7.0e-12  5.9e-12/5.9e-12  4.5e-13/2.3e-12
  wide_mixed       3.0e-12/6.4e-12  3.2e-12/6.3e-12  6.6e-12/6.6e-12  6.5e-13/1.5e-12

  512-row items (case 6), diagonal blocks of S / g, both dampings: big_mixed_groups 2.5e-15 / 2.9e-15 (e64 1.8e-14 / 1.7e-14),
  big_wide 4.4e-15 / 7.2e-15 (e64 2.2e-14 / 1.5e-14): bound 1e-12.
The reduced systems here have 48 unknowns and are solved directly (0 PCG iterations): the PCG is not reached by these scenes.
tests/parity_margins.py prints these figures; DESIGN.md section 4 has the table too."""
import functools

import numpy as np
import pytest

import longdouble_schur as ld
import offbox_scenes as sc
from conftest import rel_err
from oracle import gn_oracle as orc
from test_gpu_parity import TOL_BLOCK, TOL_COST, TOL_DX, accurate_solve

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ld.LONGDOUBLE_OK, reason=ld.LONGDOUBLE_SKIP)]

FACTOR = 8
LAMBDAS = (0., 1e-3)
PCG_MAX_ITERS = 2000
PCG_TOL = 1e-12                    # what the default (tolerance 0) resolves to on a bundle adjustment (include/pyslam_hip.h)


def bound(e64, floor=TOL_BLOCK):
    return max(floor, FACTOR * e64)


def device(lp):
    from pyslam_amd.device import DeviceProblem
    return DeviceProblem(lp)


# ---------------------------------------------------------------------------
# references: once per scene, shared, never written to
# ---------------------------------------------------------------------------
LOSS_NAMES = ('L2', 'L1', 'Cauchy', 'Huber', 'Tukey', 'TDist')


DRAWS = 8           # copies of a scene one ulp away (longdouble_schur.one_ulp_away) on which the fp64 error is sampled as well


@functools.lru_cache(maxsize=None)
def problems(name):
    """The scene and DRAWS copies of it with every input one ulp away."""
    lp, _ = sc.scene(name)
    return [lp] + [ld.one_ulp_away(lp, k) for k in range(DRAWS)]


@functools.lru_cache(maxsize=None)
def block_pairs(name):
    """Per problem of problems(name): (its blocks in long double, its blocks in fp64) -- like for like, the same input on both sides."""
    return [(ld.scaled_blocks(q, np.longdouble), ld.scaled_blocks(q, np.float64)) for q in problems(name)]


def block_reference(name):
    """(the scene's long-double blocks, the loss id of every row)."""
    lp = problems(name)[0]
    return block_pairs(name)[0][0], lp.obs_groups[lp.obs_grp, 2].astype(int)


def sampled(err_of_pair, pairs):
    """e64: the largest distance of an fp64 evaluation from the long-double evaluation OF THE SAME INPUT over the sample."""
    return max(err_of_pair(r, t) for r, t in pairs)


@functools.lru_cache(maxsize=None)
def elimination(name, lam):
    """(the scene's long-double elimination, [(long-double, fp64 twin) per problem of problems(name)], e64 per quantity)."""
    pairs = [(ld.Elimination(q, lam, np.longdouble, bl), ld.Elimination(q, lam, np.float64, b64))
             for q, (bl, b64) in zip(problems(name), block_pairs(name))]
    e64 = dict(Cinv=sampled(lambda r, t: ld.row_err(t.device_factors()[0], r.device_factors()[0]), pairs),
               c=sampled(lambda r, t: ld.row_err(t.device_factors()[1], r.device_factors()[1]), pairs),
               S=sampled(lambda r, t: ld.block_err(t.S, r.S), pairs), g=sampled(lambda r, t: ld.vec_err(t.g, r.g), pairs))
    return pairs[0][0], pairs, e64


def report(name, what, err, e64, limit):
    print('{:15s} {:28s} device {:.2e}   e64 {:.2e}   bound {:.2e}'.format(name, what, err, e64, limit))


def check(name, what, got, ref, e64, measure=ld.row_err, floor=TOL_BLOCK, fixed=False):
    err = measure(got, ref)
    limit = floor if fixed else bound(e64, floor)
    report(name, what, err, e64, limit)
    assert err <= limit, (name, what, err, e64, limit)
    return err


def check_factors(name, lam, dev, tag=''):
    ref, _, e64 = elimination(name, lam)
    cinv, c = dev.landmark_factors()
    Mr, cr = ref.device_factors()
    check(name, 'C^-1 lambda={} {}'.format(lam, tag), cinv, Mr, e64['Cinv'])
    check(name, 'c lambda={} {}'.format(lam, tag), c, cr, e64['c'])
    return cinv, c


def check_reduced(name, lam, dev, tag=''):
    ref, _, e64 = elimination(name, lam)
    S, g = dev.reduced_dense()
    check(name, 'S lambda={} {}'.format(lam, tag), S, ref.S, e64['S'], ld.block_err)
    check(name, 'g lambda={} {}'.format(lam, tag), g, ref.g, e64['g'], ld.vec_err)
    assert np.abs(S - S.T).max() <= 1e-13 * np.abs(S).max()            # (tests/test_gpu_parity.py: test_reduced_system)
    return S, g


# ---------------------------------------------------------------------------
# 1. blocks and costs
# ---------------------------------------------------------------------------
def blocks_and_costs(name):
    """ps_debug_reproj_blocks evaluates through reproj_eval_obs, and the cost passes of these scenes (they have constant landmarks)
    likewise: the fetched evaluation of the production passes (reproj_eval_obs_fetched) is not what this case sees -- it is held to
    the reference behind the elimination (cases 2 to 6) and, bit for bit, to the plain evaluation (case 3b)."""
    lp, _ = sc.scene(name)
    ref, loss = block_reference(name)
    dev = device(lp)
    got = dev.debug_reproj_blocks()
    assert all(np.all(np.isfinite(a)) for a in got)
    for lid in np.unique(loss):                            # the rows of each loss under the bound of that loss's own e64
        m = loss == lid
        for k, what in enumerate(('r~', 'J~p', 'J~l')):
            e64 = sampled(lambda r, t: ld.row_err(t[k][m], r[k][m]), block_pairs(name))
            check(name, '{} {} rows'.format(what, LOSS_NAMES[lid]), got[k][m], ref[k][m], e64)
    want_all, want_act = orc.eval_cost(lp), orc.linearize(lp, points_first=False)[2]
    assert ld.costs(lp, np.longdouble) == pytest.approx((want_all, want_act), rel=1e-11)
    for flag, want in ((True, want_all), (False, want_act)):
        c = dev.eval_cost(flag)
        report(name, 'eval_cost({})'.format(flag), abs(c - want) / abs(want), 0., TOL_COST)
        assert abs(c - want) <= TOL_COST * abs(c)
    dev.close()


@pytest.mark.parametrize('name', sc.SCENES)
def test_blocks_and_costs(name):
    blocks_and_costs(name)


# ---------------------------------------------------------------------------
# 2. landmark pass: C^-1 (its inverse Cholesky factor, as the handle keeps it) and c
# ---------------------------------------------------------------------------
LANDMARK_VARIANTS = (('packed', 1, 1), ('packed_no_prefetch', 1, 0), ('16_lane', 0, 1))     # (the 16-lane kernels have no prefetch)


@pytest.mark.parametrize('name', sc.SCENES)
def test_landmark_pass(name):
    lp, _ = sc.scene(name)
    for tag, packed, prefetch in LANDMARK_VARIANTS:
        dev = device(lp)
        dev.set_option('lm_packed', packed)
        dev.set_option('packed_prefetch', prefetch)
        assert dev.packed_runs()[0].shape[0] > 0                        # (the run table exists: no track longer than 16)
        for lam in LAMBDAS:
            dev.linearize(lam)
            check_factors(name, lam, dev, tag)
            check_reduced(name, lam, dev, tag)                         # ... and what the pass's Z rows feed
        dev.close()


# ---------------------------------------------------------------------------
# 3. reduced system: both pose passes x both pair lists x both dampings
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('tiling', ['untiled', 'tiled'])
@pytest.mark.parametrize('name', sc.SCENES)
def test_reduced_system(name, tiling, monkeypatch):
    if tiling == 'tiled':                                              # (the switch of tests/test_gpu_edges.py)
        monkeypatch.setenv('PS_SCHUR_TILE_KB', '256')
        monkeypatch.setenv('PS_SCHUR_TILE_MIN_MB', '0')
    else:
        monkeypatch.setenv('PS_SCHUR_TILE_KB', '0')
    lp, _ = sc.scene(name)
    for prefetch in (1, 0):
        dev = device(lp)
        dev.set_option('pose_prefetch', prefetch)
        for lam in LAMBDAS:
            dev.linearize(lam)
            check_reduced(name, lam, dev, '{} pose_prefetch={}'.format(tiling, prefetch))
        dev.close()


# ---------------------------------------------------------------------------
# 3b. the bit-for-bit claims between variants, apart from the comparisons with the reference
# ---------------------------------------------------------------------------
def _left_behind(lp, option, value):
    dev = device(lp)
    dev.set_option(option, value)
    out = []
    for lam in LAMBDAS:
        dev.linearize(lam)
        out += list(dev.landmark_factors()) + [dev.pose_items()[1]] + list(dev.reduced_system())
    dev.close()
    return out


@pytest.mark.parametrize('option', ['packed_prefetch', 'pose_prefetch'])
@pytest.mark.parametrize('name', sc.SCENES)
def test_prefetch_on_equals_prefetch_off_bit_for_bit(name, option):
    """tests/test_gpu_packed_prefetch.py and tests/test_gpu_pose_prefetch.py: only WHERE a load is issued differs between the option's
    two values, so what the passes leave behind is equal to the last bit.  Their scenes have one camera and diagonal stiffnesses.

    This test found the claim false on mixed_wave, high_group_ids and wide_mixed (packed_prefetch: C^-1 and c up to 6.1e-13
    relative in a third of the landmarks, S up to 1.6e-11; pose_prefetch: partial sums 7.1e-15, S 3.5e-15; every variant within its
    bound of the reference): reproj_eval_s left the fusing of its Jacobian's multiply-adds to the compiler, and its inlined copies
    were not fused alike.  They are explicit now (csrc/ps_math.h); DESIGN.md section 4."""
    lp, _ = sc.scene(name)
    on, off = _left_behind(lp, option, 1), _left_behind(lp, option, 0)
    worst = max(float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0. for a, b in zip(on, off))
    print('{:15s} {} on against off: largest relative difference {:.2e}'.format(name, option, worst))
    for k, (a, b) in enumerate(zip(on, off)):
        assert np.array_equal(a, b), (name, option, k, worst)


# ---------------------------------------------------------------------------
# 4. the step
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def arbiter_step(name):
    """(test_gpu_parity.accurate_solve on the oracle's normal equations in device order, the distance of the oracle's spsolve
    step -- orc.gauss_newton_step -- from it).  A scene with an L1 group on a monocular camera has NaN in the oracle's J~ (the
    weight of the dead third row): there the normal equations are the fp64 twin's, formed from the same blocks with that row's
    scale pinned (tests/test_offbox_host.py holds the two equal where both exist), and solved by the same spsolve."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    lp, _ = sc.scene(name)
    P, b, _ = orc.normal_equations(lp, points_first=False)
    if np.all(np.isfinite(P.data)):
        dx_spsolve, _ = orc.gauss_newton_step(lp, points_first=False, linear_solver='spsolve')
        P = P.toarray()
    else:
        assert np.any(ld.mono_rows(lp) & (lp.obs_groups[lp.obs_grp, 2] == 1.))
        P, b = elimination(name, 0.)[1][0][1].normal_equations()
        dx_spsolve = spla.spsolve(sp.csc_matrix(P), b)
    exact = accurate_solve(P, b)
    return exact, rel_err(dx_spsolve, exact)


def step(name):
    """The landmark part of the step from the device's own pose part, against the reference's back-substitution; the whole step
    against the arbiter.  Every reduced system here has 48 unknowns and is solved directly (0 PCG iterations, asserted): the PCG and
    its non-convergence report are not reached by these scenes -- tests/test_gpu_parity.py and tests/test_gpu_scale.py run it."""
    lp, _ = sc.scene(name)
    ref, pairs, _ = elimination(name, 0.)
    dev = device(lp)
    dev.linearize(0.)
    its, rel = dev.solve_reduced(0., PCG_MAX_ITERS)
    dev.backsub()
    xp, xl = dev.get_dx()
    dev.close()
    assert np.all(np.isfinite(xp)) and np.all(np.isfinite(xl))
    check(name, 'dx_l given dx_p', xl, ref.backsub(xp), sampled(lambda r, t: ld.row_err(t.backsub(xp), r.backsub(xp)), pairs))
    exact, e_ref = arbiter_step(name)
    err = rel_err(np.concatenate([xp.ravel(), xl.ravel()]), exact)
    limit = bound(e_ref, TOL_DX)
    print('{:15s} reduced solve: {} iterations, residual {:.2e}'.format(name, its, rel))
    report(name, 'dx against the arbiter', err, e_ref, limit)
    assert its == 0 and rel <= 10 * PCG_TOL, (its, rel)
    assert err <= limit, (name, err, e_ref)


@pytest.mark.parametrize('name', sc.SCENES)
def test_step(name):
    step(name)


# ---------------------------------------------------------------------------
# 5. a whole iteration
# ---------------------------------------------------------------------------
def whole_iteration(name):
    """The cost gn_iteration returns is the landmark pass's fused sum at the updated parameters: the oracle's cost at the oracle's
    update of the device's own step; so are the parameters."""
    lp, _ = sc.scene(name)
    dev = device(lp)
    cost, nrm, its, rel = dev.gn_iteration(0., 0., PCG_MAX_ITERS, True)
    xp, xl = dev.get_dx()
    poses, points = dev.get_params()
    dev.close()
    dx = np.concatenate([xp.ravel(), xl.ravel()])
    assert abs(nrm - np.linalg.norm(dx)) <= 1e-12 * nrm
    moved = orc.apply_update(lp, dx, points_first=False)
    want = orc.eval_cost(moved)
    report(name, 'cost after the step', abs(cost - want) / abs(want), 0., TOL_COST)
    assert abs(cost - want) <= TOL_COST * abs(want)
    check(name, 'poses after the step', poses, moved.poses, 0., fixed=True)
    check(name, 'points after the step', points, moved.points, 0., fixed=True)


@pytest.mark.parametrize('name', sc.SCENES)
def test_whole_iteration(name):
    whole_iteration(name)


# ---------------------------------------------------------------------------
# 6. items of 512 rows: two observations per thread (k_pose_pass_pf's second trip)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['big_mixed_groups', 'big_wide'])
def test_two_observations_per_thread_against_the_reference(name):
    """What only the pose pass forms -- the diagonal 6 x 6 blocks of S and all of g -- on the problems of
    tests/test_gpu_pose_prefetch.py that mix groups inside every wave (the off-diagonal blocks are the pair kernel's: case 3)."""
    import test_gpu_pose_prefetch as tpp
    lp = {'big_mixed_groups': tpp.big_mixed, 'big_wide': tpp.big_wide}[name]()
    blocks = ld.scaled_blocks(lp, np.longdouble)
    dev = device(lp)
    assert dev.get_option('pose_prefetch') == 1
    for lam in LAMBDAS:
        ref = ld.Elimination(lp, lam, np.longdouble, blocks, diagonal_only=True)
        twin = ld.Elimination(lp, lam, np.float64, diagonal_only=True)
        dev.linearize(lam)
        items = dev.pose_items()[0]
        assert (items[:, 2] - items[:, 1]).max() == 512                 # the two-trip form ran
        rp, ci, vals, g = dev.reduced_system()
        diag = np.stack([vals[rp[r] + np.flatnonzero(ci[rp[r]:rp[r + 1]] == r)[0]] for r in range(dev.nr)])
        check(name, 'diag(S) lambda={}'.format(lam), diag, ref.Sdiag, ld.row_err(twin.Sdiag, ref.Sdiag))
        check(name, 'g lambda={}'.format(lam), g, ref.g, ld.vec_err(twin.g, ref.g), ld.vec_err)
    dev.close()


# ---------------------------------------------------------------------------
# 7. group ids 127 .. 254
# ---------------------------------------------------------------------------
def _everything_cases_1_to_3_read(lp):
    out = []
    dev = device(lp)
    out += list(dev.debug_reproj_blocks())
    out += [np.float64(dev.eval_cost(True)), np.float64(dev.eval_cost(False))]
    dev.close()
    # (packed kernels with both prefetches and with neither, 16-lane kernels with either pose pass)
    for packed, packed_prefetch, pose_prefetch in ((1, 1, 1), (1, 0, 0), (0, 1, 1), (0, 1, 0)):
        dev = device(lp)
        dev.set_option('lm_packed', packed)
        dev.set_option('packed_prefetch', packed_prefetch)
        dev.set_option('pose_prefetch', pose_prefetch)
        for lam in LAMBDAS:
            dev.linearize(lam)
            out += list(dev.landmark_factors()) + list(dev.reduced_system())
        dev.close()
    return out


def test_high_group_ids_give_the_bits_of_the_low_ones():
    """Only the ids differ between mixed_wave and high_group_ids (tests/test_offbox_host.py), and an id is only ever an index into the
    group table: from 128 on it sets the top bit of the observation record's int32 (PS_GRP_OF, csrc/ps_kernels.h; re-packed in
    csrc/ps_host_build.h and ps_host_structure.h)."""
    low = _everything_cases_1_to_3_read(sc.scene('mixed_wave')[0])
    high = _everything_cases_1_to_3_read(sc.scene('high_group_ids')[0])
    assert len(low) == len(high)
    for k, (a, b) in enumerate(zip(low, high)):
        assert np.array_equal(a, b), k


def margins(name):
    """Every figure of the default variant on one scene, printed: tests/parity_margins.py."""
    blocks_and_costs(name)
    dev = device(sc.scene(name)[0])
    for lam in LAMBDAS:
        dev.linearize(lam)
        check_factors(name, lam, dev)
        check_reduced(name, lam, dev)
    dev.close()
    step(name)
    whole_iteration(name)
