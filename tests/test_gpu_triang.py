"""Multi-view triangulation on the device (k_triangulate, csrc/ps_k_triang.h; entry ps_triangulate) against the long-double restatement
of DESIGN.md section 7 (tests/longdouble_triangulation.py), beyond the monocular L2 tables of tests/test_gpu_mono.py and
tests/test_gpu_twoview.py: the depth row of the linear start (stereo and RGB-D), landmarks seen by several camera types, refinement
under Huber, Cauchy and L1 weights, one stiffness per observation (the WIDE instantiation), group ids from 128 on, subsets with
write-back, landmark counts around the 16-landmark workgroup, tracks around the 16-lane stride (up to 80 observations: five per
lane), non-positive disparities.  Scenes: tests/triang_scenes.py.  Run with `-m gpu` on an MI355X.  Every test prints its figure
before it asserts.

Every variable point handed to the device is a sentinel ((1e6, -2e6, 3e6); in a second run another): a result never comes from the
input, the two runs are bit-identical where the status is 0, and a landmark with a non-zero status returns the sentinel
(device_result; every test goes through it).  In tests 1 to 3 the device's status must equal the reference's wherever the reference
decides clearly, so that no landmark escapes a comparison by failing.

Measure: per landmark |p - p_ref| / |p_ref|, the largest over the landmarks (longdouble_triangulation.point_err).
Bounds.  e64 is the distance of the fp64 twin (the same reference code run in fp64) from the long-double result OF THE SAME INPUT,
sampled on the scene and DRAWS = 8 copies with every pose entry and observation one ulp away (longdouble_schur.one_ulp_away), the
largest of the nine; never taken from the device's output.
  1 linear start (refine_iters 0)      max(1e-12, 8 e64) against linear_start
  2 one step (refine_iters 1)          max(1e-12, 8 e64) against p0 + gn_step(p0), over the landmarks whose long-double cost falls by
                                       more than 1e-9 of itself in that step (accept / reject is no rounding decision there) and that
                                       have more than one observation (a single depth-bearing observation is solved exactly by the
                                       linear start: its cost is rounding noise).  Condition: at most 2 % left out per scene, checked
                                       on the reference alone (tests/test_triang_host.py).  far10 and mixed_depth miss it (6.5 % and
                                       6.1 %: at 60 m and more the first step from a noisy disparity often does not lower the cost)
                                       and are left out of this test; tests 1, 3 and 4 keep them.
  3 converged (refine_iters 20)        smooth losses only (a landmark with an L1 observation: test 5).  The long-double Gauss-Newton
                                       step at the device's point, |dx| / |p|, at most max(1e-9, 8 x the same at the fp64 twin's
                                       point, the largest of the nine).  The device's cost in long double at that point is no higher
                                       than at its own linear start, up to the rounding of an fp64 cost (cost_slack).  A landmark
                                       that has run away to where the long-double H has no depth direction (step_size) has no step:
                                       counted, at most 5 % per scene (the twin's largest share: 2.9 % on mixed_depth).
  4 status                             equal to the reference's where it is clear (pivots above 1e-6 relative, |min_cos - cos_min|
                                       above 1e-9, smallest z beyond 1e-6 |p|): at most 5 % unclear per scene, 15 % on far100; and
                                       equal to pyslam_amd/triangulation.py everywhere except on far100.
  5 monotone in refine_iters           0, 1, 5, 20 on mixed_wave, wide_mixed, tracks: status 0 stays 0 (unless the reference says 3
                                       there), the long-double cost does not rise (cost_slack).  Before the kernel stopped calling an
                                       unsolvable refinement step "degenerate" this failed on all three scenes: on mixed_wave 181
                                       landmarks with an L1 observation, having converged, had status 2 after 20 steps.
  6 subsets and write-back             bit for bit
  7 counts, decisions                  as 1 and 4, and by construction

Observed on an MI355X, device / e64 (test 3: device / twin); "left out" and "run away" are the shares under the conditions of tests
2 and 3:

  scene                linear start           one step   left out    step left after 20   run away
  near            8.6e-16 / 1.6e-15  2.3e-16 / 5.5e-16      0 %     1.4e-09 / 1.4e-09       0 %
  base            9.2e-16 / 7.5e-16  1.5e-14 / 1.7e-14      0 %     6.8e-09 / 2.0e-08       0 %
  far10           2.2e-15 / 3.2e-15            not run    6.5 %     4.8e+00 / 4.8e+00       0 %
  mm              8.9e-16 / 7.9e-16  4.2e-14 / 7.1e-14      0 %     1.6e-08 / 6.8e-08       0 %
  mixed_depth     1.6e-15 / 1.9e-15            not run    6.1 %     1.3e+01 / 1.3e+01     2.9 %
  mixed_wave      1.1e-15 / 1.4e-15  2.6e-14 / 6.5e-14      0 %     3.2e-05 / 3.2e-05       0 %
  high_group_ids  1.1e-15 / 1.4e-15  2.6e-14 / 6.5e-14      0 %     3.2e-05 / 3.2e-05       0 %
  wide_mixed      1.1e-15 / 1.4e-15  1.1e-13 / 1.4e-13      0 %     6.9e-05 / 6.9e-05       0 %
  tracks          4.3e-16 / 6.3e-16  2.3e-16 / 1.1e-15      0 %     1.7e-10 / 2.5e-10       0 %
  decisions       3.9e-16 / 5.8e-16  3.8e-16 / 1.7e-15      0 %     3.1e-10 / 6.5e-10       0 %
  counts1         2.5e-16 / 2.7e-16  1.6e-17 / 1.5e-15      0 %     8.5e-11 / 8.5e-11       0 %
  counts15        5.9e-16 / 4.8e-16  2.4e-15 / 4.2e-15      0 %     2.1e-10 / 9.8e-09       0 %
  counts16        5.9e-16 / 5.8e-16  2.4e-15 / 5.5e-15      0 %     2.1e-10 / 9.8e-09       0 %
  counts17        5.9e-16 / 4.6e-16  2.4e-15 / 4.2e-15      0 %     2.1e-10 / 9.8e-09       0 %
  counts33        6.1e-16 / 9.5e-16  1.3e-14 / 2.2e-14      0 %     1.1e-09 / 9.8e-09       0 %

On far10 and mixed_depth neither the device nor the twin is converged after 20 steps: landmarks whose disparities are noise around
zero have their minimiser at infinity and are on their way out.  Under Huber and Cauchy IRLS converges linearly (3e-5 left on the
mixed scenes).  Status: unclear 0 % on every scene (far100 included; decisions at its 1 degree: one landmark, on purpose); counts
[ok, few, degenerate, behind] at 5 steps: near, base, mm [574, 0, 0, 0], far10 [566, 0, 0, 8], mixed_depth [526, 0, 0, 48], the mixed
scenes [571, 0, 3, 0], far100 [354, 0, 0, 220].  Test 5: no landmark lost, the cost never higher.  Test 6: eval_cost after the
write-back within 4e-16 of the oracle's.  tools/mono_bench.py, parent / change: 50 000 landmarks 0.231 / 0.234 ms for the linear
start, 0.319 / 0.322 ms with five steps (0.0176 / 0.0176 ms per step).  tests/parity_margins.py prints these figures; DESIGN.md
section 4 has the table too.
"""
import functools

import numpy as np
import pytest

import longdouble_schur as ld
import longdouble_triangulation as lt
import offbox_scenes as sc
import triang_scenes as ts
from oracle import gn_oracle as orc
from pyslam_amd import triangulation

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ld.LONGDOUBLE_OK, reason=ld.LONGDOUBLE_SKIP)]

FACTOR = 8
FLOOR = 1e-12
FLOOR_CONVERGED = 1e-9
DRAWS = 8
MIN_PARALLAX_DEG = 1.0
ITERS = (0, 1, 5, 20)
MIN_DECREASE = 1e-9
ONE_STEP_LEFT_OUT = 0.02
RUNAWAY_PIVOT = 1e-12             # (depth known 1e-6 as well as bearing: below, the step rests on digits an fp64 H does not have)
RUNAWAY_SHARE = 0.05              # (the share test 4 allows the reference to leave undecided; the twin's largest: 2.9 % on mixed_depth)
UNCLEAR = 0.05
UNCLEAR_FAR100 = 0.15
ONE_STEP_SCENES = tuple(n for n in ts.SCENES if n not in ('far10', 'mixed_depth'))
MONOTONE_SCENES = ('mixed_wave', 'wide_mixed', 'tracks')
L1 = 1


def bound(e64, floor=FLOOR):
    return max(floor, FACTOR * e64)


# ---------------------------------------------------------------------------
# references: once per scene, shared, never written to (all on the host: tests/test_triang_host.py checks their conditions)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problems(name):
    lp = ts.scene(name)
    return [lp] + [ld.one_ulp_away(lp, k) for k in range(DRAWS)]


@functools.lru_cache(maxsize=None)
def reference(name, iters, mp=MIN_PARALLAX_DEG):
    """(points, status, clear, lin) of the scene in long double."""
    return lt.triangulate(ts.scene(name), iters, mp)


@functools.lru_cache(maxsize=None)
def linear_e64(name, mp=MIN_PARALLAX_DEG):
    e = 0.
    for q in problems(name):
        ref, st, _, _ = lt.triangulate(q, 0, mp)
        twin, st64, _, _ = lt.triangulate(q, 0, mp, np.float64)
        e = max(e, lt.point_err(twin, ref, (st == 0) & (st64 == 0)))
    return e


def _one_step(q, dtype):
    """(p0 + gn_step(p0), included) of the tables q in `dtype`."""
    _, st, _, lin = lt.triangulate(q, 0, MIN_PARALLAX_DEG, dtype)
    act = st == 0
    p0 = np.where(act[:, None], lin.point, 1.)
    ev = lt.evaluate(q, p0, dtype)
    dx, ok = lt.gn_step(q, p0, dtype, ev)
    p1 = p0 + dx
    with np.errstate(all='ignore'):
        falls = ev[0] - lt.evaluate(q, p1, dtype)[0] > MIN_DECREASE * ev[0]
    return p1, act, act & ok & falls & (lin.nobs > 1), lin.nobs


@functools.lru_cache(maxsize=None)
def one_step(name):
    """(p1 in long double, included, share left out among the landmarks with more than one observation, e64)."""
    e, out = 0., None
    for q in problems(name):
        p1, act, inc, nobs = _one_step(q, np.longdouble)
        twin, _, inc64, _ = _one_step(q, np.float64)
        e = max(e, lt.point_err(twin, p1, inc & inc64))
        if out is None:
            asked = act & (nobs > 1)
            out = (p1, inc, 1. - inc[asked].mean() if asked.any() else 0.)
    return out + (e,)


def smooth(name):
    return ~ts.has_loss(ts.scene(name), L1)


def step_size(lp, p, rows):
    """(the largest |dx| / |p| of the long-double Gauss-Newton step at p over `rows`, the share of `rows` without a step).  A
    landmark has no step where a pivot of its long-double H is below RUNAWAY_PIVOT of its diagonal entry: the observed disparities
    of a landmark at 600 m and more are noise around zero, the minimiser of its cost lies at infinity, and the refinement runs
    out along the ray (1e11 m and more) until the cost is flat -- there the depth direction of H is zero to rounding."""
    if not rows.any():
        return 0., 0.
    p = np.where(rows[:, None], np.asarray(p, dtype=np.longdouble), 1.)
    _, H, g, _, _ = lt.evaluate(lp, p)
    dx, piv, ok = lt.ldl_solve(H, -g)
    with np.errstate(all='ignore'):
        has_step = rows & ok & (piv.min(axis=1) > RUNAWAY_PIVOT) & np.all(np.isfinite(dx), axis=1)
    return lt.point_err(p + np.where(has_step[:, None], dx, 0), p, has_step), 1. - has_step[rows].mean()


@functools.lru_cache(maxsize=None)
def converged_twin(name):
    """(the step left at the fp64 twin's point after 20 steps (smooth landmarks), the share of them without a step): the largest
    over the scene and its copies."""
    e, gone = 0., 0.
    for q in problems(name):
        p, st, _, _ = lt.triangulate(q, 20, MIN_PARALLAX_DEG, np.float64)
        left, share = step_size(q, p, (st == 0) & smooth(name))
        e, gone = max(e, left), max(gone, share)
    return e, gone


# ---------------------------------------------------------------------------
# the device: one handle per scene, every call twice from two sentinels
# ---------------------------------------------------------------------------
_HANDLES = {}


def handle(name):
    from pyslam_amd.device import DeviceProblem
    if name not in _HANDLES:
        _HANDLES[name] = DeviceProblem(ts.scene(name))
    return _HANDLES[name]


@pytest.fixture(scope='module', autouse=True)
def _close_handles():
    yield
    for dev in _HANDLES.values():
        dev.close()
    _HANDLES.clear()


@functools.lru_cache(maxsize=None)
def device_result(name, iters, mp=MIN_PARALLAX_DEG):
    lp = ts.scene(name)
    dev = handle(name)
    runs = []
    for which in (0, 1):
        start = ts.with_sentinel(lp, which)
        dev.set_params(start.poses, start.points)
        pts, st = dev.triangulate(None, iters, mp, write_back=False)
        assert np.array_equal(dev.get_params()[1], start.points)             # (write_back False: nothing moves)
        assert np.all(np.isfinite(pts)), (name, iters)
        assert np.all(pts[st != 0] == ts.SENTINELS[which]) and set(np.unique(st)) <= {0, 1, 2, 3}
        assert not np.any(np.all(pts[st == 0] == ts.SENTINELS[which], axis=1))
        runs.append((pts, st))
    (a, sa), (b, sb) = runs
    assert np.array_equal(sa, sb) and np.array_equal(a[sa == 0], b[sa == 0]), (name, iters)
    return a, sa


def agreed_rows(name, iters, mp=MIN_PARALLAX_DEG):
    """The device's status equals the reference's wherever that is clear; -> (device points, rows where both are 0)."""
    pts, st = device_result(name, iters, mp)
    _, rst, clear, _ = reference(name, iters, mp)
    wrong = np.flatnonzero((st != rst) & clear)
    print('{:15s} refine_iters {:2d}: status counts {} (reference {}), unclear {} of {}, differing where clear {}'.format(
        name, iters, np.bincount(st, minlength=4).tolist(), np.bincount(rst, minlength=4).tolist(), int((~clear).sum()), clear.size, wrong.size))
    assert wrong.size == 0, (name, iters, wrong[:10], st[wrong[:10]], rst[wrong[:10]])
    return pts, (st == 0) & (rst == 0)


def report(name, what, err, e64, limit):
    print('{:15s} {:34s} device {:.2e}   e64 {:.2e}   bound {:.2e}'.format(name, what, err, e64, limit))


# ---------------------------------------------------------------------------
# 1. linear start
# ---------------------------------------------------------------------------
def linear_start(name):
    pts, rows = agreed_rows(name, 0)
    err, e64 = lt.point_err(pts, reference(name, 0)[3].point, rows), linear_e64(name)
    report(name, 'linear start ({} landmarks)'.format(int(rows.sum())), err, e64, bound(e64))
    assert rows.any() and err <= bound(e64), (name, err, e64)


@pytest.mark.parametrize('name', ts.SCENES)
def test_linear_start(name):
    linear_start(name)


# ---------------------------------------------------------------------------
# 2. one step
# ---------------------------------------------------------------------------
def one_refinement_step(name):
    pts, rows = agreed_rows(name, 1)
    p1, inc, left_out, e64 = one_step(name)
    print('{:15s} one step: {:.1%} of the landmarks left out'.format(name, left_out))
    assert left_out <= ONE_STEP_LEFT_OUT
    assert not (inc & ~rows & reference(name, 1)[2]).any()
    inc = inc & rows
    err = lt.point_err(pts, p1, inc)
    report(name, 'one step ({} landmarks)'.format(int(inc.sum())), err, e64, bound(e64))
    assert inc.any() and err <= bound(e64), (name, err, e64)


@pytest.mark.parametrize('name', ONE_STEP_SCENES)
def test_one_step(name):
    one_refinement_step(name)


# ---------------------------------------------------------------------------
# 3. converged
# ---------------------------------------------------------------------------
def costs_at(name, pts, rows):
    """(long-double cost per landmark at the device's points, the slack of an fp64 comparison of two such costs); rows only."""
    lp = ts.scene(name)
    cost, _, _, _, r1 = lt.evaluate(lp, np.where(rows[:, None], pts, 1.))
    return cost, lt.cost_slack(lp, r1)


def converged(name):
    lp = ts.scene(name)
    pts, rows = agreed_rows(name, 20)
    rows = rows & smooth(name)
    (left, no_step), (twin, twin_no_step) = step_size(lp, pts, rows), converged_twin(name)
    limit = bound(twin, FLOOR_CONVERGED)
    report(name, 'step left after 20 ({} landmarks)'.format(int(rows.sum())), left, twin, limit)
    print('{:15s} run away to where H has no depth direction: {:.1%} of them (twin {:.1%})'.format(name, no_step, twin_no_step))
    assert no_step <= RUNAWAY_SHARE
    start, st0 = device_result(name, 0)
    assert np.all(st0[rows] == 0)
    c20, slack = costs_at(name, pts, rows)
    c0, slack0 = costs_at(name, start, rows)
    rise = float(((c20 - c0) / np.maximum(slack, slack0))[rows].max()) if rows.any() else 0.
    print('{:15s} cost after 20 steps against the linear start: largest rise {:.2e} of the slack'.format(name, rise))
    assert rows.any() and left <= limit, (name, left, twin)
    assert rise <= 1.


@pytest.mark.parametrize('name', ts.SCENES)
def test_converged(name):
    converged(name)


# ---------------------------------------------------------------------------
# 4. status
# ---------------------------------------------------------------------------
def status(name, mp=MIN_PARALLAX_DEG):
    for iters in (0, 5):
        agreed_rows(name, iters, mp)
        clear = reference(name, iters, mp)[2]
        assert 1. - clear.mean() <= (UNCLEAR_FAR100 if name == 'far100' else UNCLEAR)
        if name != 'far100':
            st = device_result(name, iters, mp)[1]
            want = triangulation.triangulate(ts.scene(name), None, iters, mp)[1]
            assert np.array_equal(st, want), (name, iters, np.flatnonzero(st != want)[:10])


@pytest.mark.parametrize('name', ts.SCENES + ts.STATUS_ONLY)
def test_status(name):
    """(decisions: asked for 0.9 degrees, clear of the 1 degree its two rays are built at -- test_decisions is about that threshold.)"""
    status(name, 0.9 if name == 'decisions' else MIN_PARALLAX_DEG)


def test_high_group_ids_give_the_bits_of_the_low_ones():
    """Only the ids differ between mixed_wave and high_group_ids, and an id is only ever an index into the group table (from 128 on
    it sets the top bit of the observation record's group byte: PS_GRP_OF)."""
    for iters in ITERS:
        (low, sl), (high, sh) = device_result('mixed_wave', iters), device_result('high_group_ids', iters)
        assert np.array_equal(sl, sh) and np.array_equal(low, high), iters


def test_status_of_long_tracks_at_the_parallax_gate():
    """With this minimum parallax the all-mono tracks of 31 and more observations have it only between two observations in slots
    16 and up (tests/test_triang_host.py): the all-pairs loop of a lane's second and later observations."""
    status('tracks', ts.TRACKS_PARALLAX_GATE)
    st = device_result('tracks', 5, ts.TRACKS_PARALLAX_GATE)[1]
    print('tracks at {} degrees: status {}'.format(ts.TRACKS_PARALLAX_GATE, st.tolist()))
    assert not st.any()


# ---------------------------------------------------------------------------
# 5. monotone in refine_iters
# ---------------------------------------------------------------------------
def monotone(name):
    results = [device_result(name, it) for it in ITERS]
    lost, worst = np.zeros(results[0][1].size, dtype=bool), 0.
    for a in range(len(ITERS)):
        for b in range(a + 1, len(ITERS)):
            (pa, sa), (pb, sb) = results[a], results[b]
            said_behind = reference(name, ITERS[b])[1] == lt.BEHIND
            gone = (sa == 0) & (sb != 0) & ~said_behind
            lost |= gone
            if gone.any():
                print('{:15s} status 0 at {} steps, not at {}: landmarks {} -> status {}'.format(
                    name, ITERS[a], ITERS[b], np.flatnonzero(gone)[:8].tolist(), sb[gone][:8].tolist()))
            both = (sa == 0) & (sb == 0)
            if both.any():
                ca, slack_a = costs_at(name, pa, both)
                cb, slack_b = costs_at(name, pb, both)
                worst = max(worst, float(((cb - ca) / np.maximum(slack_a, slack_b))[both].max()))
    print('{:15s} over refine_iters {}: {} landmarks lost, largest rise of the long-double cost {:.2e} of the slack'.format(
        name, ITERS, int(lost.sum()), worst))
    assert not lost.any()
    assert worst <= 1.


@pytest.mark.parametrize('name', MONOTONE_SCENES)
def test_monotone_in_refine_iters(name):
    monotone(name)


# ---------------------------------------------------------------------------
# 6. subsets and write-back
# ---------------------------------------------------------------------------
def test_subsets_and_write_back():
    from pyslam_amd.device import DeviceProblem
    name, iters = 'mixed_wave', 5
    lp = ts.scene(name)
    nv = lp.num_var_points
    full, fst = device_result(name, iters)
    assert (fst != 0).any() and (fst == 0).any()
    point_of_vid = np.empty(nv, dtype=np.int64)
    var = np.flatnonzero(lp.point_vid >= 0)
    point_of_vid[lp.point_vid[var]] = var
    start = sc.scene(name)[0].points                                     # the scene's own start, off the observations' truth
    dev = DeviceProblem(lp)
    subsets = dict(permutation=np.random.default_rng(7).permutation(nv), reverse=np.arange(nv)[::-1], strided_half=np.arange(0, nv, 2))
    for what, vids in subsets.items():
        for write_back in (False, True):
            before = start.copy()
            before[point_of_vid[vids]] = ts.SENTINELS[0]
            dev.set_params(lp.poses, before)
            pts, st = dev.triangulate(vids, iters, MIN_PARALLAX_DEG, write_back=write_back)
            print('{} write_back={}: {} landmarks, {} with status 0'.format(what, write_back, vids.size, int((st == 0).sum())))
            assert np.array_equal(st, fst[vids]) and np.array_equal(pts[st == 0], full[vids][st == 0])
            assert np.all(pts[st != 0] == ts.SENTINELS[0])
            poses, points = dev.get_params()
            want = before.copy()
            if write_back:
                want[point_of_vid[vids[st == 0]]] = pts[st == 0]
            assert np.array_equal(poses, lp.poses) and np.array_equal(points, want)
            if write_back:
                moved = lp.copy()
                moved.points = want
                cost, oracle = dev.eval_cost(True), orc.eval_cost(moved)
                print('    eval_cost after the write-back: device {:.12e} oracle {:.12e} rel {:.1e}'.format(cost, oracle, abs(cost - oracle) / oracle))
                assert abs(cost - oracle) <= 1e-10 * oracle
                dev.set_params(lp.poses, before)
                again, st2 = dev.triangulate(vids, iters, MIN_PARALLAX_DEG, write_back=True)
                assert np.array_equal(again, pts) and np.array_equal(st2, st)
                assert np.array_equal(dev.get_params()[1], want)
    dev.close()


# ---------------------------------------------------------------------------
# 7. counts and decisions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n', ts.COUNTS)
def test_counts(n):
    """pyslam_amd.triangulate_tables (its own handle, -1 for a constant landmark) on n variable landmarks: what the all-landmarks
    call of `base` gives for the same landmarks, bit for bit (a landmark's result depends on nothing but its own observations)."""
    from pyslam_amd import triangulate_tables
    name = 'counts{}'.format(n)
    lp = ts.scene(name)
    const = lp.point_vid < 0
    assert lp.num_var_points == n and const.sum() == (ts.COUNTS_CONSTANT if n == max(ts.COUNTS) else 0)
    for iters in (0, 5):
        pts, st = triangulate_tables(lp, iters, MIN_PARALLAX_DEG)
        assert pts.shape == (lp.num_points, 3) and np.all(st[const] == -1) and np.array_equal(pts[const], lp.points[const])
        want, wst = device_result('base', iters)
        print('{} refine_iters {}: status {}'.format(name, iters, np.bincount(st[~const], minlength=4).tolist()))
        assert np.array_equal(st[~const], wst[:n]) and np.array_equal(pts[~const][st[~const] == 0], want[:n][wst[:n] == 0])
        ref, rst, clear, _ = reference(name, iters)
        assert np.array_equal(st[~const][clear], rst[clear])
    linear_start(name)


def test_decisions():
    lp, named, _ = ts.decisions()
    lin = reference('decisions', 0)[3]
    theta = float(np.degrees(np.arccos(lin.min_cos[named['two_rays']])))
    late = float(np.degrees(np.arccos(lin.min_cos[named['late_pair']])))
    print('decisions: two rays at {:.15f} degrees, the late pair at {:.6f}'.format(theta, late))
    assert abs(theta - ts.DECISION_ANGLE_DEG) < 1e-9 and late > 1.1 * theta
    known = dict(two_rays_and_stereo=0, one_mono=1, one_stereo=0, one_rgbd=0, behind=3, late_pair=0)
    special = np.array([named['zero_disparity'], named['negative_disparity']])
    for mp, two_rays in ((theta * (1. - 1e-6), 0), (theta * (1. + 1e-6), 2)):
        for iters in (0, 5):
            pts, st = device_result('decisions', iters, mp)
            print('min_parallax_deg {:.9f} refine_iters {}: {}'.format(mp, iters, {k: int(st[v]) for k, v in named.items()}))
            assert st[named['two_rays']] == two_rays
            for k, want in known.items():
                assert st[named[k]] == want, (k, mp, iters)
            # non-positive disparities: refused, or a finite point in front of its cameras
            _, _, _, min_z, _ = lt.evaluate(lp, np.where((st == 0)[:, None], pts, 1.))
            assert np.all((st[special] != 0) | (min_z[special] > 0))
            # the others: the reference's status, and its linear start under test 1's bound
            ref, rst, clear, rlin = reference('decisions', iters, mp)
            others = np.setdiff1d(np.arange(st.size), np.concatenate([special, [named['two_rays']]]))
            assert clear[others].all() and np.array_equal(st[others], rst[others])
            if iters == 0:
                rows = np.zeros(st.size, dtype=bool)
                rows[others] = True
                rows &= st == 0
                err, e64 = lt.point_err(pts, rlin.point, rows), linear_e64('decisions', mp)
                report('decisions', 'linear start beside the refused', err, e64, bound(e64))
                assert err <= bound(e64)


def margins(name):
    """Every figure of one scene, printed: tests/parity_margins.py."""
    linear_start(name)
    if name in ONE_STEP_SCENES:
        one_refinement_step(name)
    converged(name)
    status(name, 0.9 if name == 'decisions' else MIN_PARALLAX_DEG)
    if name in MONOTONE_SCENES:
        monotone(name)
