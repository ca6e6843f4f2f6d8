"""The pose-factor kernels on the device outside synthetic.pose_graph's helix, against a long-double reference
(tests/longdouble_posegraph.py) -- never against another device variant; the bit-for-bit claims are asserted beside that, separately.
Scenes: tests/posegraph_scenes.py (error rotations from 0 to 3.1415 rad through both 1e-8 branches, kilometres and millimetres,
rotation-only rows, 64-factor workgroups that mix edges, priors and seven stiffness / loss groups, every tail of the wave's 16-factor
share, duplicate / reversed / constant-ended edges, a star, priors only, a bundle adjustment with odometry, 120 unknowns for the folded
CG).  Kernels: k_factor_pass, k_factor_assemble (csrc/ps_k_linearize.h), k_cost_factors, k_update_poses (csrc/ps_k_tail.h), se3_log /
se3_exp / se2_log / se2_exp and the losses (csrc/ps_math.h).  Counterpart of reference pyslam/residuals/pose_to_pose_residual.py:12-32,
pose_residual.py:12-27 and problem.py:332-360, :110-128, :186.

Nothing closer to pi than 3.1415 is tested: from pi - 1e-6 the definition itself carries no digits in fp64 (the error of acos / sin grows
as 2^-53 / (pi - theta)^2), and the reference pipeline shares it.  L1 at a zero residual is NaN by definition and is not tested either.

Steps.  Every definite scene: one gn_iteration without line search, then the same step scaled through apply_update to 2.5 rad and to
0.5e-8 rad (both branches of exp in k_update_poses).  The handle whose PARAMETERS are moved by 2.5 rad first, so that the Gauss-Newton step
itself is large, runs on the all-L2 scenes alone (angles, km, mm, near_pi: elsewhere a start that far need not leave a definite system)
and asserts |phi| > 1 of its step (observed 3.8 .. 5.5), not a value.

Measure.  Per factor row (r~, J~_1, J~_2), per D x D block of S, per D-vector of g, per pose row: the largest absolute difference over
max(the row's own largest reference entry, u).  u is the row's rounding scale: for a factor the infinity norm of its stiffness times
max(1, the largest |t| among T_1, T_2, T_obs) -- the size of the numbers whose rounded products the row was formed from (a row can be
all cancellation: an error rotation of 1e-10 carries the 1e-16 of the triple product); for a block of S or a vector of g the largest
u_f max(|J~_f|, u_f) among the factors that touch it (longdouble_posegraph.system_floors); for a pose row max(1, |t|).  The whole
step: the largest difference over the step's largest entry.  conftest.rel_err over a whole table is never used.

Bounds.  max(TOL_BLOCK, 8 e64) for blocks, S, g and the retracted poses, e64 being the largest distance of the fp64 twin from the
long-double twin on the same input over the scene and eight one-ulp copies (posegraph_scenes.e64: tests/test_posegraph_host.py prints
it), in the same measure, r~ / J~ per (loss, factor kind, log branch) class.  Cost: TOL_COST.  Whole dx: max(TOL_DX, 8 e_ref), e_ref the
distance of a sparse LU step on the fp64 twin's system from test_gpu_parity.accurate_solve on the long-double system.  No bound comes
from the device's output.  The `exact` scene's r~, g and step are rounding noise and are held absolutely beside the row measure (which holds
them through its floor only): 32 x 2^-53 of the rounding scale, the step behind the reference's S^-1.  By the reference alone every scene sits on the 1e-12 floor except near_pi (8 e64 = 6e-8 for r~, 2e-8 for g),
mixed_wg (its L1 rows: J~ 5e-12, S 1.1e-11 for SE(3), 1.7e-12 for SE(2): the weight 1 / |r_k| hands a residual component's relative
error to its whole row) and mixed_ba (g 1e-11, S 3.4e-12: the landmark elimination's own error); tests/test_posegraph_host.py.

Branches.  Where the two branches of se3_log's `ang <= 1e-8` differ by more than 64 x 2^-53 in the rotation part of a factor (L2, unit
stiffness: angles, km, mm, near_pi), the device must lie nearer the fp64 twin forced into the branch the fp64 predicate takes than the
twin forced into the other (a defect at the band is a different
BRANCH from fp64 numpy on the same input, not a different last bit).

Observed on an MI355X, "device / e64" (the bound is max(1e-12, 8 e64); per scene the entry with the least margin over both groups,
both dampings, every (loss, kind, branch) class and every step variant; dx: device / e_ref against its arbiter; cost: the worse of
eval_cost(True) and eval_cost(False), relative).  tails = tails1 .. tails257, structure = dup, const_middle, const_pair, star70,
prior_every, priors_only; tests/parity_margins.py prints every scene on its own:

  scene                  r~                 J~                  S                  g                 dx              poses        cost
  angles    1.2e-14/3.3e-14    1.6e-16/2.1e-16    3.2e-16/3.9e-16    2.7e-15/6.5e-15    4.0e-14/3.6e-15    2.0e-10/2.0e-10     4.3e-15
  km        2.0e-15/3.0e-15    2.0e-16/3.0e-16    3.4e-16/4.5e-16    5.6e-16/1.1e-15    1.4e-08/5.1e-09    1.3e-10/1.3e-10     1.9e-15
  mm        6.2e-14/1.1e-13    1.2e-16/1.2e-16    3.5e-16/4.1e-16    6.2e-14/1.1e-13    4.6e-14/1.7e-14    1.8e-13/1.8e-13     3.6e-14
  rot_only  3.2e-14/6.3e-14    7.2e-16/7.5e-16    1.0e-15/2.3e-15    3.7e-16/7.3e-16    1.8e-13/2.6e-14    2.4e-15/2.4e-15     0
  mixed_wg  9.1e-16/1.4e-15    5.2e-13/6.8e-13    1.0e-12/1.4e-12    7.2e-17/1.2e-16    1.1e-14/7.8e-15    6.2e-15/6.2e-15     2.1e-16
  tails     2.9e-16/2.7e-16    1.2e-15/1.8e-15    1.5e-15/6.1e-16    2.5e-16/1.4e-16    9.2e-13/1.9e-12    3.5e-15/3.7e-15     4.9e-16
  structure 2.0e-16/2.7e-16    9.4e-16/9.3e-16    7.4e-16/7.4e-16    1.6e-16/2.0e-16    6.7e-14/1.3e-12    6.7e-16/6.7e-16     3.3e-16
  exact     9.7e-17/1.5e-16    4.6e-16/4.9e-16    1.0e-15/1.1e-15    1.1e-16/1.2e-16    |dx| 5.6e-16 abs.  3.2e-16/3.3e-16     cost 1e-31
  near_pi   2.6e-09/6.0e-09    1.1e-16/2.3e-16    2.5e-16/5.1e-16    1.2e-09/2.6e-09    3.4e-09/4.1e-09    4.7e-16/4.5e-16     2.8e-09
  mixed_ba  5.4e-17/9.1e-17    2.7e-16/3.9e-16    2.0e-14/4.3e-13    3.4e-13/1.2e-12    7.6e-14/1.5e-12    7.1e-16/7.4e-16     < 1e-16
  cg_size   1.8e-16/2.5e-16    3.0e-15/5.9e-15    4.8e-15/9.1e-15    5.6e-17/1.3e-16    9.6e-15/2.5e-14    3.3e-16/3.5e-16     2.1e-16

The poses column of angles and km is the step scaled to 2.5 rad: a pose whose own |phi step| is ~1e-7 there gets (1 - cos) / |phi| with
2^-53 / |phi|^2 of relative error, from the device and from fp64 numpy alike (device = e64 to two digits).  cg_size: 98 iterations of the
folded CG; every system of at most 90 unknowns is solved directly (0 iterations).  No defect was found: nothing in csrc/ changed.

That the checks can fail (each change made in a scratch copy of the kernels, one run of the narrowest test, not kept): (a) phase 2 of
k_factor_pass with the group of the workgroup's first factor fails test_factor_blocks[mixed_wg] (J~_1 off by 0.48); (b) k_factor_assemble
without the transpose flag fails test_reduced_system[dup, tails17]; (c) (1 + lambda) on every entry of a diagonal slot fails
test_reduced_system[dup] at lambda = 1e-3; (d) se3_log's small branch up to 1e-6 fails test_factor_blocks[angles-se3, km-se3, mm-se3] in the branch check
alone, at the factor of 3e-7 that was added to ANGLES for this (1.2e-14 .. 2.2e-14 from the fp64 twin of the predicate's branch, 4e-17 ..
7e-17 from the other's; the row measure with its floor u cannot see it: 2e-13 < 1e-12 even at 1e-6); (e) k_cost_factors skipping a factor with EITHER end constant fails test_costs on
const_middle, const_pair and tails17.  The earlier tests (tests/test_gpu_blocks.py, the pose-graph cases of tests/test_gpu_parity.py and
tests/test_gpu_edges.py, 48 tests) pass under (c), (d) and (e); they fail under (a) -- the goldens' prior has a stiffness group of its
own -- and under (b) -- every edge's lower block is the transposed one."""
import functools

import numpy as np
import pytest

import longdouble_posegraph as ldp
import posegraph_scenes as sc
from test_gpu_parity import TOL_BLOCK, TOL_COST, TOL_DX, accurate_solve

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ldp.LONGDOUBLE_OK, reason=ldp.LONGDOUBLE_SKIP)]

LD = sc.LD
CASES = sc.cases()
PCG_MAX_ITERS = 2000
INDEFINITE = ()                       # scenes whose reduced system is not definite (asserted on the reference): no step is taken there
EPS = 2. ** -53


def _id(c):
    return '{}-se{}'.format(c[0], 3 if c[1] == 6 else 2)


def device(lp):
    from pyslam_amd.device import DeviceProblem
    return DeviceProblem(lp)


def report(case, what, err, e64, limit):
    print('{:13s} se{} {:34s} device {:.2e}   e64 {:.2e}   bound {:.2e}'.format(case[0], case[1] // 3 + 1, what, err, e64, limit))


def check(case, what, err, e64, floor=TOL_BLOCK):
    limit = sc.bound(e64, floor)
    report(case, what, err, e64, limit)
    assert err <= limit, (case, what, err, e64, limit)


# ---------------------------------------------------------------------------
# 1. the tap: r~, J~_1, J~_2 per factor
# ---------------------------------------------------------------------------
def classes(fac):
    """{(loss, kind, branch): rows}: kind 'edge' / 'prior', branch 'vee' (ang <= 1e-8, or SE(2)'s |phi| <= 1e-8) / 'log'."""
    small = fac.small_angle if fac.lp.dof == 6 else fac.small_phi
    out = {}
    for f in range(fac.F):
        key = (ldp.LOSS_NAMES[fac.loss[f]], 'edge' if fac.i[f] >= 0 else 'prior', 'vee' if small[f] else 'log')
        out.setdefault(key, []).append(f)
    return {k: np.array(v) for k, v in out.items()}


def blocks(case):
    lp, _ = sc.scene(*case)
    pairs = sc.factor_pairs(*case)
    ref = pairs[0][0]
    u = ldp.factor_scale(lp)
    dev = device(lp)
    got = dict(zip(('rt', 'J1', 'J2'), dev.debug_factor_blocks()))
    dev.close()
    assert all(np.all(np.isfinite(a)) for a in got.values())
    assert np.all(got['J1'][ref.i < 0] == 0.)                                   # J~_1 of a prior
    absent = ~ref.present
    assert np.all(got['rt'][absent] == 0.) and np.all(got['J1'][absent] == 0.) and np.all(got['J2'][absent] == 0.)
    cls = classes(ref)
    if case[0] in ('angles', 'km', 'mm') and lp.dof == 6:
        # the band: a factor whose angle is above 1e-8 sits in vee(R - I) by the fp64 predicate, as an L2 class judged below
        wanted = np.abs(sc.scene(*case)[1]['angle'])
        in_vee = np.concatenate([rows for key, rows in cls.items() if key[0] == 'L2' and key[2] == 'vee'])
        assert np.any(wanted[in_vee] > 1e-8) and np.any(wanted[np.setdiff1d(np.arange(ref.F), in_vee)] < 3e-8), case
    if case[0] == 'exact':
        # r~ is rounding noise: three rounded transforms are multiplied (each entry a sum of at most four products, about four ulps of
        # u per product and level) and the stiffness row adds D terms -- 32 x 2^-53 u.  (The row measure below holds it to the 1e-12
        # floor only.)
        worst = float((np.abs(got['rt']).max(axis=1) / u).max())
        print('{:13s} se{} {:34s} device {:.2e}   bound {:.2e} (absolute, over u)'.format(case[0], lp.dof // 3 + 1, '|r~|', worst, 32 * EPS))
        assert worst <= 32 * EPS, (case, worst)
    for key, rows in sorted(cls.items()):
        for what in ('rt', 'J1', 'J2'):
            # (the class's rows in every draw: a copy one ulp away has the same factors, and nearly always the same branches)
            e64 = max(ldp.row_err(getattr(t, what)[rows], getattr(r, what)[rows], ldp.factor_scale(r.lp)[rows]) for r, t in pairs)
            err = ldp.row_err(got[what][rows], getattr(ref, what)[rows], u[rows])
            check(case, '{} {} {} {}'.format(what, *key), err, e64)
    if lp.dof == 6 and np.all(lp.edge_groups[:, 1] == ldp.L2) and np.all(lp.stiffd == np.identity(6).ravel()):
        # the branch the device took (module docstring).  Under L2 and a unit stiffness r~ is xi; its rotation part is formed from
        # rotation entries alone (scale 1, whatever the translations), and an fp64 evaluation in the same branch agrees with another to a
        # few 2^-53: a factor is judged where the branches lie more than 64 x 2^-53 apart there (from about 2e-7 rad on, and in the band)
        forced = {b: ldp.Factors(lp, np.float64, force={'log_angle': b}).rt[:, 3:] for b in (True, False)}
        with np.errstate(invalid='ignore'):
            apart = np.abs(forced[True] - forced[False]).max(axis=1)
            judged = np.flatnonzero(np.isfinite(apart) & (apart > 64 * EPS))
        for f in judged:
            mine, other = forced[bool(ref.small_angle[f])][f], forced[not ref.small_angle[f]][f]
            d_mine, d_other = np.abs(got['rt'][f, 3:] - mine).max(), np.abs(got['rt'][f, 3:] - other).max()
            assert d_mine < d_other, (case, 'factor {} took the other branch of se3_log'.format(f), d_mine, d_other)
        print('{:13s} branch of se3_log judged on {} of {} factors'.format(case[0], len(judged), ref.F))
        if case[0] in ('angles', 'km', 'mm'):   # ... among them factors below 1e-6 that belong to the logarithm
            wanted = np.abs(sc.scene(*case)[1]['angle'])
            assert np.any((wanted[judged] > 1e-7) & (wanted[judged] < 1e-6)), (case, wanted[judged])


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_factor_blocks(case):
    blocks(case)


# ---------------------------------------------------------------------------
# 2. S and g
# ---------------------------------------------------------------------------
def reduced(case, dev, lam, tag=''):
    lp, info = sc.scene(*case)
    d, nr = lp.dof, lp.num_reduced
    pairs, syspairs = sc.factor_pairs(*case), sc.system_pairs(case[0], case[1], lam)
    ref_fac, (Sr, gr, touched) = pairs[0][0], syspairs[0][0]
    e64 = sc.e64(*case)
    dev.linearize(lam)
    S, g = dev.reduced_dense()
    assert np.all(np.isfinite(S)) and np.all(np.isfinite(g))
    eS, eg = sc.err_system((S, g), (Sr, gr), ref_fac)
    check(case, 'S lambda={} {}'.format(lam, tag), eS, e64['S', lam])
    check(case, 'g lambda={} {}'.format(lam, tag), eg, e64['g', lam])
    if case[0] == 'exact':                      # g is rounding noise: 32 x 2^-53 of its rounding scale per factor that touches the pose
        fg = ldp.system_floors(ref_fac)[1]
        count = np.bincount(np.concatenate([lp.pose_rid[ref_fac.j], lp.pose_rid[ref_fac.i[ref_fac.i >= 0]]]), minlength=nr)
        worst = float((np.abs(g).reshape(nr, d).max(axis=1) / (fg * count)).max())
        print('{:13s} se{} {:34s} device {:.2e}   bound {:.2e} (absolute, over the scale)'.format(case[0], d // 3 + 1, '|g|', worst, 32 * EPS))
        assert worst <= 32 * EPS, (case, worst)
    # blocks the pattern holds but nothing touches are exactly zero
    quiet = ~np.repeat(np.repeat(touched, d, axis=0), d, axis=1)
    assert np.all(S[quiet] == 0.)
    if lp.num_obs:
        # the landmark elimination's diagonal blocks are not the same sum transposed (tests/test_gpu_parity.py promises 1e-13 |S|):
        # no bit-for-bit promise there, so symmetry is held to 2^-52 |S|, |S| the largest entry; the block only a factor writes is
        # k_factor_assemble's alone -- the same sum transposed -- and is symmetric bit for bit
        asym = np.abs(S - S.T).max() / np.abs(S).max()
        print('{:13s} se3 {:34s} device {:.2e}   bound {:.2e}'.format(case[0], 'asymmetry of S lambda={} {}'.format(lam, tag), asym, 2. ** -52))
        assert asym <= 2. ** -52, (case, lam, asym)
        a, b = lp.pose_rid[info['factor_only'][0]], lp.pose_rid[info['factor_only'][1]]
        assert np.array_equal(S[d * a:d * a + d, d * b:d * b + d], S[d * b:d * b + d, d * a:d * a + d].T), (case, 'factor-only block', lam)
        fS, _ = ldp.system_floors(ref_fac)
        cut = lambda A: ldp.cut_blocks(A, d).reshape(nr, nr, d * d)                     # noqa: E731
        rid = lp.pose_rid
        for what in ('factor_only', 'shared'):
            a, b = rid[info[what][0]], rid[info[what][1]]
            err = ldp.row_err(cut(S)[[a, b], [b, a]], cut(Sr)[[a, b], [b, a]], fS.reshape(nr, nr)[[a, b], [b, a]])
            limit = sc.bound(e64['S', lam])
            assert err <= limit, (case, 'the {} block {} of S, lambda={}'.format(what.replace('_', '-'), info[what], lam), err, limit)
    else:
        # the two halves of S are the same sums transposed (k_factor_assemble walks one item list per slot in factor order; the
        # products of k_factor_pass commute): symmetric bit for bit
        assert np.array_equal(S, S.T), np.abs(S - S.T).max()
    return S, g


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_reduced_system(case):
    lp, _ = sc.scene(*case)
    dev = device(lp)
    out = [reduced(case, dev, lam) for lam in sc.LAMBDAS]
    zero_list = dev.get_option('lin_zero_list')
    dev.close()
    if case[0] == 'mixed_ba':                   # the list zeroing against the fill: the same bits, each within bound of the reference
        assert zero_list == 1
        off = device(lp)
        off.set_option('lin_zero_list', 0)
        assert off.get_option('lin_zero_list') == 0
        for lam, (S, g) in zip(sc.LAMBDAS, out):
            S0, g0 = reduced(case, off, lam, 'lin_zero_list=0')
            assert np.array_equal(S0, S) and np.array_equal(g0, g), lam
        off.close()


# ---------------------------------------------------------------------------
# 3. costs
# ---------------------------------------------------------------------------
def reference_costs(case):
    lp, _ = sc.scene(*case)
    want = sc.factor_pairs(*case)[0][0].costs()
    if lp.num_obs:
        import longdouble_schur as lds
        ba = lds.costs(lp, np.longdouble)
        want = (want[0] + ba[0], want[1] + ba[1])
    return want


def costs(case, dev=None):
    """eval_cost(True) and eval_cost(False) against the long-double sums: k_cost_factors and its skip rule (a factor is left out of
    the second only when NO end is variable).  The absolute term is what 2^-52 u of error in every residual component leaves of a cost
    that is all cancellation (`exact`)."""
    lp, _ = sc.scene(*case)
    own = dev is None
    dev = dev or device(lp)
    u = ldp.factor_scale(lp)
    slack = lp.dof * float(((2 * EPS * u) ** 2).sum())
    got = (dev.eval_cost(True), dev.eval_cost(False))
    if own:
        dev.close()
    e64 = sc.e64(*case)['cost']
    limit = sc.bound(e64, TOL_COST) if case[0] == 'near_pi' else TOL_COST           # (near_pi is judged by the e64 rule alone)
    for flag, c, want in zip((True, False), got, reference_costs(case)):
        err = abs(c - want) / max(abs(want), 1e-300)
        report(case, 'eval_cost({})'.format(flag), err, e64, limit)
        assert abs(c - want) <= limit * abs(want) + slack, (case, flag, c, want)
    return got


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_costs(case):
    got = costs(case)
    if case[0] == 'const_pair':                 # the constant-constant edges are in the first sum only
        assert got[0] > got[1] > 0.
    if case[0] == 'exact':
        assert 0. <= got[0] <= 1e-26


# ---------------------------------------------------------------------------
# 4. one step, and the retraction on its own
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def arbiter(case):
    """(accurate_solve of the long-double system rounded to fp64, e_ref: the distance of a sparse LU step on the fp64 twin's system
    from it, whether the reference system is definite)."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    (Sr, gr, _), (St, gt, _) = sc.system_pairs(case[0], case[1], 0.)[0]
    S, g = Sr.astype(np.float64), gr.astype(np.float64)
    dg = np.diag(S)
    if dg.min() <= 0. or np.linalg.eigvalsh(S / np.sqrt(dg[:, None] * dg[None, :])).min() <= 1e-10:           # (Jacobi-scaled)
        return None, None, False
    exact = accurate_solve(S, g)
    lu = spla.spsolve(sp.csc_matrix(St), gt)
    return exact, float(np.abs(lu - exact).max() / np.abs(exact).max()), True


def check_retraction(case, lp, dev, dx, step, what, want_small=None):
    poses, _ = dev.get_params()
    ref, small = ldp.retract(lp, dx, step, LD)
    if want_small is not None:
        assert np.all(small == want_small), (case, what, 'branch of exp')
    err = ldp.row_err(poses, ref, sc.pose_floor(lp))
    worst = 0.                                  # e64: the start that was used and DRAWS copies of it one ulp away
    for q in [lp] + [ldp.one_ulp_away(lp, k) for k in range(sc.DRAWS)]:
        worst = max(worst, ldp.row_err(ldp.retract(q, dx, step, np.float64)[0], ldp.retract(q, dx, step, LD)[0], sc.pose_floor(q)))
    check(case, what, err, worst)
    const = lp.pose_rid < 0
    assert np.array_equal(poses[const], lp.poses[const])                       # constant poses: the same bits
    return poses


def step(case):
    lp, _ = sc.scene(*case)
    exact, e_ref, definite = arbiter(case)
    assert definite == (case[0] not in INDEFINITE), case
    if not definite:
        pytest.skip('{}: the reduced system is not definite'.format(case[0]))
    d = lp.dof
    # (a) one Gauss-Newton iteration without line search
    dev = device(lp)
    cost, nrm, its, rel = dev.gn_iteration(0., 0., PCG_MAX_ITERS, False)
    xp, xl = dev.get_dx()
    assert np.all(np.isfinite(xp))
    print('{:13s} reduced solve: {} unknowns, {} iterations, residual {:.2e}'.format(case[0], exact.size, its, rel))
    if case[0] == 'exact':
        # g is rounding noise here and so is the step: no digit to compare.  It is bounded absolutely instead, by what 2^-52 of g's
        # rounding scale (longdouble_posegraph.system_floors) becomes behind the reference's S^-1
        (Sr, _, _), _ = sc.system_pairs(case[0], case[1], 0.)[0]
        limit = 8 * np.abs(np.linalg.inv(Sr.astype(np.float64))).sum(axis=1).max() * 2 * EPS * ldp.system_floors(sc.factor_pairs(*case)[0][0])[1].max()
        print('{:13s} se{} {:34s} device {:.2e}   bound {:.2e} (absolute)'.format(case[0], d // 3 + 1, '|dx|', np.abs(xp).max(), limit))
        assert np.abs(xp).max() <= limit and np.abs(exact).max() <= limit, (case, np.abs(xp).max(), limit)
    else:
        err = float(np.abs(xp.ravel() - exact).max() / np.abs(exact).max())
        limit = sc.bound(e_ref, TOL_DX)
        report(case, 'dx against the arbiter', err, e_ref, limit)
        assert err <= limit, (case, err, e_ref)
    if case[0] == 'cg_size':
        assert its > 0                                                        # past k_direct_solve: the folded CG ran
    check_retraction(case, lp, dev, xp, 1., 'poses after the step')
    dev.close()
    # (b), (c) the same step scaled through apply_update so that the largest |phi step| is 2.5 (the sin / cos branch of exp at a
    # large angle) and 0.5e-8 (every pose in the branch below 1e-8)
    for target, what, small in ((2.5, 'poses after a step scaled to 2.5 rad', None), (0.5e-8, 'poses after a step below 1e-8', True)):
        dev = device(lp)
        dev.linearize(0.)
        dev.solve_reduced(0., PCG_MAX_ITERS)
        dev.backsub()
        xp, _ = dev.get_dx()
        scale = target / np.sqrt((xp[:, d // 3 + 1:] ** 2).sum(axis=1)).max()
        dev.apply_update(scale)
        check_retraction(case, lp, dev, xp, scale, what, want_small=small)
        dev.close()
    # (d) under L2 alone (the system stays definite wherever it is linearised): a handle whose parameters were moved by 2.5 rad
    # first, so that the Gauss-Newton step itself is large
    if np.all(lp.edge_groups[:, 1] == ldp.L2):
        rng = np.random.default_rng(77)
        var = np.flatnonzero(lp.pose_rid >= 0)
        far = lp.copy()
        far.poses = ldp.retract(lp, np.stack([sc._tangent(rng, d, 2.5, 1.) for _ in var]), 1., LD)[0].astype(np.float64)
        dev = device(lp)
        dev.set_params(far.poses, None)
        dev.gn_iteration(0., 0., PCG_MAX_ITERS, False)
        xp, _ = dev.get_dx()
        assert np.all(np.isfinite(xp))
        phi = np.sqrt((xp[:, d // 3 + 1:] ** 2).sum(axis=1)).max()
        print('{:13s} step from a start 2.5 rad away: largest |phi| {:.2f}'.format(case[0], phi))
        assert phi > 1., phi
        check_retraction(case, far, dev, xp, 1., 'poses after a large step')
        dev.close()


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_step_and_retraction(case):
    step(case)


# ---------------------------------------------------------------------------
# 5. and 6. the same bits from two handles; the tap leaves the solver state alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=_id)
def test_two_handles_and_the_tap(case):
    lp, _ = sc.scene(*case)
    a, b = device(lp), device(lp)
    tap_a = a.debug_factor_blocks()                     # a: tap, then linearise;  b: linearise without a tap before it
    out = []
    for dev in (a, b):
        dev.linearize(1e-3)
        out.append(list(dev.reduced_system()) + [np.float64(dev.eval_cost(True)), np.float64(dev.eval_cost(False))])
    tap_b = b.debug_factor_blocks()
    b.linearize(1e-3)                                   # ... and once more after it
    again = list(b.reduced_system())
    a.close()
    b.close()
    for k, (x, y) in enumerate(zip(tap_a, tap_b)):
        assert np.array_equal(x, y), ('tap', k)
    for k, (x, y) in enumerate(zip(out[0], out[1])):
        assert np.array_equal(x, y), ('two handles, tap before one linearisation', k)
    for k, (x, y) in enumerate(zip(again, out[1])):
        assert np.array_equal(x, y), ('linearisation after the tap', k)


def margins(case):
    """Every figure of one scene, printed: tests/parity_margins.py."""
    lp, _ = sc.scene(*case)
    blocks(case)
    dev = device(lp)
    for lam in sc.LAMBDAS:
        reduced(case, dev, lam)
    costs(case, dev)
    dev.close()
    if case[0] not in INDEFINITE:
        step(case)
