"""Host checks of the pose-factor scenes and of their long-double reference (tests/posegraph_scenes.py, tests/longdouble_posegraph.py):
the scenes are what they say (counts, branch membership by the fp64 predicate, both sides of every k), the fp64 twin of the new
definition agrees with the oracle (oracle/gn_oracle.py: eval_edges, eval_priors, eval_cost, normal_equations) to 1e-13 per row -- which
ties the definition to the oracle without using the oracle as the reference -- log(exp(xi)) = xi in long double, and e64 of every scene
and quantity over nine draws, printed (`pytest -s`); tests/test_gpu_posegraph.py takes its bounds from the same function.

e64 observed here, in the measure of tests/test_gpu_posegraph.py: the WHOLE-SCENE figure, the largest over all rows of r~, J~, S, g, both
dampings and nine draws (the table of the device test quotes, per quantity, the class or variant with the least margin: its e64 can be
smaller).  Every scene but near_pi sits below the 1e-12 floor by the reference alone -- angles 3.3e-14, km 3.0e-15, mm 1.1e-13, rot_only
6.3e-14 (SE(2) 4.6e-16), tails / structure / exact / cg_size <= 9.1e-15 -- except
  mixed_wg           SE(3): S 1.4e-12, J~_2 6.8e-13; SE(2): S 2.1e-13, J~ 1.0e-13 -- its L1 rows alone (every other loss: <= 2e-15): the
                     weight 1 / |r_k| hands the RELATIVE error of a residual component, 2^-53 u / |r_k|, to the whole row of J~ (a
                     component of 1e-3 among N(0, 0.3^2) ones: 1e-13), the row's own largest entry grows with it, and one evaluation's
                     worst row says little about another's (tests/test_gpu_offbox.py found the same under L1);
  mixed_ba           g 1.3e-12, S 4.3e-13: the landmark elimination's own error (tests/test_gpu_offbox.py: `base`), not the factors';
  near_pi            r~ 8.1e-9, g 2.6e-9 (its prior class alone: r~ 6.0e-9): 2^-53 / (pi - theta)^2 at 3.1415."""
import numpy as np
import pytest

import longdouble_posegraph as ldp
import posegraph_scenes as sc
from oracle import gn_oracle as orc

pytestmark = pytest.mark.skipif(not ldp.LONGDOUBLE_OK, reason=ldp.LONGDOUBLE_SKIP)

LD = sc.LD
TIE = 1e-13
CASES = sc.cases()


def _ids(c):
    return '{}-se{}'.format(c[0], 3 if c[1] == 6 else 2)


# ---------------------------------------------------------------------------
# the scenes are what they say
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('dof', [6, 3])
@pytest.mark.parametrize('name', ['angles', 'km', 'mm'])
def test_angle_scenes_hold_the_wanted_rotations_and_branches(name, dof):
    lp, info = sc.scene(name, dof)
    want = np.abs(info['angle'])
    n = len(sc.ANGLES) if dof == 6 else 2 * len(sc.ANGLES) - 1 + len(sc.SE2_EXTRA)
    assert lp.num_edges == n and lp.num_priors == n and lp.num_reduced == 2 * n
    got = sc.error_rotation(lp)
    # (poses are rounded to fp64 after the product: 2^-53 of a rotation entry -- which moves an angle beyond 2 rad by that over
    # sin(theta), and what acos makes of it by as much again)
    slack = np.where(want <= 2., 4e-16 * np.maximum(1., want) + 1e-16, 1e-15 / (np.pi - np.minimum(want, 3.14)) ** 2)
    assert np.all(np.abs(got - want) <= slack), (np.abs(got - want) / slack).max()
    small_angle, small_phi = ldp.in_branch(lp)
    print(name, dof, 'angle / vee(R - I) branch / I - phi^/2 branch')
    for a, s1, s2 in zip(info['angle'], small_angle, small_phi):
        print('   {:9.2e} {:d} {:d}'.format(a, s1, s2))
    clear_small, clear_large = want <= 5e-9, want >= 3e-8
    assert np.all(small_phi[clear_small]) and not np.any(small_phi[clear_large])
    if dof == 6:
        assert np.all(small_angle[clear_small]) and not np.any(small_angle[clear_large])
        # between 1e-8 and ~1.5e-8 the fp64 acos returns 0: such a factor sits in vee(R - I) although its angle is above 1e-8
        # and which side of it is decided by the rounding of the poses' entries.  Both sides occur in every scene: the band is tested
        band = (want > 1e-8) & (want < 3e-8)
        assert band.sum() == 4
        assert np.all(small_angle[want == 0.9e-8])
        assert (small_angle & band).sum() >= 1 and (~small_angle & band).sum() >= 1, (small_angle[band], want[band])
        # (with |phi| = 0 from acos the factor's phi is vee(R - I), above 1e-8: the inverse left Jacobian takes its series branch)
        assert not np.any(small_phi[band])
    # the translations have the scale the scene says
    tscale = dict(angles=1., km=1e3, mm=1e-3)[name]
    tmax = np.abs(lp.poses[:, (9 if dof == 6 else 4):]).max()
    assert 0.5 * tscale < tmax < 20. * tscale


def test_near_pi():
    lp, info = sc.scene('near_pi', 6)
    assert np.allclose(sc.error_rotation(lp), info['angle'], rtol=0, atol=1e-7) and np.pi - info['angle'].max() > 9e-5


@pytest.mark.parametrize('dof', [6, 3])
def test_rot_only(dof):
    lp, info = sc.scene('rot_only', dof)
    m = dof // 3 + 1
    fac = ldp.Factors(lp, LD)
    E = lp.num_edges
    assert E == (len(sc.ANGLES) if dof == 6 else 2 * len(sc.ANGLES) - 1 + len(sc.SE2_EXTRA)) and lp.num_priors == 2 * E
    assert not fac.present[:E, :m].any() and fac.present[:E, m:].all() and fac.present[E:].all()
    assert np.all(fac.s[:E, :m] == 0) and np.all(fac.rt[:E, :m] == 0) and np.all(fac.J2[:E, :m] == 0) and np.all(fac.J1[:E, :m] == 0)
    assert np.all(lp.e_Tobs_inv[:, m * m:] == 0.)
    assert np.abs(fac.xi[E:, :m]).max() <= 2e-6                       # priors: |t_E| <= 1e-6, phi is the row
    assert set(fac.loss[:E]) == {ldp.L2, ldp.HUBER, ldp.CAUCHY, ldp.L1}
    assert np.all(np.isfinite(fac.rt.astype(float))) and np.all(np.isfinite(fac.J1.astype(float)))
    # the oracle evaluates L1's weight on the absent rows: NaN there (what the kernel's rule avoids)
    ro = orc.eval_edges(lp, jac=False)
    assert np.isnan(orc._by_group(lp.edge_groups, lp.e_grp, 1, 2, orc.loss_weight, ro)[fac.loss[:E] == ldp.L1][:, :m]).all()


@pytest.mark.parametrize('dof', [6, 3])
def test_mixed_wg_mixes_kinds_groups_and_both_sides_of_every_k(dof):
    lp, _ = sc.scene('mixed_wg', dof)
    fac = ldp.Factors(lp, LD)
    assert fac.F == 129 and lp.num_edges == 40
    assert lp.edge_groups.shape[0] == sc.HIGH_GROUP_ROWS
    ids = sorted(set(fac.grp))
    assert ids == [0, 1, 2, 3, 4, 5, sc.HIGH_GROUP_ROWS - 1]
    # workgroup 0 (factors 0 .. 63) and its third wave (32 .. 47) hold edges and priors; every run of 7 factors holds 7 groups
    assert (fac.i[32:48] >= 0).any() and (fac.i[32:48] < 0).any()
    assert all(len(set(fac.grp[k:k + 7])) == 7 for k in range(fac.F - 6))
    for g in ids:
        lid, k = int(lp.edge_groups[g, 1]), lp.edge_groups[g, 2]
        a = np.abs(fac.r[fac.grp == g]).astype(float)
        if lid in (ldp.CAUCHY, ldp.HUBER, ldp.TUKEY):
            assert (a < k).sum() >= 5 and (a > k).sum() >= 5, (g, lid)
        if lid == ldp.L1:
            assert a.min() > 1e-6
    S = lp.stiffd[lp.edge_groups[ids, 0].astype(int)].reshape(-1, dof, dof)
    assert np.all(np.abs(S - np.identity(dof)).max(axis=(1, 2)) < 1.5) and np.all(S != 0.)        # full matrices near the identity


@pytest.mark.parametrize('dof', [6, 3])
def test_tails_and_structure_shapes(dof):
    for nf in sc.TAILS:
        lp, _ = sc.scene('tails{}'.format(nf), dof)
        assert lp.num_edges == nf and lp.num_priors == 0 and lp.pose_rid[0] == -1
        if nf >= 17:
            assert (lp.e_i > lp.e_j).sum() >= nf // 3 - 1 and len(set(lp.e_grp[:16])) == 2
    lp, _ = sc.scene('dup', dof)
    pairs = list(zip(lp.e_i.tolist(), lp.e_j.tolist()))
    assert pairs.count((1, 2)) == 3 and pairs.count((2, 1)) == 1
    lp, _ = sc.scene('const_middle', dof)
    assert lp.pose_rid[2] == -1 and lp.num_reduced == 4
    lp, _ = sc.scene('const_pair', dof)
    fac = ldp.Factors(lp, LD)
    assert list(np.flatnonzero(~fac.active())) == [0, 1]            # the two edges between the constant poses 0 and 3
    all_, act = fac.costs()
    assert all_ > act > 0 and all_ - act == pytest.approx(float(fac.rho[:2].sum()), rel=1e-12)
    # ... and in no block: the assembly is the same with their residuals taken away (a copy whose two measurements are replaced)
    moved = lp.copy()
    moved.e_Tobs_inv[:2] = moved.e_Tobs_inv[2:4]
    for a, b in zip(fac.assemble(1e-3)[:2], ldp.Factors(moved, LD).assemble(1e-3)[:2]):
        assert np.array_equal(a, b)
    lp, _ = sc.scene('star70', dof)
    assert np.bincount(np.concatenate([lp.e_i, lp.e_j]))[0] == 70
    lp, _ = sc.scene('prior_every', dof)
    assert sorted(lp.u_i.tolist()) == list(range(lp.num_poses))
    lp, _ = sc.scene('priors_only', dof)
    assert lp.num_edges == 0 and lp.num_priors == 6


def test_mixed_ba_and_cg_size_shapes():
    lp, info = sc.scene('mixed_ba', 6)
    a, b = info['factor_only']
    seen = lambda p: set(lp.obs_point[lp.obs_pose == p].tolist())                  # noqa: E731
    assert not (seen(a) & seen(b)) and (seen(info['shared'][0]) & seen(info['shared'][1]))
    assert lp.pose_rid[a] >= 0 and lp.pose_rid[b] >= 0 and lp.pose_rid[info['prior']] >= 0
    assert (lp.e_i > lp.e_j).sum() == 1 and lp.pose_rid[0] == -1 and 0 in lp.e_i
    lp, _ = sc.scene('cg_size', 6)
    assert lp.dof * lp.num_reduced == 120


@pytest.mark.parametrize('dof', [6, 3])
def test_exact_scene_is_zero_to_rounding(dof):
    """r~ and g zero to 4e-16 u, every block finite, the cost 0 (u: the rounding scale; observed 1.2e-16 u .. 1.6e-16 u in both dtypes:
    the tables themselves are rounded to 2^-53 of their entries, three of them meet in a factor, so 1e-16 of the scale is not
    reachable by any evaluation of these inputs) -- under L2, Huber, Cauchy and Tukey (not L1: its weight at a
    zero residual is NaN by definition)."""
    lp, _ = sc.scene('exact', dof)
    fac = ldp.Factors(lp, LD)
    u = ldp.factor_scale(lp)
    assert set(fac.loss) == {ldp.L2, ldp.HUBER, ldp.CAUCHY, ldp.TUKEY}
    assert np.all(np.abs(fac.rt).max(axis=1) <= 4e-16 * u)
    S, g, _ = fac.assemble(0.)
    assert np.all(np.isfinite(S.astype(float))) and np.abs(g).max() <= 4e-16 * (u * np.abs(fac.J2).reshape(fac.F, -1).max(axis=1)).max() * 4
    assert fac.costs()[0] <= 1e-28


# ---------------------------------------------------------------------------
# the fp64 twin against the oracle
# ---------------------------------------------------------------------------
def _oracle_blocks(lp):
    d = lp.dof
    rs, j1s, j2s = [], [], []
    if lp.num_edges:
        r, j1, j2 = orc.eval_edges(lp)
        with np.errstate(invalid='ignore'):
            s = np.sqrt(orc._by_group(lp.edge_groups, lp.e_grp, 1, 2, orc.loss_weight, r))
        rs.append(s * r), j1s.append(s[:, :, None] * j1), j2s.append(s[:, :, None] * j2)
    if lp.num_priors:
        r, j2 = orc.eval_priors(lp)
        with np.errstate(invalid='ignore'):
            s = np.sqrt(orc._by_group(lp.edge_groups, lp.u_grp, 1, 2, orc.loss_weight, r))
        rs.append(s * r), j1s.append(np.zeros((len(r), d, d))), j2s.append(s[:, :, None] * j2)
    return np.concatenate(rs), np.concatenate(j1s), np.concatenate(j2s)


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_fp64_twin_agrees_with_the_oracle(case):
    """1e-13 per row in the measure of the device tests (the near-pi rows: 8 e64; the `exact` scene is all cancellation and is held
    absolutely by the measure's floor).  Rows where the oracle itself has NaN -- L1's weight on an absent stiffness row, rot_only --
    are compared where it is finite; rot_only's normal equations are NaN in the oracle for the same reason and are not compared."""
    name, dof = case
    lp, _ = sc.scene(name, dof)
    twin = ldp.Factors(lp, np.float64)
    e = sc.e64(name, dof)
    tol = lambda what: max(TIE, 8 * e[what]) if name == 'near_pi' else TIE                   # noqa: E731
    u = ldp.factor_scale(lp)
    for what, ref in zip(('rt', 'J1', 'J2'), _oracle_blocks(lp)):
        got = getattr(twin, what)
        ok = np.isfinite(ref)
        assert name == 'rot_only' or ok.all()
        assert np.all(got[~ok] == 0.)
        err = ldp.row_err(np.where(ok, got, 0.), np.where(ok, ref, 0.), u)
        assert err <= tol(what if what == 'rt' else 'J1'), (what, err)
    want = (orc.eval_cost(lp, True), orc.eval_cost(lp, False))
    if lp.num_obs:
        import longdouble_schur as lds
        ba = lds.costs(lp)
        want = (want[0] - ba[0], want[1] - ba[1])
    scale = max(abs(want[0]), 1e-300)
    assert all(abs(a - b) <= (1e-28 if name == 'exact' else tol('cost') * scale) for a, b in zip(twin.costs(), want))
    if name == 'rot_only':
        return
    q = lp
    if lp.num_obs:                                   # the factor part alone: the problem without its observations
        q = lp.copy()
        q.obs_pose, q.obs_point, q.obs_grp, q.obs_uvd = q.obs_pose[:0], q.obs_point[:0], q.obs_grp[:0], q.obs_uvd[:0]
        q = q.finalize()
    n = dof * lp.num_reduced
    for lam in sc.LAMBDAS:
        P, b, _ = orc.normal_equations(q, points_first=False, lm_lambda=lam)
        eS, eg = sc.err_system(twin.assemble(lam), (P.toarray()[:n, :n], b[:n]), twin)
        assert eS <= tol(('S', lam)) and eg <= tol(('g', lam)), (lam, eS, eg)


# ---------------------------------------------------------------------------
# log(exp(xi)) = xi in long double
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('dof', [6, 3])
def test_log_of_exp_in_long_double(dof):
    """1e-17 max(1, |xi|) over the angles table -- plus, where the DEFINITION itself is not an identity in exact arithmetic: the
    truncated series of its small branches (a row that any 1e-8 branch handles: theta^2 / 2 max(1, |rho|); observed, absolute: 2.1e-17
    at 0.9e-8 against 6.5e-17, 5.4e-17 at 1.6e-8 through vee(R - I) against 1.5e-16 -- a term of fp64's own size: an fp64 value
    leaking into these few rows would not be seen by this test, the dtype assertions are what excludes it) and, in SE(3) beyond 3 rad,
    the cancellation of acos / sin in long double, 8 x 2^-64 / (pi - theta)^2 (3.1: observed 1.6e-16 against 2.8e-16).  Between
    these the reference returns xi to 2e-19."""
    rng = np.random.default_rng(7)
    angles = list(sc.ANGLES) + ([] if dof == 6 else [-a for a in sc.ANGLES] + list(sc.SE2_EXTRA))
    xi = np.stack([sc._tangent(rng, dof, a, 1.) for a in angles])
    T = sc._exp(xi)
    pred = ldp.Predicates()
    ldp.log(ldp.unpack(ldp.pack(T).astype(float), dof, np.float64), pred, 'x')
    pred.recording = False
    back = ldp.log(T, pred, 'x')
    assert back.dtype == LD
    theta = np.abs(np.array(angles))
    touched_small = np.any([v for v in pred.table.values()], axis=0) | (theta <= ldp.SMALL)
    tol = 1e-17 * np.maximum(1., np.linalg.norm(xi, axis=1))
    tol = tol + np.where(touched_small, 0.5 * theta ** 2 * np.maximum(1., np.abs(xi[:, :dof // 3 + 1]).max(axis=1)), 0.)
    if dof == 6:                                # (SE(2)'s atan2 has no such cancellation)
        tol = tol + np.where(theta > 3., 8 * 2. ** -64 / (np.pi - theta) ** 2, 0.)
    err = np.abs(back - xi.astype(LD)).max(axis=1).astype(float)
    for a, e, t in zip(angles, err, tol):
        print('se{} angle {:10.3e}  |log(exp(xi)) - xi| {:.1e}  bound {:.1e}'.format(dof // 3 + 1, a, e, t))
    assert np.all(err <= tol), (err / tol).max()


# ---------------------------------------------------------------------------
# e64 of every scene and quantity
# ---------------------------------------------------------------------------
FLOOR_EXCEPTIONS = {('near_pi', 6), ('mixed_wg', 6), ('mixed_wg', 3), ('mixed_ba', 6)}           # (the module docstring says why)


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_e64_over_nine_draws(case):
    name, dof = case
    e = sc.e64(name, dof)
    print('{:13s} se{}  '.format(name, dof // 3 + 1) + '  '.join(
        '{}={:.1e}'.format(k if isinstance(k, str) else '{}@{}'.format(*k), v) for k, v in e.items()))
    assert all(np.isfinite(v) for v in e.values())
    worst = max(v for k, v in e.items() if k != 'cost')
    if case not in FLOOR_EXCEPTIONS:
        assert worst <= 1e-12 / sc.FACTOR, worst                    # the bound of the device tests is the 1e-12 floor itself
    if name != 'exact':
        assert e['cost'] <= 1e-10 / sc.FACTOR or name == 'near_pi'
