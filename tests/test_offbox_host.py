"""The off-box scenes (tests/offbox_scenes.py) and the long-double landmark elimination (tests/longdouble_schur.py) on the host: the
reference's fp64 twin against the oracle's dense Schur complement, the rounding error of an fp64 elimination per depth against the
figures the scenes were written to reproduce, and that the scenes hold what they say (depths, disparities, groups per wave, camera
types per landmark).  Counterpart of reference pyslam/problem.py:332-333 + :186."""
import numpy as np
import pytest

import longdouble_schur as ld
import offbox_scenes as sc
from oracle import gn_oracle as orc
from test_gpu_parity import oracle_reduced

needs_longdouble = pytest.mark.skipif(not ld.LONGDOUBLE_OK, reason=ld.LONGDOUBLE_SKIP)


@pytest.mark.parametrize('lam', [0., 1e-3])
def test_fp64_twin_equals_the_oracles_dense_schur_complement(lam):
    """On stereo_ba itself (the scenes' base, TABLE_SHAPE, with its constants): S, g to 1e-13 of their largest entry, the landmark
    part of the dense solve's step from its pose part, and the two costs."""
    lp, _ = sc._base(sc.TABLE_SHAPE)
    twin = ld.Elimination(lp, lam, np.float64)
    n = 6 * lp.num_reduced
    if lam == 0.:
        So, go, _ = oracle_reduced(lp)
    else:
        P, b, _ = orc.normal_equations(lp, False, lam)
        P = P.toarray()
        Hinv = np.linalg.inv(P[n:, n:])
        So, go = P[:n, :n] - P[:n, n:] @ Hinv @ P[n:, :n], b[:n] - P[:n, n:] @ Hinv @ b[n:]
    e_S, e_g = ld.max_err(twin.S, So), ld.max_err(twin.g, go)
    print('lambda {}: twin against oracle_reduced S {:.1e} g {:.1e}'.format(lam, e_S, e_g))
    assert e_S <= 1e-13 and e_g <= 1e-13
    assert np.abs(twin.S - twin.S.T).max() <= 1e-13 * np.abs(twin.S).max()
    # the factors as the device keeps them: C^-1 = M^T M, c = M b_l
    assert ld.max_err(np.einsum('vki,vkj->vij', twin.M, twin.M), twin.Cinv) <= 1e-10        # (cond(C) 3e4 here)
    P, b, cost = orc.normal_equations(lp, False, lam)
    Pt, bt = twin.normal_equations()
    assert ld.max_err(Pt, P.toarray()) <= 1e-14 and ld.max_err(bt, b) <= 1e-13
    dx = np.linalg.solve(P.toarray(), b)
    assert ld.max_err(twin.backsub(dx[:n].reshape(-1, 6)).reshape(-1), dx[n:]) <= 1e-9
    assert ld.costs(lp) == pytest.approx((orc.eval_cost(lp, True), cost), rel=1e-14)


def test_diagonal_only_is_the_diagonal_of_the_whole():
    lp, _ = sc.scene('mixed_wave', sc.TABLE_SHAPE)
    full, diag = ld.Elimination(lp, 1e-3, np.float64), ld.Elimination(lp, 1e-3, np.float64, diagonal_only=True)
    nr = lp.num_reduced
    assert np.array_equal(full.S.reshape(nr, 6, nr, 6)[np.arange(nr), :, np.arange(nr), :], diag.Sdiag)
    assert np.array_equal(full.g, diag.g)


@needs_longdouble
@pytest.mark.parametrize('name', sorted(sc.EXPECTED_E64))
def test_fp64_elimination_error_per_depth_is_the_tabulated_one(name):
    """The distance of the fp64 elimination from the long-double one on TABLE_SHAPE, largest difference over largest entry: within
    a factor 3 of offbox_scenes.EXPECTED_E64 -- cond(C) and with it the error grow as depth^2."""
    lp, _ = sc.scene(name, sc.TABLE_SHAPE)
    blocks = ld.scaled_blocks(lp)
    ref, twin = ld.Elimination(lp, 0., np.longdouble, blocks), ld.Elimination(lp, 0., np.float64, blocks)
    e_S, e_g = ld.max_err(twin.S, ref.S), ld.max_err(twin.g, ref.g)
    want_S, want_g = sc.EXPECTED_E64[name]
    print('{}: cond(C) {:.1e}  e64 S {:.1e} (tabulated {:.1e})  g {:.1e} ({:.1e})'.format(
        name, np.linalg.cond(ref.C.astype(np.float64)).max(), e_S, want_S, e_g, want_g))
    assert want_S / 3 <= e_S <= 3 * want_S
    assert want_g / 3 <= e_g <= 3 * want_g


@pytest.mark.parametrize('shape', [sc.TABLE_SHAPE, sc.GPU_SHAPE], ids=['table_shape', 'gpu_shape'])
@pytest.mark.parametrize('name', sc.DEPTH_SCENES)
def test_depths_and_disparities(name, shape):
    lp, truth = sc.scene(name, shape)
    (z0, z1), (d0, d1) = sc.depth_and_disparity(lp, truth)
    print('{}: z {:.2f} .. {:.2f} m, disparity {:.2f} .. {:.2f} px'.format(name, z0, z1, d0, d1))
    zr, dr = sc.Z_RANGE[name], sc.DISPARITY_RANGE[name]
    assert zr[0] <= z0 < 1.3 * zr[0] and 0.9 * zr[1] < z1 <= zr[1]
    assert dr[0] <= d0 and d1 <= dr[1]
    if name in ('far10', 'far100'):
        assert d0 < 0.                                  # disparities the noise has made negative: farther than infinity
    assert lp.pose_rid[0] < 0 and 0 < np.count_nonzero(lp.point_vid < 0) < lp.num_points // 5
    assert lp.num_poses <= 9 and lp.num_points <= 600


@pytest.mark.parametrize('shape', [sc.TABLE_SHAPE, sc.GPU_SHAPE], ids=['table_shape', 'gpu_shape'])
def test_units_and_mixed_depth(shape):
    base, _ = sc._base(shape)
    mm, _ = sc.scene('mm', shape)
    assert np.array_equal(mm.obs_uvd, base.obs_uvd) and mm.cams[0, 4] == 1000. * base.cams[0, 4]
    assert np.array_equal(mm.points, 1000. * base.points) and np.array_equal(mm.poses[:, :9], base.poses[:, :9])
    assert np.array_equal(mm.poses[:, 9:], 1000. * base.poses[:, 9:])
    lp, truth = sc.scene('mixed_depth', shape)
    factor = sc._mixed_depth_factors(shape)
    assert set(np.unique(factor)) == {0.08, 1., 10., 100.}
    # every wave of the landmark pass (ten or more whole landmarks of at most six rows) mixes magnitudes: any ten consecutive variable
    # landmarks hold at least two factors, any sixty-four rows at least three
    f = factor[np.argsort(np.where(lp.point_vid >= 0, lp.point_vid, lp.num_points), kind='stable')[:lp.num_var_points]]
    assert sc.min_distinct_per_run(f, 10) >= 2
    assert sc.min_distinct_per_run(factor[lp.obs_point][sc.observation_orders(lp)[0]], 64) >= 3
    C = ld.Elimination(lp, 0., np.float64).C
    assert np.abs(C).max(axis=(1, 2)).max() / np.abs(C).max(axis=(1, 2)).min() > 1e5


@pytest.mark.parametrize('shape', [sc.TABLE_SHAPE, sc.GPU_SHAPE], ids=['table_shape', 'gpu_shape'])
@pytest.mark.parametrize('name', sc.MIXED_SCENES)
def test_mixed_scenes_mix_every_wave(name, shape):
    lp, _ = sc.scene(name, shape)
    cams = lp.cams[:, 4]
    assert cams[0] > 0. and cams[1] == -1. and cams[2] == -2.
    mono = ld.mono_rows(lp)
    S = lp.stiff3[lp.obs_groups[lp.obs_grp, 1].astype(int)].reshape(-1, 3, 3)
    assert not S[mono][:, 2, :].any() and not S[mono][:, :, 2].any() and not lp.obs_uvd[mono, 2].any()
    assert np.any(S[:, 0, 1] != 0.) and np.any(S[:, 0, 1] == 0.)                        # a non-diagonal and a diagonal stiffness
    used = lp.obs_groups[np.unique(lp.obs_grp)]
    assert len({(g[0], g[2], g[3]) for g in used}) >= 6 and len({g[2] for g in used}) >= 2
    assert any(g[0] == 2. and g[2] == 1. for g in used)                                 # L1 on a monocular group
    assert sc.min_classes_per_wave(lp) >= 3
    all_three = sc.landmarks_with_all_cameras(lp)
    assert all_three.size >= 1
    # ... and on one of them each camera's row has a loss of its own: stereo under L2, RGB-D under Cauchy, monocular under L1
    want = {(0., 0.), (1., 2.), (2., 1.)}
    assert any(want <= {(g[0], g[2]) for g in lp.obs_groups[lp.obs_grp[lp.obs_point == j]]} for j in all_three)
    assert sc.underdetermined(lp).size == 0
    if name == 'high_group_ids':
        assert lp.obs_groups.shape[0] == 255 and set(np.unique(lp.obs_grp)) == set(sc.HIGH_IDS)
        assert {127, 128, 200, 254} <= set(sc.HIGH_IDS)
        low, _ = sc.scene('mixed_wave', shape)
        assert np.array_equal(lp.obs_groups[lp.obs_grp], low.obs_groups[low.obs_grp]) and np.array_equal(lp.obs_uvd, low.obs_uvd)
    elif name == 'wide_mixed':
        assert lp.obs_groups.shape[0] == lp.num_obs > 255 and np.unique(lp.stiff3, axis=0).shape[0] == lp.num_obs
    else:
        assert lp.obs_groups.shape[0] == 6


@pytest.mark.parametrize('name', sc.MIXED_SCENES)
def test_the_oracle_evaluates_all_three_cameras_finitely(name):
    """Blocks, weights and costs of every row; the one NaN is the host's L1 weight of the dead monocular row, which the scaled
    blocks pin to 1 as the device does."""
    lp, _ = sc.scene(name)
    r, Jp, Jl = orc.eval_reproj(lp)
    assert all(np.all(np.isfinite(a)) for a in (r, Jp, Jl))
    mono = ld.mono_rows(lp)
    assert not r[mono, 2].any() and not Jp[mono, 2].any() and not Jl[mono, 2].any()
    w = ld._per_loss(lp, orc.loss_weight, r)
    l1 = lp.obs_groups[lp.obs_grp, 2] == 1.
    assert np.all(np.isnan(w[mono & l1, 2])) and np.all(np.isfinite(np.delete(w, 2, axis=1)))
    assert np.all(np.isfinite(w[~(mono & l1)]))
    assert all(np.all(np.isfinite(a)) for a in ld.scaled_blocks(lp))
    assert np.isfinite(ld.costs(lp)).all()
    if lp.obs_groups.shape[0] <= 255:                      # (row by row over a table of one group per observation: minutes)
        assert ld.costs(lp)[0] == pytest.approx(orc.eval_cost(lp, True), rel=1e-14)
    # both branches of Huber's and Cauchy's weights occur
    huber = lp.obs_groups[lp.obs_grp, 2] == 3.
    assert np.any(w[huber] < 1.) and np.any(w[huber] == 1.)
