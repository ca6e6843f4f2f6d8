"""Launches taken off the linearisation's critical path (option "lin_zero_list": trailing workgroups of the pose pass zero what
a linearisation accumulates into, in place of a fill over all of [S | g | cost | status]) are re-plumbing: with the option on
and off every value is the same to the last bit, a handle that is linearised a second time carries nothing over from the
first, and handles the split of S into stored and accumulated blocks does not hold for keep the fill.

Tolerance: bit identity between the two settings; the reduced system against the oracle's Schur complement at the 1e-12 of
tests/test_gpu_parity.py::test_reduced_system (the oracle's own error; measured maxima there 4e-14)."""
import numpy as np
import pytest

from oracle import gn_oracle as orc
from pyslam_amd import synthetic
from conftest import rel_err

pytestmark = pytest.mark.gpu

OPTIONS = ('lin_zero_list',)
TOL_BLOCK = 1e-12


def device(lp, on, **kw):
    from pyslam_amd.device import DeviceProblem
    dev = DeviceProblem(lp, **kw)
    if not on:
        for name in OPTIONS:
            dev.set_option(name, 0)
    return dev


def oracle_reduced(lp, lam=0.):
    """Schur complement of the oracle's (damped) normal equations in device order (poses by rid, landmarks by vid)."""
    P, b, _ = orc.normal_equations(lp, points_first=False, lm_lambda=lam)
    n = lp.dof * lp.num_reduced
    P = P.toarray()
    Hpp, Hpl, Hll = P[:n, :n], P[:n, n:], P[n:, n:]
    if Hll.shape[0] == 0:
        return Hpp, b[:n]
    Hinv = np.linalg.inv(Hll)
    return Hpp - Hpl @ Hinv @ Hpl.T, b[:n] - Hpl @ Hinv @ b[n:]


def moved(lp, seed, scale=2e-3):
    """The problem at another point: every unknown moved by a small random step (through the oracle's own retraction)."""
    _, _, n = orc.unknown_offsets(lp, False)
    return orc.apply_update(lp, scale * np.random.default_rng(seed).standard_normal(n), points_first=False)


def stage(dev, lam, with_landmarks=True):
    """One staged Gauss-Newton step: everything a caller can read on the way."""
    dev.linearize(lam)
    _, _, vals, g = dev.reduced_system()
    S, _ = dev.reduced_dense()
    fac = dev.landmark_factors() if with_landmarks else (np.zeros(0), np.zeros(0))
    dev.solve_reduced(1e-13, 3000)
    dev.backsub()
    xp, xl = dev.get_dx()
    dev.apply_update(1.0)
    poses, points = dev.get_params()
    cost = dev.eval_cost(True)
    return dict(vals=vals, g=g, S=S, cinv=fac[0], c=fac[1], xp=xp, xl=xl, poses=poses, points=points, cost=np.array(cost))


def assert_same_bits(a, b, what=''):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def assert_oracle(out, lp, lam):
    So, go = oracle_reduced(lp, lam)
    err_S, err_g = rel_err(out['S'], So), rel_err(out['g'], go)
    print('reduced system vs oracle: S %.2e  g %.2e' % (err_S, err_g))
    assert err_S < TOL_BLOCK and err_g < TOL_BLOCK


def counters(dev):
    return int(dev.get_option('lin_zero_launches')), int(dev.get_option('lin_fills'))


@pytest.mark.parametrize('lam', [0., 1e-3])
@pytest.mark.parametrize('shape', [(6, 40), (12, 200)])
def test_a_second_linearisation_carries_nothing_over_from_the_first(shape, lam):
    """Linearise at A, move the parameters, linearise at B on the SAME handle: S holds A's values when the second linearisation
    starts, and nothing but the pair kernel's stores and the list's zeros stands between them and B's.  Equal, bit for bit, to
    fresh handles at B with the option on and off (lambda = 1e-3: the finalisation adds lambda * diag into the diagonal)."""
    lpA, _ = synthetic.stereo_ba(num_kf=shape[0], num_lm=shape[1], obs_per_lm=4, half_window=3, seed=21)
    lpB = moved(lpA, 5)
    stale = device(lpA, True)
    assert stale.get_option('lin_zero_list') == 1
    stale.linearize(lam)
    valsA = stale.reduced_system()[2].copy()
    stale.set_params(lpB.poses, lpB.points)
    got = stage(stale, lam)
    assert counters(stale) == (2, 0)
    assert not np.array_equal(valsA, got['vals'])                # (the point did move)
    fresh_on, fresh_off = device(lpB, True), device(lpB, False)
    assert fresh_off.get_option('lin_zero_list') == 0
    on, off = stage(fresh_on, lam), stage(fresh_off, lam)
    assert counters(fresh_on) == (1, 0) and counters(fresh_off) == (0, 1)
    assert_same_bits(on, off, 'on / off')
    assert_same_bits(got, off, 'stale / fresh')
    assert_oracle(got, lpB, lam)
    for d in (stale, fresh_on, fresh_off):
        d.close()


def factor_only_blocks():
    """Stereo BA whose pattern has blocks NO Schur pair writes: pose-to-pose factors between keyframes that share no landmark
    (half_window 2: keyframes five apart never see the same landmark), and a landmark seen from one keyframe only."""
    from pyslam_amd.lowering import pack_pose_matrices
    lp, truth = synthetic.stereo_ba(num_kf=12, num_lm=90, obs_per_lm=3, half_window=2, seed=23)
    first = np.nonzero(lp.obs_point == 0)[0]
    keep = np.ones(lp.num_obs, bool)
    keep[first[1:]] = False                                      # landmark 0: one observation, nothing off the diagonal
    for k in ('obs_pose', 'obs_point', 'obs_uvd', 'obs_grp'):
        setattr(lp, k, getattr(lp, k)[keep])
    T = truth['poses']
    ei, ej = np.array([1, 2, 4]), np.array([7, 9, 11])
    rel = np.einsum('nij,njk->nik', T[ej], np.linalg.inv(T[ei]))
    lp.e_i, lp.e_j = ei, ej
    lp.e_Tobs_inv = pack_pose_matrices(np.linalg.inv(rel))
    lp.e_grp = np.zeros(3)
    lp.stiffd = np.stack([(10. * np.eye(6)).ravel()])
    lp.edge_groups = np.array([[0., 3., 0.7]])                   # Huber: the factor's blocks change with the point
    lp = lp.finalize()
    seen = [set(lp.obs_point[lp.obs_pose == k]) for k in range(12)]
    for a, b in zip(ei, ej):
        assert not (seen[a] & seen[b])                           # the block (a, b) exists through the factor only
    assert (lp.obs_point == 0).sum() == 1
    return lp, ei, ej


def test_a_pattern_block_no_pair_writes_holds_the_factor_alone():
    lpA, ei, ej = factor_only_blocks()
    lpB = moved(lpA, 6)
    stale = device(lpA, True)
    assert stale.get_option('lin_zero_list') == 1
    first = stage(stale, 0.)                                     # (at A; the handle moves on by its own step)
    assert_oracle(first, lpA, 0.)
    stale.set_params(lpB.poses, lpB.points)
    got = stage(stale, 0.)
    on, off = stage(device(lpB, True), 0.), stage(device(lpB, False), 0.)
    assert_same_bits(on, off, 'on / off')
    assert_same_bits(got, off, 'stale / fresh')
    assert_oracle(got, lpB, 0.)
    # the blocks themselves: non-zero, different at the two points, and at B what the oracle says -- not A's plus B's
    So, _ = oracle_reduced(lpB, 0.)
    for a, b in zip(ei, ej):
        ra, rb = lpA.pose_rid[a], lpA.pose_rid[b]
        blk, blk_first = got['S'][6 * ra:6 * ra + 6, 6 * rb:6 * rb + 6], first['S'][6 * ra:6 * ra + 6, 6 * rb:6 * rb + 6]
        assert np.abs(blk).max() > 0 and not np.array_equal(blk, blk_first)
        assert np.abs(blk - So[6 * ra:6 * ra + 6, 6 * rb:6 * rb + 6]).max() <= TOL_BLOCK * np.abs(So).max()


def test_pair_tasks_that_write_a_diagonal_block():
    """A landmark observed twice from one pose: its pair task subtracts from the DIAGONAL block (has_diag_tasks, as
    tests/test_gpu_edges.py::test_duplicate_observations_of_a_pose builds it), which the finalisation also adds into."""
    lp, _ = synthetic.stereo_ba(num_kf=6, num_lm=40, obs_per_lm=4, half_window=3, seed=12)
    dup = np.arange(0, lp.num_obs, 3)
    noise = np.random.default_rng(1).standard_normal((dup.size, 3))
    lp.obs_pose = np.concatenate([lp.obs_pose, lp.obs_pose[dup]])
    lp.obs_point = np.concatenate([lp.obs_point, lp.obs_point[dup]])
    lp.obs_uvd = np.concatenate([lp.obs_uvd, lp.obs_uvd[dup] + noise])
    lp.obs_grp = np.concatenate([lp.obs_grp, lp.obs_grp[dup]])
    lpA = lp.finalize()
    lpB = moved(lpA, 7)
    stale = device(lpA, True)
    assert stale.get_option('lin_zero_list') == 1
    stale.linearize(0.)
    stale.set_params(lpB.poses, lpB.points)
    got = stage(stale, 0.)
    on, off = stage(device(lpB, True), 0.), stage(device(lpB, False), 0.)
    assert_same_bits(on, off, 'on / off')
    assert_same_bits(got, off, 'stale / fresh')
    assert_oracle(got, lpB, 0.)


def test_whole_iterations_are_the_same_bits_with_the_option_off():
    """ps_gn_iteration (landmark pass in the previous tail, lagged set-up, one-launch CG): three iterations, then a cold
    second solve on the same handles."""
    lp, _ = synthetic.stereo_ba(num_kf=40, num_lm=4000, obs_per_lm=6, half_window=8, seed=3)
    on, off = device(lp, True), device(lp, False)
    for d in (on, off):
        d.set_expect_next(True)
    for rnd in range(2):
        for _ in range(3):
            assert on.gn_iteration(0., 1e-12, 1000, True) == off.gn_iteration(0., 1e-12, 1000, True)
        for d in (on, off):
            d.reset_solver_state()
    pa, la = on.get_params()
    pb, lb = off.get_params()
    assert np.array_equal(pa, pb) and np.array_equal(la, lb)
    (zon, fon), (zoff, foff) = counters(on), counters(off)
    assert on.get_info()['landmark_passes_taken_over'] >= 2 and zon >= 6 and fon == 0 and zoff == 0 and foff >= 6


def test_handles_the_split_does_not_hold_for_keep_the_fill(monkeypatch):
    """Tiled Schur (partials + combine: S is summed into), SE(2) poses, a landmark shard: ps_get_option reports the fill, the
    option changes nothing, and their results are those of the oracle."""
    # tiled
    monkeypatch.setenv('PS_SCHUR_TILE_KB', '256')
    monkeypatch.setenv('PS_SCHUR_TILE_MIN_MB', '0')
    lp, _ = synthetic.stereo_ba(num_kf=70, num_lm=6000, obs_per_lm=7, half_window=10, seed=13)
    tiled = device(lp, True)
    monkeypatch.delenv('PS_SCHUR_TILE_MIN_MB')
    monkeypatch.setenv('PS_SCHUR_TILE_KB', '0')                  # (untiled from here on)
    assert tiled.get_option('lin_zero_list') == 0
    tiled.linearize(0.)
    vals = tiled.reduced_system()[2].copy()
    tiled.set_option('lin_zero_list', 0)
    tiled.linearize(0.)
    assert np.array_equal(vals, tiled.reduced_system()[2]) and counters(tiled) == (0, 2)
    untiled = device(lp, True)
    assert untiled.get_option('lin_zero_list') == 1              # (the same problem without tiles is eligible ...)
    untiled.linearize(0.)
    assert rel_err(untiled.reduced_system()[2], vals) < TOL_BLOCK      # (... and sums its pairs in another grouping)
    # SE(2)
    lp2, _ = synthetic.pose_graph(num_poses=60, num_loops=90, dof=3, seed=4, const_first=True)
    se2 = device(lp2, True)
    assert se2.get_option('lin_zero_list') == 0
    out = stage(se2, 0., with_landmarks=False)
    assert counters(se2) == (0, 1)
    assert_oracle(out, lp2, 0.)


def test_a_one_rank_landmark_shard_keeps_the_fill():
    import os
    import torch
    import torch.distributed as dist
    from pyslam_amd.device import DeviceProblem
    from pyslam_amd.distributed import ShardedDeviceProblem
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='29541', RANK='0', WORLD_SIZE='1')
    dist.init_process_group('nccl', device_id=torch.device('cuda', 0))
    try:
        lp, _ = synthetic.stereo_ba(num_kf=40, num_lm=4000, obs_per_lm=6, half_window=8, seed=3)
        ref = DeviceProblem(lp, stream=torch.cuda.current_stream().cuda_stream)
        ref.set_option('lagged_inverse', 0)                      # (as tests/test_gpu_sharded.py: the shard's solve never has it)
        sh = ShardedDeviceProblem(lp, dist, native_rccl=True)
        assert sh.native is not None
        assert sh.dev.get_option('lin_zero_list') == 0 and ref.get_option('lin_zero_list') == 1
        for _ in range(3):
            a = ref.gn_iteration(0., 1e-12, 1000, True)
            b = sh.gn_iteration(0., 1e-12, 1000, True)
            assert a[0] == b[0] and a[2] == b[2]
        pa, la = ref.get_params()
        pb, lb = sh.get_params()
        assert np.array_equal(pa, pb) and np.array_equal(la, lb)
        assert counters(sh.dev)[0] == 0 and counters(sh.dev)[1] >= 3 and counters(ref)[0] >= 3 and counters(ref)[1] == 0
        sh.close()
        ref.close()
    finally:
        dist.destroy_process_group()
