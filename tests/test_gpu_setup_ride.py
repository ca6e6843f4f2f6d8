"""The block-Jacobi factor kernel at the head of the reduced solve's set-up rides in a launch that is there anyway (option
"setup_ride"): the factor of a pose is formed by the wave of the pair launch that has just finalised its diagonal block.  Both
routes call one device function, so this is re-plumbing: with the option on and off every value is the same to the last bit,
the factors are used once and formed again by the kernel for every later set-up on the same linearisation, and handles the
finalisation does not end the diagonal blocks for keep the launch.

Tolerance: bit identity between the two settings (np.array_equal); nothing is compared against a bound.

Shapes: a coarse level needs >= 16 reduced poses and > 90 unknowns.  18, 24 and 33 keyframes (the first is constant) give 17,
23 and 32 reduced poses: the last finalising workgroup of the pair launch has 1, 3 and 4 live waves."""
import numpy as np
import pytest

import bench
from oracle import gn_oracle as orc
from pyslam_amd import synthetic
from pyslam_amd.problem import Options, device_solve

pytestmark = pytest.mark.gpu

COUNTERS = ('factor_launches', 'factors_ridden', 'factor_plan_mismatches')
SHAPES = [(18, 400), (24, 500), (33, 600)]


def ba(num_kf, num_lm, seed=31, **kw):
    lp, _ = synthetic.stereo_ba(num_kf=num_kf, num_lm=num_lm, obs_per_lm=5, half_window=4, seed=seed, **kw)
    return lp


def device(lp, on):
    from pyslam_amd.device import DeviceProblem
    dev = DeviceProblem(lp)
    if not on:
        dev.set_option('setup_ride', 0)
    return dev


def counters(dev):
    return tuple(int(dev.get_option(n)) for n in COUNTERS)


def linearisations(dev):
    return int(dev.get_option('lin_zero_launches')) + int(dev.get_option('lin_fills'))


def options(lam):
    opt = bench.example_options()
    opt.lm_lambda = lam
    return opt


def solve(dev, opt):
    hist, stats = device_solve(dev, opt)
    poses, points = dev.get_params()
    return dict(hist=np.array(hist), its=np.array([s[0] for s in stats]), rel=np.array([s[1] for s in stats]), poses=poses, points=points)


def assert_same_bits(a, b, what=''):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize('lam', [0., 1e-3])
@pytest.mark.parametrize('shape', SHAPES)
def test_whole_iteration_calls_are_the_same_bits(shape, lam):
    """1. device_solve under bench.py's example options, switch on and off, fresh handles."""
    lp = ba(*shape)
    assert lp.num_reduced == shape[0] - 1
    on, off = device(lp, True), device(lp, False)
    assert on.get_option('setup_ride') == 1 and off.get_option('setup_ride') == 0
    a, b = solve(on, options(lam)), solve(off, options(lam))
    print('calls', len(a['its']), 'pcg', a['its'].tolist(), 'counters on', counters(on), 'off', counters(off))
    assert_same_bits(a, b, 'on / off')
    assert len(a['its']) >= 2
    fl, fr, mm = counters(on)
    assert fl == 0 and fr == linearisations(on) and mm == 0       # no launch of its own, one ridden per linearisation
    fl, fr, mm = counters(off)
    assert fl == len(b['its']) and fr == 0 and mm == 0            # the reverse: one launch per set-up
    on.close(); off.close()


def staged(dev, lam):
    dev.linearize(lam)
    first = dev.solve_reduced(1e-13, 3000)
    dev.backsub()
    xp, xl = dev.get_dx()
    second = dev.solve_reduced(1e-13, 3000)           # the same linearisation: the ridden factors were consumed by the first
    dev.backsub()
    xp2, xl2 = dev.get_dx()
    return dict(first=np.array(first), second=np.array(second), xp=xp, xl=xl, xp2=xp2, xl2=xl2)


@pytest.mark.parametrize('lam', [0., 1e-3])
def test_the_staged_api_uses_the_ridden_factors_once(lam):
    """2. linearize -> solve_reduced -> backsub, then a second solve_reduced on the same linearisation."""
    lp = ba(24, 500)
    on, off = device(lp, True), device(lp, False)
    a, b = staged(on, lam), staged(off, lam)
    assert_same_bits(a, b, 'on / off')
    assert np.array_equal(a['xp'], a['xp2']) and np.array_equal(a['xl'], a['xl2'])
    print('counters on', counters(on), 'off', counters(off))
    assert counters(on) == (1, 1, 0) and counters(off) == (2, 0, 0)
    on.close(); off.close()


def test_linearize_then_solve_finish_keeps_the_lagged_basis():
    """2b. ps_linearize plans the exact set-up, ps_gn_solve_finish behind it may take the lagged one, which reads the previous
    iteration's basis beside that iteration's X and coarse factor.  A linearisation whose exact plan points at that basis does
    not ride; one whose plan merely differs rides, is counted as a mismatch and the kernel runs.  Three rounds, on and off, bit
    for bit.  The counters follow from the buffers: round 1 has no factor yet (both plan exact: ridden); round 2 would write
    the basis of round 1, which its lagged set-up reads (no ride, no mismatch: a launch); every set-up either takes a ridden
    factor or launches the kernel."""
    lp = ba(24, 500)
    out = {}
    for on in (True, False):
        dev = device(lp, on)
        rounds, seen = [], []
        for _ in range(3):
            dev.linearize(0.)
            rounds.append(dev.gn_solve_finish(1e-12, 1000, True))
            seen.append(counters(dev))
        poses, points = dev.get_params()
        out[on] = dict(rounds=np.array(rounds), poses=poses, points=points)
        print('on' if on else 'off', 'counters per round', seen)
        if on:
            assert seen[0] == (0, 1, 0) and seen[1] == (1, 1, 0)
            for n, (fl, fr, mm) in enumerate(seen, 1):
                assert mm <= fr and fl + fr - mm == n
        else:
            assert seen == [(1, 0, 0), (2, 0, 0), (3, 0, 0)]
        dev.close()
    assert_same_bits(out[True], out[False], 'on / off')


def test_a_second_solve_on_a_live_handle():
    """3. reset_solver_state, move the parameters, solve again: a fresh handle with the switch off gives the same bits."""
    lpA = ba(24, 500)
    _, _, n = orc.unknown_offsets(lpA, False)                  # the same problem from another start
    lpB = orc.apply_update(lpA, 2e-3 * np.random.default_rng(5).standard_normal(n), points_first=False)
    live = device(lpA, True)
    solve(live, options(0.))
    live.reset_solver_state()
    live.set_params(lpB.poses, lpB.points)
    got = solve(live, options(0.))
    fresh = device(lpB, False)
    want = solve(fresh, options(0.))
    assert_same_bits(got, want, 'live on / fresh off')
    fl, fr, mm = counters(live)
    assert fl == 0 and fr == linearisations(live) and mm == 0
    live.close(); fresh.close()


def keeps_the_launch(lp, solver, what):
    """The gate reads 0 whatever the option says, nothing rides, and the option changes no bit."""
    on, off = device(lp, True), device(lp, False)
    assert on.get_option('setup_ride') == 0 and off.get_option('setup_ride') == 0, what
    a, b = solver(on), solver(off)
    assert_same_bits(a, b, what)
    assert counters(on)[1:] == (0, 0) and counters(off)[1:] == (0, 0), what
    on.close(); off.close()


def iterations(dev, n=3):
    out = [dev.gn_iteration(0., 1e-12, 1000, True) for _ in range(n)]
    poses, points = dev.get_params()
    return dict(calls=np.array(out), poses=poses, points=points)


def ba_with_pose_factors():
    """A BA with pose-to-pose factors (as tests/test_gpu_launch_diet.py::factor_only_blocks): they add into the diagonal blocks
    behind the pair launch."""
    from pyslam_amd.lowering import pack_pose_matrices
    lp, truth = synthetic.stereo_ba(num_kf=24, num_lm=500, obs_per_lm=5, half_window=4, seed=31)
    T = truth['poses']
    ei, ej = np.array([1, 2, 4]), np.array([13, 17, 22])
    rel = np.einsum('nij,njk->nik', T[ej], np.linalg.inv(T[ei]))
    lp.e_i, lp.e_j = ei, ej
    lp.e_Tobs_inv = pack_pose_matrices(np.linalg.inv(rel))
    lp.e_grp = np.zeros(3)
    lp.stiffd = np.stack([(10. * np.eye(6)).ravel()])
    lp.edge_groups = np.array([[0., 3., 0.7]])
    return lp.finalize()


def test_handles_that_must_keep_the_launch(monkeypatch):
    """4. Pose-to-pose factors, SE(2), a tiled pair list: the factor kernel keeps its launch."""
    keeps_the_launch(ba_with_pose_factors(), iterations, 'pose-to-pose factors')
    lp2, _ = synthetic.pose_graph(num_poses=60, num_loops=90, dof=3, seed=4, const_first=True)
    keeps_the_launch(lp2, iterations, 'SE(2)')
    monkeypatch.setenv('PS_SCHUR_TILE_KB', '256')
    monkeypatch.setenv('PS_SCHUR_TILE_MIN_MB', '0')
    lpt, _ = synthetic.stereo_ba(num_kf=70, num_lm=6000, obs_per_lm=7, half_window=10, seed=13)
    keeps_the_launch(lpt, iterations, 'tiled')


def test_a_direct_solve_keeps_its_path():
    """4d. <= 15 reduced poses: k_direct_solve takes the system, no factor is formed at all."""
    lp = ba(12, 200)
    assert lp.num_reduced * 6 <= 90
    keeps_the_launch(lp, iterations, 'direct')


def test_the_failure_report_survives_the_move():
    """5. No constant pose, no prior (tests/test_gpu_edges.py): whatever the solve reports with the switch off -- a step or the
    "non-positive-definite diagonal block" error, a numerical status -- it reports with the switch on."""
    from pyslam_amd._native import NativeError
    free = ba(24, 500, const_first_pose=False)
    assert free.num_reduced == 24

    def outcome(on):
        dev = device(free, on)
        assert dev.get_option('setup_ride') == (1 if on else 0)
        try:
            return ('step',) + tuple(dev.gn_iteration(0., 1e-12, 50, True))
        except NativeError as e:
            return ('error', str(e))
        finally:
            dev.close()
    a, b = outcome(True), outcome(False)
    print(b)
    assert a == b


def test_adaptive_lm_with_rejected_steps():
    """6. ps_lm_iteration from a far start: rejected steps linearise the same point again under a raised damping.  The
    trajectory (costs, lambda, rho, decisions, model decrease) is the same on and off."""
    lp = ba(24, 500, seed=1, pose_noise=0.4, point_noise=0.8)
    out = []
    for on in (True, False):
        opt = Options()
        opt.lm_adaptive, opt.lm_lambda, opt.max_iters, opt.min_cost_decrease = True, 1e-3, 8, 0.999999
        opt.pcg_tol, opt.pcg_max_iters = 1e-12, 2000
        dev = device(lp, on)
        res = solve(dev, opt)
        res['lm'] = np.array(dev.lm_history)
        print('lm decisions', res['lm'][:, 2].astype(int).tolist(), 'counters', counters(dev))
        assert counters(dev)[2] == 0 and (counters(dev)[0] == 0) == on
        out.append(res)
        dev.close()
    assert_same_bits(out[0], out[1], 'on / off')
    assert (out[0]['lm'][:, 2] == 0).any()                  # (the case does reject)
