"""The one-launch folded CG (csrc/ps_k_cg_persist.h) leaves as soon as r_new . r_new is below the threshold -- before the exchange
whose products only the NEXT pass's convergence test would have looked past -- and gathers every entry's sums straight from the
granules.  Held against the launch-per-iteration kernels (cg_persist 0) where the early exit meets the launch cap (the pass that
would have detected convergence must exist: at the cap nothing changes), on a right-hand side that is (nearly) zero, in the other
shapes of the kernel (D = 3; more than 512 tasks, whose coarse rows have many tasks: the long-row loop of the gather), and against
itself: every workgroup takes the exit decision from the same bits, so twenty cold solves give one answer.  No exchange is made
to time out here (tests/test_gpu_cg_persist.py does that)."""
import numpy as np
import pytest

from oracle import gn_oracle as orc
from pyslam_amd import synthetic

pytestmark = pytest.mark.gpu

TOL = 1e-13


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _handle(lp, persist):
    from pyslam_amd.device import DeviceProblem
    dev = DeviceProblem(lp)
    dev.set_option('cg_persist', persist)
    dev.set_option('lagged_inverse', 0)
    if lp.num_reduced > 250:                                         # (without the lagged inverse the explicit PCG takes over from 250 poses)
        dev.set_option('cg_explicit_min_rows', 100000)
    return dev


def _ran_in_one_launch(counts, persist):
    if persist:
        assert counts[0] >= 1 and counts[1] == 0, counts
    else:
        assert counts == (0, 0), counts


@pytest.fixture(scope='module')
def ba24():
    return synthetic.stereo_ba(num_kf=24, num_lm=600, obs_per_lm=5, half_window=6, seed=3)[0]


def _staged_solve(lp, persist, cap):
    dev = _handle(lp, persist)
    dev.linearize(0.0)
    its, relres = dev.solve_reduced(TOL, cap)
    dev.backsub()
    xp, xl = dev.get_dx()
    counts = dev.cg_persist_counts()
    dev.close()
    _ran_in_one_launch(counts, persist)
    return its, relres, np.concatenate([xp.ravel(), xl.ravel()])


def test_early_exit_at_the_launch_cap(ba24):
    """pcg_max_iters = K, K - 1, K + 1 around the iteration count K of the uncapped solve: the same iterations (a sum in another
    order may move a count by one), the same converged / not-converged outcome, and the same step where both converged."""
    K = _staged_solve(ba24, 1, 4000)[0]
    assert K >= 3
    for cap in (K, K - 1, K + 1):
        a = _staged_solve(ba24, 1, cap)
        b = _staged_solve(ba24, 0, cap)
        print('cap %d (K = %d): one launch %d its, relres %.3e | per iteration %d its, relres %.3e' % (cap, K, a[0], a[1], b[0], b[1]))
        assert abs(a[0] - b[0]) <= 1
        conv_a, conv_b = a[1] <= TOL * 1.001, b[1] <= TOL * 1.001
        assert conv_a == conv_b
        if conv_a and conv_b:
            assert rel(a[2], b[2]) <= 1e-9


def test_nearly_zero_right_hand_side():
    """A 40-pose SE(3) graph where there is (almost) nothing left to solve for.  The generator's ground truth with noise-free
    measurements does NOT have an exactly zero residual on the host (T_j T_i^-1 (T_j T_i^-1)^-1 is the identity only to rounding:
    the oracle gives max |r| = 3.9e-13, checked below), so the case is built the other way: the parameters are a converged
    solve's output, and both forms must agree on what they make of it."""
    lp0, _ = synthetic.pose_graph(num_poses=40, num_loops=30, dof=6, seed=2, init_noise=0.0, meas_noise=0.0)
    r0 = np.abs(orc.eval_edges(lp0, jac=False)).max()
    assert 0.0 < r0 < 1e-10                                          # (not exactly zero: hence the construction below)
    lp, _ = synthetic.pose_graph(num_poses=40, num_loops=30, dof=6, seed=2)
    ref = _handle(lp, 0)
    for _ in range(12):
        ref.gn_iteration(0.0, 1e-12, 4000, True)
    conv = ref.get_params()
    ref.close()
    out = {}
    for persist in (1, 0):
        dev = _handle(lp, persist)
        dev.set_params(*conv)
        got = dev.gn_iteration(0.0, 1e-12, 4000, True)
        out[persist] = (got, dev.get_params(), dev.cg_persist_counts())
        dev.close()
        _ran_in_one_launch(out[persist][2], persist)
    (a, pa, _), (b, pb, _) = out[1], out[0]
    print('converged start: one launch %r | per iteration %r' % (a, b))
    assert abs(a[0] - b[0]) <= 1e-10 * abs(b[0]) + 1e-18 and abs(a[2] - b[2]) <= 1
    assert np.abs(pa[0] - pb[0]).max() <= 1e-9
    assert np.abs(pa[0] - conv[0]).max() <= 1e-6                     # (nothing left to move)


OTHER = [
    ('se2_graph_200', lambda: synthetic.pose_graph(num_poses=200, num_loops=150, dof=3, seed=4)[0]),     # D = 3
    ('se3_graph_300', lambda: synthetic.pose_graph(num_poses=300, num_loops=200, dof=6, seed=2)[0]),     # 517 tasks, long coarse rows
]


@pytest.mark.parametrize('name,make', OTHER, ids=[c[0] for c in OTHER])
def test_other_shapes_equal_the_launch_per_iteration_kernels(name, make):
    lp = make()
    out = {}
    for persist in (1, 0):
        dev = _handle(lp, persist)
        trace = [dev.gn_iteration(0.0, 1e-12, 4000, True) for _ in range(3)]
        out[persist] = (trace, dev.get_params(), dev.cg_persist_counts())
        dev.close()
        _ran_in_one_launch(out[persist][2], persist)
    a, b = out[1], out[0]
    for ta, tb in zip(a[0], b[0]):
        assert abs(ta[0] - tb[0]) <= 1e-10 * abs(tb[0]) + 1e-18 and abs(ta[2] - tb[2]) <= max(1, tb[2] // 50)
    assert np.abs(a[1][0] - b[1][0]).max() <= 1e-9


def test_twenty_cold_solves_are_bit_identical(ba24):
    from pyslam_amd.device import DeviceProblem
    start = (ba24.poses.copy(), ba24.points.copy())

    def cold(dev):
        dev.reset_solver_state(); dev.set_params(*start)
        return dev.gn_iteration(0.0, 1e-12, 2000, True), dev.get_params()

    dev = DeviceProblem(ba24)
    dev.set_option('lagged_inverse', 0)
    first = cold(dev)
    for _ in range(19):
        got = cold(dev)
        assert got[0] == first[0]
        assert np.array_equal(got[1][0], first[1][0]) and np.array_equal(got[1][1], first[1][1])
    counts = dev.cg_persist_counts()
    dev.close()
    assert counts == (20, 0)
    other = DeviceProblem(ba24)
    other.set_option('lagged_inverse', 0)
    got = cold(other)
    counts = other.cg_persist_counts()
    other.close()
    assert counts == (1, 0)
    assert got[0] == first[0]
    assert np.array_equal(got[1][0], first[1][0]) and np.array_equal(got[1][1], first[1][1])
