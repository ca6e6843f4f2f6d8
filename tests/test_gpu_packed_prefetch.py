"""The packed observation passes with their operands requested in four dependent trips (csrc/ps_k_packed.h: PF, option
"packed_prefetch", default) against the same kernels in the load order they had before (option 0): only WHERE a load is issued
differs, so everything they leave behind is compared bit for bit -- landmark factors and the reduced system they feed, the cost,
the step, the updated parameters, the cost history of a whole solve.  Plus the run record the kernels read (LmwRun) against the
tables it is made from, for both structure builders, and a closed gate.  No reference counterpart (the reference evaluates block
by block on the host: pyslam/problem.py:338-360)."""
import numpy as np
import pytest

from pyslam_amd import synthetic, losses
from pyslam_amd.problem import Options
from test_gpu_packed import ragged_ba

pytestmark = pytest.mark.gpu


def every_landmark_sees_pose_0(seed=3, num_lm=200):
    """Four keyframes, every landmark observed from all of them, pose 0 constant: a row with rid = -1 in every landmark, so in
    every run."""
    lp, _ = synthetic.stereo_ba(num_kf=4, num_lm=num_lm, obs_per_lm=4, half_window=4, seed=seed)
    assert lp.pose_rid[0] < 0 and np.bincount(lp.obs_point[lp.obs_pose == 0], minlength=lp.num_points).min() >= 1
    return lp


CASES = [
    ('ragged16', lambda: ragged_ba(5)),
    ('two_obs', lambda: synthetic.stereo_ba(num_kf=12, num_lm=500, obs_per_lm=2, half_window=3, seed=9)[0]),
    ('sixteen', lambda: synthetic.stereo_ba(num_kf=40, num_lm=300, obs_per_lm=16, half_window=10, seed=4, const_point_fraction=0.1)[0]),
    ('ragged7_huber', lambda: ragged_ba(6, max_obs=7, loss=losses.HuberLoss(1.5))),
    # edges: one wave (48 rows); a last workgroup of fewer than four runs; constant-pose rows in every run
    ('one_wave', lambda: every_landmark_sees_pose_0(seed=7, num_lm=12)),
    ('short_last_group', lambda: synthetic.stereo_ba(num_kf=6, num_lm=100, obs_per_lm=4, half_window=3, seed=1)[0]),
    ('const_pose_rows', every_landmark_sees_pose_0),
]
# (runs on the handle, runs in the last workgroup) the edge cases are there for
SHAPES = {'one_wave': (1, 1), 'short_last_group': (7, 3), 'const_pose_rows': (14, 2)}


def everything(lp, on):
    """What the packed passes leave behind on a fresh handle, and the cost history of a whole solve on another."""
    from pyslam_amd.device import DeviceProblem
    dev = DeviceProblem(lp)
    dev.set_option('packed_prefetch', on)
    assert dev.get_option('packed_prefetch') == on
    nw = dev.packed_runs()[0].shape[0]
    out = [np.float64(dev.eval_cost(True))]                 # k_cost_packed (or the landmark pass summing on its way)
    dev.linearize(0.0)                                      # k_landmark_pass_packed<.., false>
    out += list(dev.landmark_factors())                     # C^-1, c
    out += list(dev.reduced_system())                       # S, g: what Z feeds
    out.append(np.array(dev.gn_iteration(0.0, 1e-12, 1000, True)))     # cost after the step, ||dx||, iterations, residual
    out += list(dev.get_dx())                               # dx_pose, dx_l: k_backsub_packed
    out += list(dev.get_params())                           # ... and its fused update
    out.append(dev.packed_runs()[3])                        # the partials of ||dx_l||^2
    out.append(np.array(dev.gn_iteration(0.0, 1e-12, 1000, True)))     # a second call: the landmark pass of the tail before it
    out += list(dev.get_params())
    dev.close()
    dev = DeviceProblem(lp)
    dev.set_option('packed_prefetch', on)
    opt = Options()
    opt.max_iters, opt.allow_nondecreasing_steps = 6, True
    hist, its, _ = dev.solve_loop(opt)
    out.append(np.array(hist))
    out.append(np.array(its))
    out += list(dev.get_params())
    dev.close()
    return nw, out


@pytest.mark.parametrize('name,make', CASES, ids=[c[0] for c in CASES])
def test_option_on_equals_option_off_bit_for_bit(name, make):
    lp = make()
    nw, on = everything(lp, 1)
    nw0, off = everything(lp, 0)
    assert nw == nw0 and nw > 0                              # (the packed kernels run: no track longer than 16)
    if name in SHAPES:
        assert (nw, nw - 4 * ((nw - 1) // 4)) == SHAPES[name]
    assert len(on) == len(off)
    for k, (a, b) in enumerate(zip(on, off)):
        assert np.array_equal(a, b, equal_nan=True), (name, k)
    assert np.isfinite(on[0]) and np.all(np.isfinite(on[-4])) and on[-4][-1] < on[0]       # (a solve that went somewhere)


@pytest.mark.parametrize('mode', ['0', '2'], ids=['host_build', 'device_build'])
def test_the_run_records_are_the_run_starts_and_lm_ptr(mode, monkeypatch):
    """LmwRun[w] = {first[w], first[w + 1], lm_ptr[first[w]], lm_ptr[first[w + 1]] - lm_ptr[first[w]]}, first[w] = the first
    landmark whose first row is >= W w: recomputed here from the handle's lm_ptr, for the host builder's loop and for the device
    builder's kernel (PS_CREATE_DEVICE=2, as tests/test_gpu_packed.py switches it)."""
    from pyslam_amd.device import DeviceProblem
    monkeypatch.setenv('PS_CREATE_DEVICE', mode)
    lp = ragged_ba(11, num_kf=40, num_lm=900, max_obs=12)
    dev = DeviceProblem(lp)
    run, first, lm_ptr, _ = dev.packed_runs()
    bytes_held = dev.get_info()['device_bytes']
    dev.close()
    nv = lm_ptr.size - 1
    per_lm = np.diff(lm_ptr)
    # lm_ptr itself: the variable landmarks' track lengths, in some slot order
    counts = np.bincount(lp.point_vid[lp.obs_point][lp.point_vid[lp.obs_point] >= 0], minlength=nv)
    assert nv == counts.size and np.array_equal(np.sort(per_lm), np.sort(counts))
    W = 64 - (per_lm.max() - 1)
    nw = -(-int(lm_ptr[-1]) // W)
    assert run.shape == (nw, 4) and nw > 4
    first_ref = np.r_[np.searchsorted(lm_ptr[:nv], W * np.arange(nw), side='left'), nv].astype(np.int32)
    assert np.array_equal(first, first_ref)
    row0 = lm_ptr[first_ref[:-1]]
    run_ref = np.stack([first_ref[:-1], first_ref[1:], row0, lm_ptr[first_ref[1:]] - row0], axis=1)
    assert np.array_equal(run, run_ref)
    assert run[:, 3].min() >= 1 and run[:, 3].max() <= 64 and run[:, 3].sum() == lm_ptr[-1]
    assert bytes_held > 16 * nw


def test_a_closed_gate_leaves_everything_where_it_was():
    """Tukey weights that vanish on every observation leave H_ll = 0 and a NaN reduced system: the CG reports breakdown (status 2,
    tests/test_gpu_edges.py), the gated tail -- back-substitution with its fused update, the next landmark pass -- finds its gate
    closed.  With the operands prefetched it must still store nothing: points, poses, dx_l and the partials of ||dx_l||^2 are
    what they were."""
    from pyslam_amd.device import DeviceProblem
    from pyslam_amd._native import NativeError
    lp, _ = synthetic.stereo_ba(num_kf=30, num_lm=1200, obs_per_lm=4, half_window=5, seed=2, loss=losses.TukeyLoss(1e-9))
    dev = DeviceProblem(lp)
    assert dev.get_option('packed_prefetch') == 1 and dev.packed_runs()[0].shape[0] > 0
    poses, points = dev.get_params()
    dxl, sq = dev.get_dx()[1], dev.packed_runs()[3]
    with pytest.raises(NativeError, match='landmark block'):
        dev.gn_iteration(0., 1e-12, 500, True)
    after = dev.get_params()
    assert np.array_equal(poses, after[0]) and np.array_equal(points, after[1])
    assert np.array_equal(dxl, dev.get_dx()[1], equal_nan=True) and np.array_equal(sq, dev.packed_runs()[3], equal_nan=True)
    dev.close()
