"""The recovery x = L^-T (x^_f + P y), y = L_c^-T x^_c of the one-launch folded CG (csrc/ps_k_cg_persist.h, option
cg_persist_recover): every workgroup recovers its own slice of poses inside the launch, from operands it prefetched into LDS.
The yardstick is k_coarse_recover (csrc/ps_k_coarse.h) on the same x^ -- option 0 runs it, gated, behind the launch; x_io carries
the bits the kernel's first workgroup holds, and every workgroup holds the same.  The two forms call one device function
(coarse_recover_ylane / coarse_recover_entry: explicit fma chains in a fixed order), and the parent's two forms -- the recovery by
the first workgroup alone out of memory, and k_coarse_recover -- agreed bit for bit on all five cases below when measured on the
build that had the option but still that recovery: so the comparison is np.array_equal, not a tolerance.
The cases are those of tests/test_gpu_cg_persist.py whose slices differ in kind: ba40 (39 reduced poses: more workgroups than
slices, empty and short ones), ba_with_edges, se3_graph_120 (long coarse rows), se2_graph_200 (D = 3), ba260 (nr no multiple of
the slice)."""
import numpy as np
import pytest

from pyslam_amd import synthetic

pytestmark = pytest.mark.gpu

CASES = [
    ('ba40', lambda: synthetic.stereo_ba(num_kf=40, num_lm=3000, obs_per_lm=10, half_window=8, seed=2)[0]),
    ('ba_with_edges', lambda: synthetic.with_pose_edges(synthetic.stereo_ba(num_kf=60, num_lm=4000, obs_per_lm=6, half_window=9, seed=8)[0], 40, 9)),
    ('se3_graph_120', lambda: synthetic.pose_graph(num_poses=120, num_loops=90, dof=6, seed=3)[0]),
    ('se2_graph_200', lambda: synthetic.pose_graph(num_poses=200, num_loops=150, dof=3, seed=4)[0]),
    ('ba260', lambda: synthetic.stereo_ba(num_kf=260, num_lm=8000, obs_per_lm=10, half_window=20, seed=1)[0]),
]


def run(lp, recover, lds=None):
    """-> (pose part of the staged solve's step, tuples of three whole iterations, parameters, one-launch solves,
    (recovered inside, left to k_coarse_recover), bytes the largest slice needs)"""
    from pyslam_amd.device import DeviceProblem
    dev = DeviceProblem(lp)
    dev.set_option('cg_persist_recover', recover)
    dev.set_option('lagged_inverse', 0)
    if lds is not None:
        dev.set_option('cg_persist_recover_lds', lds)
        assert dev.get_option('cg_persist_recover_lds') == lds
    assert dev.get_option('cg_persist_recover') == recover
    if lp.num_reduced > 250:                                         # (without the lagged inverse the explicit PCG takes over from 250 poses)
        dev.set_option('cg_explicit_min_rows', 100000)
    dev.linearize(0.0)
    dev.solve_reduced(1e-13, 4000)
    dev.backsub()
    xp, _ = dev.get_dx()
    trace = [dev.gn_iteration(0.0, 1e-12, 4000, True) for _ in range(3)]
    out = (xp.copy(), trace, dev.get_params(), dev.cg_persist_counts(), dev.cg_persist_recover_counts(),
           int(dev.get_option('cg_persist_recover_need')))
    dev.close()
    return out


def same(a, b):
    assert np.array_equal(a[0], b[0])
    assert a[1] == b[1]
    assert np.array_equal(a[2][0], b[2][0]) and np.array_equal(a[2][1], b[2][1])


@pytest.mark.parametrize('name,make', CASES, ids=[c[0] for c in CASES])
def test_the_recovery_in_the_launch_equals_k_coarse_recover(name, make):
    lp = make()
    inside = run(lp, 1)
    behind = run(lp, 0)
    solves, failures = inside[3]
    assert solves >= 4 and failures == 0 and behind[3] == inside[3]  # the one-launch form ran (staged solve + three iterations), never failed
    need = inside[5]
    assert 0 < need <= 143 * 1024 and behind[5] == need
    assert inside[4] == (solves, 0) and behind[4] == (0, solves)     # the counters say which form ran
    print(name, 'slice operands', need, 'bytes; largest difference', float(np.abs(inside[0] - behind[0]).max()))
    same(inside, behind)
    # a cap below one slice's need: every launch falls back, to the same bits as option 0
    capped = run(lp, 1, lds=need - 8)
    assert capped[3] == inside[3] and capped[4] == (0, solves)
    same(capped, behind)


def test_the_cap_is_refused_out_of_range():
    from pyslam_amd.device import DeviceProblem
    lp, _ = synthetic.stereo_ba(num_kf=6, num_lm=64, obs_per_lm=4, half_window=3, seed=1)
    dev = DeviceProblem(lp)
    assert dev.get_option('cg_persist_recover') == 1 and dev.get_option('cg_persist_recover_lds') == 143 * 1024
    for bad in (-1.0, 143 * 1024 + 1.0, float('nan')):
        with pytest.raises(Exception, match='cg_persist_recover_lds out of range'):
            dev.set_option('cg_persist_recover_lds', bad)
    assert dev.get_option('cg_persist_recover_lds') == 143 * 1024
    dev.close()
