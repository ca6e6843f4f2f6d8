"""The pose pass with both observations of a thread requested up front and its 33 sums formed at the end (csrc/ps_k_linearize.h:
k_pose_pass_pf, option "pose_prefetch", default) against k_pose_pass (option 0): the same terms enter every sum in the same order,
so everything the pass leaves behind is compared bit for bit -- its partial sums per item, the reduced system with and without
damping, two whole iterations, the parameters, the cost history of a solve.  The two-observations-per-thread shape exists only
from 131 072 observations on variable poses, so the main problem is that large, trimmed until the last items of its first six
variable poses end everywhere a second trip can: 1, 255, 256, 257, 511 and 512 observations.  No reference counterpart (the
reference evaluates block by block on the host: pyslam/problem.py:338-360)."""
import functools

import numpy as np
import pytest

from pyslam_amd import synthetic, losses
from pyslam_amd.problem import Options
from test_gpu_packed import ragged_ba

pytestmark = pytest.mark.gpu

RESIDUES = (1, 255, 256, 257, 511, 0)          # observations of the first six variable poses, mod 512


def trim_to_residues(lp, residues=RESIDUES, chunk=512, min_track=3):
    """Drop observations of the first len(residues) variable poses until their counts are the residues mod `chunk`; only rows
    whose landmark keeps at least `min_track` observations go."""
    track = np.bincount(lp.obs_point, minlength=lp.num_points)
    keep = np.ones(lp.num_obs, dtype=bool)
    rid_of_obs = lp.pose_rid[lp.obs_pose]
    for r, want in enumerate(residues):
        rows = np.flatnonzero(rid_of_obs == r)
        need = (rows.size - want) % chunk
        cand = rows[track[lp.obs_point[rows]] > min_track]
        # (a pose sees a landmark once, so the candidates' landmarks are distinct: one decrement each)
        assert np.unique(lp.obs_point[cand]).size == cand.size >= need
        keep[cand[:need]] = False
        track[lp.obs_point[cand[:need]]] -= 1
    assert track.min() >= min_track
    out = lp.copy()
    out.obs_pose, out.obs_point = lp.obs_pose[keep], lp.obs_point[keep]
    out.obs_uvd, out.obs_grp = lp.obs_uvd[keep], lp.obs_grp[keep]
    return out.finalize()


@functools.lru_cache(maxsize=None)
def big():
    """Nine keyframes (eight variable), 30 000 landmarks of six observations, 5 % of them constant: more than 131 072 observations
    on variable poses after the trim, so the handle cuts 512-observation items."""
    lp, _ = synthetic.stereo_ba(num_kf=9, num_lm=30000, obs_per_lm=6, half_window=4, seed=5, const_point_fraction=0.05)
    lp = trim_to_residues(lp)
    assert np.count_nonzero(lp.pose_rid[lp.obs_pose] >= 0) >= 131072 and np.count_nonzero(lp.point_vid < 0) > 1000
    return lp


def big_mixed():
    """The same rows, a seeded random third of them in a second group (another stiffness, Huber): the two observations of a
    thread, and the lanes of a wave, disagree about the group."""
    lp = big().copy()
    lp.stiff3 = np.vstack([lp.stiff3, (np.diag([0.8, 1.1, 0.6])).reshape(1, 9)])
    lp.obs_groups = np.vstack([lp.obs_groups, [0., 1., *synthetic._loss_row(losses.HuberLoss(1.5))]])
    grp = lp.obs_grp.copy()
    grp[np.random.default_rng(17).random(lp.num_obs) < 1. / 3.] = 1
    lp.obs_grp = grp
    return lp.finalize()


def big_wide():
    """The same rows, one group (its own stiffness) per observation: more than 255 rows, the WIDE instantiations."""
    lp = big().copy()
    n = lp.num_obs
    scale = 0.5 + np.random.default_rng(23).random((n, 3))
    stiff = np.zeros((n, 9))
    stiff[:, [0, 4, 8]] = scale * np.diag(lp.stiff3[0].reshape(3, 3))
    lp.stiff3 = stiff
    lp.obs_groups = np.column_stack([np.zeros(n), np.arange(n, dtype=float), np.full(n, lp.obs_groups[0, 2]), np.full(n, lp.obs_groups[0, 3])])
    lp.obs_grp = np.arange(n, dtype=np.int32)
    return lp.finalize()


def short_poses():
    """Four keyframes, forty landmarks seen from all of them: every variable pose has fewer than 64 observations (one wave of an
    item works, three are absent)."""
    lp, _ = synthetic.stereo_ba(num_kf=4, num_lm=40, obs_per_lm=4, half_window=4, seed=3)
    assert np.bincount(lp.obs_pose).max() < 64
    return lp


CASES = [
    ('big', big, True),
    ('big_mixed_groups', big_mixed, True),
    ('big_wide', big_wide, True),
    # below the threshold: 256-observation items, one observation per thread -- the same kernel, its second half idle
    ('ragged16', lambda: ragged_ba(5), False),
    ('short_poses', short_poses, False),
]


def everything(lp, on):
    """What the pose pass leaves behind on a fresh handle, and the cost history of a whole solve on another."""
    from pyslam_amd.device import DeviceProblem
    dev = DeviceProblem(lp)
    assert dev.get_option('pose_prefetch') == 1             # default on
    dev.set_option('pose_prefetch', on)
    assert dev.get_option('pose_prefetch') == on
    dev.linearize(0.0)                                      # <WIDE, false>
    items, partial = dev.pose_items()
    out = [partial] + list(dev.reduced_system())
    dev.linearize(1e-3)                                     # <WIDE, true>: the six damping sums too
    out += [dev.pose_items()[1]] + list(dev.reduced_system())
    out.append(np.array(dev.gn_iteration(0.0, 1e-12, 1000, True)))
    out.append(np.array(dev.gn_iteration(0.0, 1e-12, 1000, True)))
    out += list(dev.get_params())
    dev.close()
    dev = DeviceProblem(lp)
    dev.set_option('pose_prefetch', on)
    opt = Options()
    opt.max_iters, opt.allow_nondecreasing_steps = 6, True
    hist, its, _ = dev.solve_loop(opt)
    out.append(np.array(hist))
    out.append(np.array(its))
    out += list(dev.get_params())
    dev.close()
    return items, out


@pytest.mark.parametrize('name,make,two_trips', CASES, ids=[c[0] for c in CASES])
def test_option_on_equals_option_off_bit_for_bit(name, make, two_trips):
    lp = make()
    items, on = everything(lp, 1)
    items0, off = everything(lp, 0)
    assert np.array_equal(items, items0) and items.shape[0] > 0
    length = items[:, 2] - items[:, 1]
    if two_trips:
        # 512-observation items, and the last item of the first six variable poses ends where a second trip can: one lane, 255
        # lanes, none (256: the first trip exactly), one lane past it, 255 lanes past it, a full item
        assert length.max() == 512
        last = np.array([length[items[:, 0] == r][-1] for r in range(len(RESIDUES))])
        assert tuple(last % 512) == RESIDUES and last[-1] == 512 and 1 in last
        assert np.count_nonzero(lp.point_vid[lp.obs_point[lp.pose_rid[lp.obs_pose] >= 0]] < 0) > 0      # rows with v < 0
    else:
        assert length.max() <= 256
    if name == 'big_mixed_groups':
        assert lp.obs_groups.shape[0] == 2 and 0.25 < np.mean(lp.obs_grp == 1) < 0.42
    if name == 'big_wide':
        assert lp.obs_groups.shape[0] == lp.num_obs > 255
    if name == 'short_poses':
        assert length.max() < 64
    assert len(on) == len(off)
    for k, (a, b) in enumerate(zip(on, off)):
        assert np.array_equal(a, b, equal_nan=True), (name, k)
    assert np.all(on[0][:, 27:] == 0.0) and np.all(on[5][:, 27:30] > 0.0)      # damping sums: compiled out / formed
    assert np.all(np.isfinite(on[-4])) and on[-4][-1] < on[-4][0]              # (a solve that went somewhere)
