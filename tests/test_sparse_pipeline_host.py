"""What of the sparse VO pipelines needs no GPU: the golden of the verbatim reference run (tests/golden/sparse_vo.npz,
tools/gen_sparse_golden.py) still describes today's inputs and today's matcher definition, and the classes have the
reference's surface."""
import hashlib
import os

import numpy as np

from pyslam_amd import synthetic
from pyslam_amd.pipelines import featproc as fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'sparse_vo.npz')


def golden_scene(g):
    """The inputs of the golden run, rebuilt from the recorded generator arguments (tools/gen_sparse_golden.py: scene)."""
    seed, hole = int(g['seed']), float(g['hole_fraction'])
    seq = synthetic.stereo_sequence(int(g['height']), int(g['width']), int(g['n_frames']), seed=seed, cell=float(g['cell']),
                                    step=tuple(g['step']))
    holes = np.random.default_rng(seed + 1000).random(seq['depth'].shape)
    depth = seq['depth'].copy()
    depth[holes < hole] = np.nan
    depth[(holes >= hole) & (holes < 2 * hole)] = 0.
    return seq['left'], depth


def golden_matches(g):
    """Per tracked frame the replayed (n, 8) match list, None for the first frame."""
    out, at = [], 0
    for n in g['match_len']:
        if n < 0:
            out.append(None)
        else:
            out.append(g['match_flat'][at:at + 8 * n].reshape(n, 8))
            at += 8 * n
    return out


def reference_frame_of(g, k):
    """Frame index of the keyframe the k-th tracked frame was matched against."""
    active_before = 0 if g['mode'][k] == 'track' and g['mode'][k - 1] == 'map' else int(g['active_idx'][k - 1])
    return int(g['keyframe_frames'][active_before])


def test_golden_inputs_are_the_generators():
    g = np.load(GOLDEN)
    images, depth = golden_scene(g)
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(images).tobytes())
    h.update(np.ascontiguousarray(depth).tobytes())
    assert np.array_equal(np.frombuffer(h.digest(), dtype=np.uint8), g['checksum'])
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_golden_matches_are_what_the_restatement_produces_today():
    g = np.load(GOLDEN)
    images, _ = golden_scene(g)
    feats = [fp.features(im) for im in images]
    recorded = golden_matches(g)
    assert recorded[0] is None and sum(m is not None for m in recorded) == len(recorded) - 1
    for k in range(1, len(recorded)):
        ref, f = reference_frame_of(g, k), int(g['frame_idx'][k])
        m, _ = fp.match((feats[ref], None), (feats[f], None), 0)
        assert np.array_equal(m, recorded[k]), (k, ref, f)


def test_class_surface_equals_the_recorded_one():
    from pyslam.pipelines import SparseVOPipeline, SparseStereoPipeline, SparseRGBDPipeline
    from pyslam.pipelines.sparse import SparseRGBDPipeline as shim
    from pyslam.sensors import RGBDCamera, StereoCamera
    from liegroups import SE3
    assert shim is SparseRGBDPipeline and issubclass(SparseStereoPipeline, SparseVOPipeline)
    g = np.load(GOLDEN)
    cu, cv, fu, fv, w, h = g['cam']
    for cls, cam, pre in ((SparseRGBDPipeline, RGBDCamera(cu, cv, fu, fv, int(w), int(h)), 'default_'),
                          (SparseStereoPipeline, StereoCamera(cu, cv, fu, fv, 0.12, int(w), int(h)), 'stereo_default_')):
        p = cls(cam, SE3.identity())
        assert sorted(vars(p)) == list(g[pre + 'attributes'])
        o = p.motion_options
        assert np.array_equal(np.array([o.allow_nondecreasing_steps, o.max_nondecreasing_steps, o.min_cost_decrease, o.max_iters,
                                        o.num_threads, o.linesearch_max_iters, o.min_update_norm, o.min_cost], dtype=float),
                              g[pre + 'options'])
        assert p.keyframe_trans_thresh == float(g[pre + 'keyframe_trans_thresh'])
        assert p.keyframe_rot_thresh == float(g[pre + 'keyframe_rot_thresh'])
        assert p.matcher_mode == int(g[pre + 'matcher_mode']) and p.mode == str(g[pre + 'mode'])
        assert np.array_equal(p.reprojection_stiffness, g[pre + 'reprojection_stiffness'])
        assert type(p.loss).__name__ == str(g[pre + 'loss_name'])
        assert [p.ransac.ransac_iters, p.ransac.ransac_thresh, p.ransac.num_min_set_pts] == list(g[pre + 'ransac'])
        assert len(p.T_c_w) == int(g[pre + 'num_T_c_w']) and len(p.keyframes) == int(g[pre + 'num_keyframes'])
        assert p.camera is cam and p.first_pose is p.T_c_w[0]
        p.set_mode('track')
        assert p.mode == 'track' and p.active_keyframe_idx == 0 and p.T_c_w == []


def test_matcher_parameters_are_the_restatements():
    from pyslam_amd.pipelines.matcher import Matcher_parameters
    d, h = Matcher_parameters(), fp.Params()
    assert vars(d) == vars(h)
