"""Loop detection on the device: the places scene through Matcher.dbQuery, the two-visits scene through loop.detect_loop against the
restatement chain and the truth, and SparseMonoPipeline with ``loop_detection`` on a camera that goes out and comes back through a map
that joins the two ends already.  Run with `-m gpu` on an MI355X.  Every comparison prints its figure before it asserts.

What the comparisons rely on is asserted on the host (tests/test_loop_host.py over tests/loop_scenes.py): every query's place wins by
1.5 x, no pair of a two-visits chain lies within the rounding margin of the threshold, the truth bounds are twice the host figures."""
import numpy as np
import pytest

import loop_scenes as ls
import mono_scenes as ms
import sim3_scenes as s3

pytestmark = pytest.mark.gpu

TOL_UV = 1e-12           # pixels (the matcher's bound)


def new_matcher():
    from pyslam_amd.pipelines.matcher import Matcher
    return Matcher()


def test_places_scores_equal_the_restatements():
    m = new_matcher()
    try:
        for d in ls.places_db():
            m.dbAdd(d)
        for (s, f), ref in ls.places_scores().items():
            m.pushBack(ls.place_sequence(s)['images'][f])
            scores = m.dbQuery()
            print('place {} frame {}: device {} restatement {}'.format(s, f, scores.tolist(), ref.tolist()))
            assert np.array_equal(scores, ref)
    finally:
        m.close()


@pytest.mark.parametrize('size', ['small', 'big'])
def test_two_visits(size):
    from pyslam_amd.pipelines.loop import detect_loop
    from pyslam_amd.pipelines.sim3 import Sim3RANSAC
    seq = ls.visit_sequence(size)
    cam = ms.camera(seq['cam'])
    entry = ls.visit_entry(size)
    entries = [entry] + [None] * (len(ls.visit_db(size)) - 1)       # a wrong place would be verified against None: it never is
    m = new_matcher()
    try:
        for d in ls.visit_db(size):
            m.dbAdd(d)
        for f in ls.VISIT_FRAMES:
            h = ls.host_visit(size, f)
            rs = Sim3RANSAC(cam)
            hit = detect_loop(cam, m, seq['images'][f], lambda uv: ls.visit_points(size, f, uv), entries, seed=ls.VISIT_SEED,
                              ransac=rs)
            assert hit is not None and hit[0] == 0
            _, scale, T_21, pairs = hit
            info = m.loop_query_['verified'][-1][1]
            T = T_21.as_matrix()
            err = ls.visit_errors(scale, T[:3, :3], T[:3, 3], size, f)
            print('{} frame {}: scores {}, {} pairs (host {}), {} inliers (host {}), scale {:.6f} (host {:.6f}), errors {:.5g} / {:.5g} '
                  'deg / {:.5g}'.format(size, f, m.loop_query_['scores'].tolist(), info['pairs'], len(h['pairs']), len(pairs),
                                        h['res']['count'], scale, h['res']['scale'], err['e_scale'], err['e_rot_deg'], err['e_t']))
            # the matched pairs: what the RANSAC was given
            assert info['matched'] == info['bound'] == info['pairs'] == len(h['pairs']) and info['connected'] == 0
            feature, status, _, _, uv = m.matchMapGlobal((4, 5))   # the verification's match, once more
            rows = np.nonzero(status == 0)[0]
            assert np.array_equal(np.stack([rows, feature[rows]], axis=1), h['pairs'])
            assert np.abs(uv[rows] - h['uv']).max() <= TOL_UV
            # the inlier pairs, from the same samples
            assert np.array_equal(rs.info_['mask'], h['res']['mask'])
            assert np.array_equal(pairs, h['inlier_pairs'])
            bound = ls.TRUTH_BOUND[size]
            assert err['e_scale'] <= bound[0] and err['e_rot_deg'] <= bound[1] and err['e_t'] <= bound[2]
            gap = s3.model_error(rs.info_['S_21'], scale, h['res']['S_21'], h['res']['scale'])
            print('    device against the host chain: rotation {:.2e} rad, translation {:.2e}, scale {:.2e}'.format(*gap))
    finally:
        m.close()


def run_pipeline(loop_detection):
    from pyslam_amd.pipelines.mono import SparseMonoPipeline
    p = SparseMonoPipeline(ms.camera(ms.sequence()['cam']))
    p.local_ba = False
    p.loop_detection = loop_detection
    p.loop_gap = ls.LOOP_GAP
    np.random.seed(ms.PIPELINE_SEED)
    for im in ls.out_and_back():
        p.track(im)
    return p


def test_no_loop_where_the_map_joins_the_two_ends_and_the_switch_changes_nothing_else():
    images = ls.out_and_back()
    on, off = run_pipeline(True), run_pipeline(False)
    try:
        kf_images = []
        for kf in on.keyframes:                                # every image but the turning point occurs twice: the next occurrence
            kf_images.append(next(f for f in range(kf_images[-1] + 1 if kf_images else 0, len(images)) if np.array_equal(images[f], kf.image)))
        print('keyframes at images {}, landmarks {}'.format(kf_images, on.landmark_counts))
        for q in on.loop_queries:
            print('keyframe {}: scores {}, candidates {}, verifications {}'.format(q['keyframe'], q['scores'].tolist(),
                                                                                  q['candidates'].tolist(), q['verified']))
        print('the host pipeline\'s keyframes: {}'.format(ls.OUT_AND_BACK_KEYFRAMES))
        assert off.matcher.dbSize() == (0, 0) and off.loop_queries == [] and off.loop_closures == []
        assert on.matcher.dbSize()[0] == len(on.keyframes) and on.matcher.dbSize()[1] == sum(kf.desc.shape[0] for kf in on.keyframes)
        # everything else is bit-identical
        assert len(on.T_c_w) == len(off.T_c_w) == len(images) and len(on.keyframes) == len(off.keyframes)
        for a, b in zip(on.T_c_w, off.T_c_w):
            assert (a is None) == (b is None) and (a is None or a.as_matrix().tobytes() == b.as_matrix().tobytes())
        for a, b in zip(on.keyframes, off.keyframes):
            assert np.array_equal(a.image, b.image) and a.T_c_w.as_matrix().tobytes() == b.T_c_w.as_matrix().tobytes()
            assert np.array_equal(a.landmark, b.landmark) and np.array_equal(a.desc, b.desc)
        assert on.landmark_counts == off.landmark_counts and on.points_w.tobytes() == off.points_w.tobytes()
        assert np.array_equal(on.alive, off.alive) and np.array_equal(on.obs_lm, off.obs_lm) and on.obs_uv.tobytes() == off.obs_uv.tobytes()
        # the loop: the last keyframes are back at the start, the old keyframes score, and what they share is the map's own
        assert len(on.keyframes) > ls.LOOP_GAP + 1 and len(on.loop_queries) == len(on.keyframes) - ls.LOOP_GAP - 1
        assert on.loop_closures == []
        last = on.loop_queries[-1]
        assert last['keyframe'] == len(on.keyframes) - 1 and last['candidates'].size > 0 and last['verified']
        assert last['verified'][-1][1]['connected'] > 0
    finally:
        on.matcher.close()
        off.matcher.close()
