"""CPU: the oracle pieces the dense device tests (tests/test_gpu_dense_kernels.py) compare against -- the vectorised
image lookup, the longdouble normal equations with their magnitude sums, and the host restatement of the dense
pipeline's coarse-to-fine solve -- pinned to the loop oracle and to the goldens of the verbatim reference."""
import numpy as np
import pytest

from oracle import photo_oracle as po
from pyslam_amd.problem import Options

from test_photometric import TAGS, gold, tables_of  # noqa: F401  (gold: the photometric.npz fixture)


def test_vectorised_bilinear_is_the_loop_bit_for_bit():
    from conftest import load_golden
    rng = np.random.default_rng(11)
    im = rng.uniform(0, 255, (13, 17))
    h, w = im.shape
    # inside, on the last row / column, on pixel centres and up to 2.5 pixels outside on every side
    x = np.concatenate([rng.uniform(-2.5, w + 1.5, 400), np.arange(w, dtype=float), np.full(h, w - 1.), [0., -0., w - 1e-12]])
    y = np.concatenate([rng.uniform(-2.5, h + 1.5, 400), np.full(w, h - 1.), np.arange(h, dtype=float), [h - 1., 0., -1e-12]])
    assert ((x < 0) | (x > w - 1) | (y < 0) | (y > h - 1)).sum() >= 60
    np.testing.assert_array_equal(po.bilinear_vec(im, x, y), po.bilinear(im, x, y))
    g = load_golden('bilinear')
    np.testing.assert_array_equal(po.bilinear_vec(g['im'], g['x'], g['y']), g['out'])
    np.testing.assert_array_equal(po.bilinear_vec(g['im'], g['x'], g['y']), po.bilinear(g['im'], g['x'], g['y']))


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('loss', [(0, 1.), (1, 1.), (2, 5.), (3, 10.), (4, 25.), (5, 3.)])
def test_longdouble_normal_equations_against_float64(gold, tag, loss):
    """The float64 sums of normal_equations() differ from the longdouble ones by no more than float64 summation allows:
    (n + 2) eps times the magnitude sums, element by element."""
    tb, eps = tables_of(gold, tag), np.finfo(float).eps
    for k in (0, 1):
        T = gold[tag + '_T%d' % k]
        H, b, cost, n = po.normal_equations(tb, gold[tag + '_im_track'], 1.0, 0.25, T[:3, :3], T[:3, 3], *loss)
        q = po.normal_equations_ld(tb, gold[tag + '_im_track'], 1.0, 0.25, T[:3, :3], T[:3, 3], *loss)
        assert q['n'] == n > 0 and q['H'].dtype == np.longdouble
        if loss[0] == 1 and q['min_abs_r'] <= 1e-8:      # L1 at a zero residual: NaN weight in both
            assert np.isnan(H).any() and np.isnan(q['H'].astype(float)).any()
            continue
        c = (n + 2) * eps
        assert np.all(np.abs(H - q['H']) <= c * q['abs_H'])
        assert np.all(np.abs(b - q['b']) <= c * q['abs_b'])
        assert abs(cost - q['cost']) <= c * q['abs_cost']
        assert np.all(q['abs_H'] >= np.abs(q['H'])) and np.all(q['abs_b'] >= np.abs(q['b']))


def test_longdouble_cholesky():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((6, 6))
    H = (A @ A.T + 0.1 * np.eye(6)).astype(np.longdouble)
    b = rng.standard_normal(6).astype(np.longdouble)
    x = po.chol_solve_ld(H, b)
    np.testing.assert_allclose(x.astype(float), np.linalg.solve(H.astype(float), b.astype(float)), rtol=1e-12)
    assert np.abs((H @ x - b).astype(float)).max() < 1e-15 * float(np.abs(H).max() * np.abs(x).max())
    H[1, :] = H[:, 1] = 0
    assert po.chol_solve_ld(H, b) is None                               # a zero pivot: not positive definite
    H[1, 1] = np.nan
    assert po.chol_solve_ld(H, b) is None


def test_dense_solve_restatement_reproduces_the_reference_pipeline():
    """tests/golden/dense_rgbd.npz, the first tracked frame (frame 1 against keyframe 0 from the identity guess): the host
    restatement of the level solve -- longdouble normal equations, Problem.solve's stopping rule, the pipeline's level
    sequence with level 3 rotation-only -- has the verbatim reference's iteration counts, cost histories and pose."""
    from pyslam_amd.liegroups import SE3
    from conftest import load_golden
    g = load_golden('dense_rgbd')
    o = Options()
    o.allow_nondecreasing_steps, o.max_nondecreasing_steps, o.min_cost_decrease = True, 5, 0.99
    o.max_iters, o.linesearch_max_iters = 30, 0
    seq = [int(l) for l in g['default_pyrlevel_sequence']]
    assert seq == [3, 2, 1, 0]
    var = float(g['default_intensity_stiffness']) ** -2
    f0, f1 = int(g['frame_idx'][0]), int(g['frame_idx'][1])
    lv = po.dense_levels(g['images'][f0], g['depth'][f0], g['images'][f1], g['cam'], seq, [l > 2 for l in seq], var, var,
                         float(g['default_min_grad']))
    T0 = SE3.from_matrix(g['T_true'][0])
    guess = T0.dot(T0.inv())                                             # the pipeline's first guess
    out = po.dense_solve(lv, o, 3, float(g['default_loss_k']), guess.rot.as_matrix(), np.asarray(guess.trans))
    assert out['iters'] == list(g['iterations'][1])
    offs = np.concatenate([[0], np.cumsum(g['hist_len'])])
    for l in range(4):
        np.testing.assert_allclose(out['hists'][l], g['hist_flat'][offs[l]:offs[l + 1]], rtol=1e-12, atol=0)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = out['R'], out['t']
    np.testing.assert_allclose(T @ g['T_true'][0], g['T_c_w'][1], rtol=0, atol=1e-12)
    assert np.array_equal(lv[0]['tb']['tri_jac_d'][:, 2], np.ones(lv[0]['tb']['im_ref'].size))


def test_dense_solve_failure_exits():
    """The restatement raises where the device reports a failure: no pixels, and a gradient that has no v component."""
    u = np.arange(64, dtype=float)
    img = np.tile(np.round(128 + 100 * np.sin(u / 5.)), (48, 1)).astype(np.uint8)
    trk = np.tile(np.round(128 + 100 * np.sin((u + 0.7) / 5.)), (48, 1)).astype(np.uint8)
    depth = np.full((48, 64), 2.0)
    o = Options()
    o.linesearch_max_iters = 0
    cam = (31.5, 23.5, 57.6, 57.6, 64, 48)
    lv = po.dense_levels(img, depth, trk, cam, [0], [False], 1e-4, 1e-4, 0.1)
    assert np.all(lv[0]['tb']['im_jac'][:, 1] == 0) and lv[0]['tb']['im_ref'].size > 100
    with pytest.raises(po.DenseSolveError, match='not positive definite'):
        po.dense_solve(lv, o, 3, 10., np.eye(3), np.zeros(3))
    lv = po.dense_levels(img, depth, trk, cam, [0], [False], 1e-4, 1e-4, 1e9)
    assert lv[0]['tb']['im_ref'].size == 0
    with pytest.raises(po.DenseSolveError, match='fewer than 6'):
        po.dense_solve(lv, o, 3, 10., np.eye(3), np.zeros(3))
