"""The scaled-block products of the fused CG's set-up in registers (option "rows_regs"): one thread owns a row of a block and
forms L_i^-1 S_ij L_j^-T and its products with the basis blocks without storing anything in between; the lagged rows kernel
forms K_i only over the coarse nodes its row reaches; and the first (exact) set-up of a solve runs its block scaling and
coarse row sums as one launch of the rows kernel.  Every sum keeps its terms and their order, so this is re-plumbing: with the
option on and off every value is the same to the last bit.

Tolerance: bit identity between the two settings (np.array_equal); nothing is compared against a bound.

Shapes (rows = blocks per row of the reduced matrix, asserted below from its row_ptr; the rows kernel has 16 waves and
holds rows of up to 96 blocks):
  a  24 keyframes:  rows  9..17   fewer blocks than waves
  b  40 keyframes:  rows 19..37   a block count that is no multiple of the waves
  c  110 keyframes, half window 23: rows 46..93, the longest the kernel admits
  d  110 keyframes, half window 24: longest row 97 -- not eligible, keeps k_scale_blocks + k_coarse_rowsums
The lagged coarse factor L~^-T (nc x nc) is staged in LDS where it fits beside the row: 4 x 93 blocks x 288 B = 107 KB of
shape c leave no room under 160 KB for the 65 - 74 KB of 90 - 96 coarse unknowns ("coarse_groups" 15); the short rows of a
and b do, and so does c with the coarse level the handle chooses itself (printed)."""
import numpy as np
import pytest

import bench
from pyslam_amd import synthetic
from pyslam_amd.problem import device_solve

pytestmark = pytest.mark.gpu

COUNTERS = ('rows_setups', 'exact_row_setups', 'rows_lci_in_lds')
#         num_kf, num_lm, obs_per_lm, half_window, seed, (shortest, longest row), reduced poses
SHAPES = {'a': (24, 500, 5, 4, 31, (9, 17), 23),
          'b': (40, 1200, 8, 9, 5, (19, 37), 39),
          'c': (110, 3000, 10, 23, 3, (46, 93), 109),
          'd': (110, 3000, 10, 24, 3, (None, 97), 109)}


def ba(name):
    kf, lm, opl, hw, seed, _, _ = SHAPES[name]
    lp, _ = synthetic.stereo_ba(num_kf=kf, num_lm=lm, obs_per_lm=opl, half_window=hw, seed=seed)
    return lp


def device(lp, on, groups=None):
    from pyslam_amd.device import DeviceProblem
    dev = DeviceProblem(lp)
    if groups is not None:
        dev.set_option('coarse_groups', groups)
    if not on:
        dev.set_option('rows_regs', 0)
    assert dev.get_option('rows_regs') == (1 if on else 0)
    return dev


def counters(dev):
    return tuple(int(dev.get_option(n)) for n in COUNTERS)


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


def row_lengths(dev):
    rp = dev.reduced_system()[0]
    return np.diff(rp)


@pytest.mark.parametrize('lam', [0., 1e-3])
@pytest.mark.parametrize('name,groups,lci', [('a', None, 1), ('b', None, 1), ('c', None, None), ('c', 15, 0)])
def test_whole_solves_are_the_same_bits(name, groups, lci, lam):
    """1. device_solve under bench.py's example options, switch on and off, fresh handles; the rows kernel ran every set-up."""
    lp = ba(name)
    lo, hi = SHAPES[name][5]
    assert lp.num_reduced == SHAPES[name][6]
    on, off = device(lp, True, groups), device(lp, False, groups)
    n = row_lengths(on)
    assert (n.min(), n.max()) == (lo, hi), (n.min(), n.max())
    a, b = solve(on, options(lam)), solve(off, options(lam))
    print('shape', name, 'groups', groups, 'calls', len(a['its']), 'pcg', a['its'].tolist(), 'counters on', counters(on), 'off', counters(off))
    assert_same_bits(a, b, 'on / off')
    calls = len(a['its'])
    assert calls >= 2
    assert counters(on)[:2] == (calls - 1, 1)             # one exact set-up heads the solve, every later one is lagged
    assert counters(off)[:2] == (calls - 1, 0)            # the same plan, through the forms before
    assert counters(on)[2] == counters(off)[2]
    if lci is not None:
        assert counters(on)[2] == lci
    on.close(); off.close()


@pytest.mark.parametrize('lam', [0., 1e-3])
def test_a_row_too_long_keeps_the_two_launches(lam):
    """1d. The control: one row of 97 blocks, the rows kernel does not apply and the switch changes nothing."""
    lp = ba('d')
    on, off = device(lp, True), device(lp, False)
    assert row_lengths(on).max() == SHAPES['d'][5][1]
    a, b = solve(on, options(lam)), solve(off, options(lam))
    print('calls', len(a['its']), 'pcg', a['its'].tolist(), 'counters on', counters(on), 'off', counters(off))
    assert_same_bits(a, b, 'on / off')
    assert len(a['its']) >= 2
    assert counters(on) == (0, 0, 0) and counters(off) == (0, 0, 0)
    on.close(); off.close()


def test_se2_pose_graph():
    """2. D = 3: the same kernels' other instantiation, on a planar pose graph of 60 poses."""
    lp, _ = synthetic.pose_graph(num_poses=60, num_loops=90, dof=3, seed=4, const_first=True)
    out = {}
    for on in (True, False):
        dev = device(lp, on)
        calls = [dev.gn_iteration(0., 1e-12, 1000, True) for _ in range(4)]
        poses, points = dev.get_params()
        out[on] = dict(calls=np.array(calls), poses=poses, points=points)
        print('on' if on else 'off', 'pcg', [c[2] for c in calls], 'counters', counters(dev))
        assert counters(dev)[:2] == (3, 1 if on else 0)
        dev.close()
    assert_same_bits(out[True], out[False], 'on / off')


def staged(dev, lam):
    dev.linearize(lam)
    first = dev.solve_reduced(1e-13, 3000)
    dev.backsub()
    xp, xl = dev.get_dx()
    second = dev.solve_reduced(1e-13, 3000)
    dev.backsub()
    xp2, xl2 = dev.get_dx()
    return dict(first=np.array(first), second=np.array(second), xp=xp, xl=xl, xp2=xp2, xl2=xl2)


@pytest.mark.parametrize('lam', [0., 1e-3])
def test_the_staged_api(lam):
    """3. linearize -> solve_reduced twice -> backsub: the staged calls take the exact set-up, both times in the rows kernel."""
    lp = ba('b')
    on, off = device(lp, True), device(lp, False)
    a, b = staged(on, lam), staged(off, lam)
    assert_same_bits(a, b, 'on / off')
    assert np.array_equal(a['xp'], a['xp2']) and np.array_equal(a['xl'], a['xl2'])
    print('counters on', counters(on), 'off', counters(off))
    assert counters(on)[:2] == (0, 2) and counters(off)[:2] == (0, 0)
    on.close(); off.close()


def test_the_switch_on_a_live_handle():
    """4. Turned off and on again between the iterations of one handle: the same bits as a handle that never had it on."""
    lp = ba('a')
    live, ref = device(lp, True), device(lp, False)
    got, want = [], []
    for n in range(4):
        live.set_option('rows_regs', n % 2)               # off for the exact set-up of call 0, on for the lagged one of call 1
        got.append(live.gn_iteration(0., 1e-12, 1000, True))
        want.append(ref.gn_iteration(0., 1e-12, 1000, True))
    assert np.array_equal(np.array(got), np.array(want))
    for x, y in zip(live.get_params(), ref.get_params()):
        assert np.array_equal(x, y)
    print('counters live', counters(live), 'ref', counters(ref))
    assert counters(live)[0] == counters(ref)[0] >= 1 and counters(ref)[1] == 0
    live.close(); ref.close()
