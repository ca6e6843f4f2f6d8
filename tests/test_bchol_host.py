"""Host side of the blocked dense factorisation chain's tests: the restatement (tests/bchol_restatement.py) against itself, the
matrix families with their condition numbers, and the DETERMINISTIC pin of k_bchol_panel's slab mapping through the host-only
export ps_debug_bchol_slab (which walks the kernel's own mapping function): no row of a panel belongs to two workgroups.  The
mapping this replaced is restated as the negative example and must fail the same check."""
import numpy as np
import pytest

import bchol_restatement as br


def test_extended_precision_is_extended_and_the_restatement_agrees_with_itself():
    assert np.finfo(br.LD).eps < 2.0 ** -60          # (x87 80-bit: the truth is 11 bits finer than what it judges)
    for name in br.FAMILIES:
        for n in (1, 23, 25, 67, 193):
            ref = br.reference(name, n)
            A = ref.A
            # LAPACK's chain is a Cholesky chain: L L^T = A, Li L = I, Ainv A = I, to the figures it states for itself
            assert np.abs(ref.L @ ref.L.T - A).max() <= 8 * n * br.EPS * np.abs(A).max()
            assert np.abs(ref.Li @ ref.L - np.eye(n)).max() <= 64 * n * br.EPS * max(1.0, np.abs(ref.Li).max() * np.abs(ref.L).max())
            # ... and sits within a small multiple of n EPS kappa of the truth; the truth is far closer to A than float64 resolves
            Lt = ref.L_true
            assert np.abs((Lt @ Lt.T).astype(np.float64) - A).max() <= 2 * br.EPS * np.abs(A).max()
            assert np.abs((ref.Li_true @ Lt).astype(np.float64) - np.eye(n)).max() <= 4 * br.EPS
            for k, v in ref.fig.items():
                assert np.isfinite(v) and v >= 0.0, (name, n, k)
            # the figures of the chain applied to itself are its own figures, and within its own bounds
            own = ref.figures(ref.L, ref.Tinv, ref.Li, ref.Ainv.astype(np.float32))
            b = ref.bounds()
            for k in ('L', 'Tinv', 'Li'):
                assert own[k] == ref.fig[k] and own[k] <= b[k], (name, n, k)
            assert own['res'] <= b['res'] and own['inv'] <= b['inv']      # (products: BLAS may sum in another order per layout)
            # the tiles are the inverses of L's diagonal tiles, zero-padded
            for s in range(ref.Tinv.shape[0]):
                w = min(br.W, n - s * br.W)
                T = ref.L[s * br.W:s * br.W + w, s * br.W:s * br.W + w]
                assert np.abs(ref.Tinv[s, :w, :w] @ T - np.eye(w)).max() <= 64 * w * br.EPS * max(1.0, np.abs(ref.Tinv[s]).max() * np.abs(T).max())
                assert not ref.Tinv[s, w:].any() and not ref.Tinv[s, :, w:].any()


def test_a_wrong_stage_leaves_the_bounds_by_orders_of_magnitude():
    """What the GPU test would see of a kernel that is subtly wrong: one panel entry computed from a half-updated row (the
    hazard's signature), one lost 16-column chunk of a merge product, one tile of the inverse not mirrored."""
    ref = br.reference('gram', 193)
    n, b = ref.n, ref.bounds()
    L = ref.L.copy()
    L[100, 30] *= 1.0 + 1e-6                                  # (a half-updated row changes an entry by O(1), not by 1e-6)
    assert abs(ref.L[100, 30]) > 1e-3 * np.abs(ref.L[100]).max()
    assert ref.figures(L, ref.Tinv, ref.Li, ref.Ainv.astype(np.float32))['L'] > 100 * b['L']
    Li = ref.Li.copy()
    Li[192, :16] = 0.0                                        # row 192 is the merged block's first row
    f = ref.figures(ref.L, ref.Tinv, Li, ref.Ainv.astype(np.float32))
    assert f['Li'] > 1e6 * b['Li'] and f['res'] > 1e6 * b['res']
    inv = ref.Ainv.astype(np.float32)
    inv[:64, 128:192] = 0.0
    assert ref.figures(ref.L, ref.Tinv, ref.Li, inv)['inv'] > 1e3 * b['inv']


def test_matrix_families_are_what_they_say(capsys):
    with capsys.disabled():
        print()
        for name in br.FAMILIES:
            for n in (25, 193, 800):
                A = br.family(name, n)
                d = 1.0 / np.sqrt(np.diag(A))
                w = np.linalg.eigvalsh(A * d[:, None] * d[None, :])           # (positive definite: judged on the unit diagonal)
                c, cs = br.conds(A)
                print('bchol family %-6s n = %3d: condition number %.2e (unit diagonal: %.2e)' % (name, n, c, cs))
                assert A.shape == (n, n) and np.array_equal(A, A.T) and w[0] > 0
                if name == 'gram':
                    assert c < 10
                if name == 'chain':
                    bw = np.abs(np.subtract.outer(np.arange(n), np.arange(n)))[A != 0].max()
                    assert bw <= 11 and (n < 100 or c > 1e3)                 # block tridiagonal in 6 x 6 blocks, chain-like
                if name == 'scaled':
                    assert c > 1e10 and cs < 10 and np.abs(A).max() / np.abs(A)[A != 0].min() > 1e12
    assert br.family('gram', 67).tobytes() == br.family('gram', 67).tobytes()     # deterministic generators


# ---- the slab mapping ---------------------------------------------------------------------------------------------------------
MS = list(range(0, 201)) + [1000, 8168]


def exported_ranges(m, w):
    from pyslam_amd.device import bchol_slab
    grid = bchol_slab(m, w, 0)[3]
    out = []
    for b in range(grid):
        lo, hi, entries, g = bchol_slab(m, w, b)
        assert g == grid
        assert entries == (hi - lo) * w, 'workgroup %d of (m %d, w %d) owns %d cells of rows [%d, %d): not whole rows' % (b, m, w, entries, lo, hi)
        out.append((lo, hi))
    return grid, out


@pytest.mark.parametrize('w', range(1, 25))
def test_no_panel_row_belongs_to_two_workgroups(w):
    """For every tile width and every panel height that matters (0 .. 200, 1000, and 8168 = the direct solve's first step): the
    workgroups' row ranges, as the kernel's own mapping function gives them, partition [0, m) in whole rows of at most 1024
    entries, and the grid is what bchol_chain launches (the same function) = ceil(m / (1024 // w)), 1 for the tile alone."""
    for m in MS:
        grid, ranges = exported_ranges(m, w)
        assert grid == br.grid_of(m, w) and ranges == br.new_slab_ranges(m, w), (m, w)
        br.check_slab_partition(ranges, m, w)
        # one workgroup past the grid owns nothing
        from pyslam_amd.device import bchol_slab
        assert bchol_slab(m, w, grid)[2] == 0


def test_the_replaced_mapping_fails_the_same_check():
    """1024 consecutive ENTRIES per workgroup: with w = 24 every slab boundary cuts a row (1024 is no multiple of 24), so from
    the first two-workgroup launch on (m = 43) a row is read by one workgroup while another overwrites it."""
    assert br.old_slab_ranges(100, 24)[:2] == [(0, 43), (42, 86)]            # row 42: columns 0..15 | 16..23
    for m in (43, 67 - 24, 100, 200, 1000, 8168):
        with pytest.raises(AssertionError, match='twice'):
            br.check_slab_partition(br.old_slab_ranges(m, 24), m, 24)
    bad = sum(1 for w in range(1, 25) for m in MS if _fails(br.old_slab_ranges(m, w), m, w))
    assert bad > 1000                                                          # (every w that does not divide 1024, every m beyond one slab)
    # widths that divide 1024 never cut a row: the old mapping passes there, which is why only full steps (w = 24) mattered
    for w in (1, 2, 4, 8, 16):
        for m in MS:
            br.check_slab_partition(br.old_slab_ranges(m, w), m, w)
    # and the grid grows by what whole rows cost: 1024 / (42 * 24) - 1 = 1.6 %
    assert br.grid_of(8168, 24) == 195 and len(br.old_slab_ranges(8168, 24)) == 192


def _fails(ranges, m, w):
    try:
        br.check_slab_partition(ranges, m, w)
    except AssertionError:
        return True
    return False


def test_slab_export_refuses_bad_arguments_without_a_device():
    from pyslam_amd import _native as nat
    from pyslam_amd.device import bchol_slab
    for m, w, b in ((-1, 24, 0), (10, 0, 0), (10, 25, 0), (10, 24, -1)):
        with pytest.raises(nat.NativeError, match='ps_debug_bchol_slab'):
            bchol_slab(m, w, b)
