"""The blocked dense factorisation chain (csrc/ps_host_bchol.h: k_bchol_panel / k_bchol_update / k_btri_inverse / k_btri_merge /
k_btri_clear + k_xcg_ainv) against its numpy restatement (tests/bchol_restatement.py), stage by stage through the test entry
ps_debug_dense_factor, at the chain's tile edges (24, 32, 4, 192 and its doublings, 64) -- the coarse level, the lagged inverse's
direct seed, the covariance marginals and the generic direct solve all run this one launch sequence, and all but the marginals
forgive a wrong factor.  Then the generic routes that sit on it or beside it (ps_sparse_normal_direct without refinement,
ps_dense_normal_solve, ps_sparse_normal_solve) at their own edges.

Bounds: every figure of the device chain is held against bchol_restatement.MULT (8) times the same figure of LAPACK's float64
chain (measured against an extended-precision factorisation), with a floor of n 2^-52; the measured ratios are in DESIGN.md
section 4.  Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import bchol_restatement as br

pytestmark = pytest.mark.gpu

SENTINEL = 123.0


def _run(A, **kw):
    from pyslam_amd.device import dense_factor
    return dense_factor(A, **kw)


@pytest.mark.parametrize('n', br.SIZES)
@pytest.mark.parametrize('name', br.FAMILIES)
def test_every_stage_against_the_restatement(name, n):
    ref = br.reference(name, n)
    A = ref.A
    exp = _run(A, dense_out=False, ld_extra=7, ainv_fill=SENTINEL)     # the explicit PCG's form, A^-1 with ld = n + 7
    den = _run(A, dense_out=True)                                      # the folded CG's form
    assert exp['diag_fail'] == 0 and den['diag_fail'] == 0
    low, blk = br.lower(n), br.same_block(n)
    ainv = exp['ainv'][:, :n]
    f, b = ref.figures(exp['L'], exp['Tinv'], exp['Li'], ainv), ref.bounds()
    print('\nbchol %-6s n = %3d: ' % (name, n) + ', '.join(
        '%s %.2e (LAPACK %.2e, ratio to max(LAPACK, n eps) %.3f)' % (k, f[k], ref.fig[k], f[k] / max(ref.fig[k], n * br.EPS))
        for k in ('L', 'Tinv', 'Li', 'res')) + ', fp32 inverse %.2e (bound %.2e)' % (f['inv'], b['inv']))
    # L below the diagonal tiles, the tiles' inverses, L^-1: relative to the truth, as LAPACK's own
    for k in ('L', 'Tinv', 'Li'):
        assert f[k] <= b[k], (k, f[k], b[k])
    # || Li A Li^T - I ||_max
    assert f['res'] <= b['res'], (f['res'], b['res'])
    # the tiles are lower triangular and zero-padded
    assert not np.triu(exp['Tinv'], 1).any()
    # LiT = Li^T bit for bit
    assert np.array_equal(exp['LiT'].T[low], exp['Li'][low])
    # what the explicit form still promises outside the lower triangle: the 192 x 192 diagonal blocks are written whole
    assert not exp['Li'][blk & ~low].any() and not exp['LiT'][blk & low & ~np.eye(n, dtype=bool)].any()
    # dense output: the same L^-1, zeros everywhere else -- k_btri_clear removed every merge intermediate, partial pairs included
    assert np.array_equal(den['Li'][low], exp['Li'][low]) and np.array_equal(den['LiT'], den['Li'].T)
    assert not den['Li'][~low].any() and not den['LiT'][~low.T].any()
    assert np.array_equal(den['L'][br.below_tiles(n)], exp['L'][br.below_tiles(n)]) and np.array_equal(den['Tinv'], exp['Tinv'])
    # A^-1 in fp32: symmetric bit for bit, the reference inverse to fp32 rounding + the fp64 term, the padding untouched
    assert np.array_equal(ainv, ainv.T)
    assert f['inv'] <= b['inv'], (f['inv'], b['inv'])
    assert np.all(exp['ainv'][:, n:] == SENTINEL)
    assert np.array_equal(den['ainv'], ainv)


@pytest.mark.parametrize('where', ['first', 'second_tile', 'last_partial_tile'])
def test_an_indefinite_matrix_is_counted_and_the_call_returns(where):
    n = 200                                                    # 8 full tiles and one of 8 columns
    A = br.family('gram', n)
    pos = {'first': 0, 'second_tile': 30, 'last_partial_tile': 195}[where]
    A[pos, pos] = -A[pos, pos]
    for dense in (False, True):
        out = _run(A, dense_out=dense)
        assert out['diag_fail'] > 0


def test_a_nan_in_the_lower_triangle_is_counted():
    A = br.family('gram', 200)
    A[150, 20] = np.nan
    assert _run(A)['diag_fail'] > 0
    A = br.family('gram', 200)
    A[199, 198] = np.nan                                       # inside the last partial tile
    assert _run(A)['diag_fail'] > 0


def test_only_the_lower_triangle_is_read():
    n = 257
    A = br.family('chain', n)
    B = A.copy()
    B[3, 50] = -7.0
    B[200, 256] = np.nan
    a, b = _run(A, dense_out=True), _run(B, dense_out=True)
    assert b['diag_fail'] == 0
    for k in ('Tinv', 'Li', 'LiT', 'ainv'):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.array_equal(a['L'][br.below_tiles(n)], b['L'][br.below_tiles(n)])


@pytest.mark.parametrize('n', [67, 385, 800])
def test_two_calls_are_bit_identical(n):
    A = br.family('chain', n)
    for dense in (False, True):
        a, b = _run(A, dense_out=dense), _run(A, dense_out=dense)
        for k in ('L', 'Tinv', 'Li', 'LiT', 'ainv'):
            assert a[k].tobytes() == b[k].tobytes(), (k, dense)    # (what a form leaves unspecified included: NaN pre-fill or intermediates)


@pytest.mark.parametrize('produce', [0, 8])
@pytest.mark.parametrize('aggressor', [0, 1, 2])
@pytest.mark.parametrize('ncb', [64, 133])
def test_the_chain_is_a_function_of_its_input_whatever_runs_beside_it(ncb, aggressor, produce):
    """Stress mode 4: 20 reruns of the chain + k_xcg_ainv on an ordinary stream beside streaming / LDS-scribbling kernels, with
    and without its input produced by a kernel in front: every fp32 inverse equals the idle run's bit for bit."""
    from pyslam_amd.device import factor_stress
    A = br.family('gram', ncb * 6)
    n_diff, n_pivot = factor_stress(A, ncb, 6, 1, 4 | produce, 20, lowprio=0, aggressor=aggressor)
    assert (n_diff, n_pivot) == (0, 0)


# ---- the generic routes at the edges ---------------------------------------------------------------------------------------------
def _sparse_j(n, seed):
    """J random sparse plus identity rows, as in tests/test_gpu_edges.py."""
    import scipy.sparse as sp
    extra = max(2, n // 10)
    R = sp.random(n + extra, n, density=min(1.0, 3.0 / n), random_state=seed, format='csr')
    return (R + sp.vstack([sp.identity(n), sp.csr_matrix((extra, n))])).tocsr()


def _relres(H, x, rhs):
    return float(np.linalg.norm(rhs - H @ x) / np.linalg.norm(rhs))


@pytest.mark.parametrize('form', ['r', 'rhs'])
@pytest.mark.parametrize('n', [1, 23, 24, 25, 67, 100, 193, 500])
def test_direct_solve_without_refinement_stands_on_the_factor_alone(n, form):
    """ps_sparse_normal_direct with refine_steps = 0: k_spd_normal, the blocked factor and k_spd_subst with nothing to repair
    them.  Bound on the relative residual: MULT x that of np.linalg.solve on the same dense normal matrix (floor n eps); on the
    step: cond(H) x (both residuals), since ||x - y|| <= ||H^-1|| (||r_x|| + ||r_y||) and ||rhs|| <= ||H|| ||x||."""
    from pyslam_amd.device import sparse_normal_direct
    J = _sparse_j(n, seed=n)
    H = (J.T @ J).toarray()
    rng = np.random.default_rng(n + 1)
    if form == 'r':
        r = rng.standard_normal(J.shape[0])
        rhs, kw = -(J.T @ r), dict(r=r)
    else:
        rhs = rng.standard_normal(n)
        kw = dict(rhs=rhs)
    want = np.linalg.solve(H, rhs)
    fig = _relres(H, want, rhs)
    bnd = br.bound(fig, n)
    dx0, _, rel0 = sparse_normal_direct(J, refine_steps=0, **kw)
    dx3, _, rel3 = sparse_normal_direct(J, **kw)
    mine0, kappa = _relres(H, dx0, rhs), np.linalg.cond(H)
    err0 = float(np.linalg.norm(dx0 - want) / np.linalg.norm(want))
    print('\ndirect n = %3d %-3s: relres %.2e (recomputed %.2e; numpy %.2e, bound %.2e), step error %.2e (cond %.1e), refined relres %.2e'
          % (n, form, rel0, mine0, fig, bnd, err0, kappa, rel3))
    assert rel0 <= bnd and mine0 <= bnd
    assert err0 <= kappa * (bnd + fig)
    assert rel3 <= rel0
    assert np.linalg.norm(dx3 - want) <= kappa * (bnd + fig) * np.linalg.norm(want)


def test_direct_solve_reports_an_empty_column_and_returns_no_step():
    from pyslam_amd import _native as nat
    from pyslam_amd.device import sparse_normal_direct
    n = 67
    J = _sparse_j(n, seed=3).tolil()
    J[:, 40] = 0.0
    J = J.tocsr()
    J.eliminate_zeros()
    r = np.ones(J.shape[0])
    for steps in (0, 3):
        with pytest.raises(nat.NativeError, match='not positive definite'):
            sparse_normal_direct(J, r=r, refine_steps=steps)
    # the C entry itself: the caller's dx is left as it was, no NaN handed back as a step
    lib = nat.require_gpu()
    Jt = J.T.tocsr()
    Jt.sort_indices()
    a = [np.ascontiguousarray(x, dtype=t) for x, t in ((J.indptr, np.int32), (J.indices, np.int32), (J.data, np.float64),
                                                        (Jt.indptr, np.int32), (Jt.indices, np.int32), (Jt.data, np.float64))]
    dx = np.full(n, 5.0)
    rel = C.c_double()
    rc = lib.ps_sparse_normal_direct(J.shape[0], n, nat.i32p(a[0]), nat.i32p(a[1]), nat.f64p(a[2]), nat.i32p(a[3]), nat.i32p(a[4]),
                                     nat.f64p(a[5]), nat.f64p(r), None, 0, nat.f64p(dx), C.cast(C.byref(rel), nat.c_f64p))
    assert rc != 0 and np.all(dx == 5.0)


@pytest.mark.parametrize('cov', [False, True])
@pytest.mark.parametrize('n', [1, 5, 255, 256, 257, 300])
def test_dense_normal_solve_beyond_four_unknowns(n, cov):
    """k_dense_normal + k_dense_chol_solve (one workgroup; one right-hand side per thread, 256 threads: with the covariance,
    n + 1 columns -- from n = 256 on the column loop wraps).  J is (2 n + 3) x n Gaussian: cond(J^T J) ~ 34.  Bounds as for the
    direct solve, the floor with m + n in place of n (the device forms J^T J itself, m terms per entry)."""
    from pyslam_amd.device import dense_normal_solve
    rng = np.random.default_rng(100 + n)
    m = 2 * n + 3
    J, r = rng.standard_normal((m, n)), rng.standard_normal(m)
    H, g = J.T @ J, -(J.T @ r)
    want = np.linalg.solve(H, g)
    kappa = np.linalg.cond(H)
    fig = _relres(H, want, g)
    tol = kappa * (br.MULT + 1) * max(fig, (m + n) * br.EPS)
    out = dense_normal_solve(J, r, want_covariance=cov)
    dx = out[0] if cov else out
    err = float(np.linalg.norm(dx - want) / np.linalg.norm(want))
    print('\ndense n = %3d cov %d: step error %.2e (bound %.2e, cond %.1f)' % (n, cov, err, tol, kappa))
    assert err <= tol
    if cov:
        inv = np.linalg.inv(H)
        figi = float(np.abs(H @ inv - np.eye(n)).max())
        toli = kappa * (br.MULT + 1) * max(figi, (m + n) * br.EPS)
        erri = float(np.abs(out[1] - inv).max() / np.abs(inv).max())
        print('dense n = %3d covariance error %.2e (bound %.2e)' % (n, erri, toli))
        assert erri <= toli and np.abs(out[1] - out[1].T).max() <= toli * np.abs(inv).max()


def test_dense_normal_solve_refuses_a_rank_deficient_jacobian():
    """A zero column: the pivot is exactly zero, which is what the kernel's test (d > 0) promises to catch -- a column that merely
    repeats another leaves a pivot of rounding size and either sign."""
    from pyslam_amd import _native as nat
    from pyslam_amd.device import dense_normal_solve
    rng = np.random.default_rng(5)
    for n, col in ((5, 4), (257, 100)):
        J = rng.standard_normal((2 * n, n))
        J[:, col] = 0.0
        for cov in (False, True):
            with pytest.raises(nat.NativeError, match='not positive definite'):
                dense_normal_solve(J, rng.standard_normal(2 * n), want_covariance=cov)


@pytest.mark.parametrize('form', ['r', 'rhs'])
@pytest.mark.parametrize('n', [1, 256, 257, 1025])
def test_sparse_cg_at_the_partial_sum_block_edges(n, form):
    """ps_sparse_normal_solve (k_sp_*): 1, 1, 2 and 5 workgroups of partial sums in k_sp_dot / k_sp_update, folded by k_sp_scalars.
    A well-conditioned J with a known solution.  The CG stops on the Jacobi-preconditioned residual, ||r||_M^-1 <= tol ||b||_M^-1:
    in the variables scaled by D^1/2 (D = diag J^T J) that is a relative residual, so the scaled error is at most cond(D^-1/2 H
    D^-1/2) tol, and the unscaled one sqrt(cond D) times that; the recurrence's drift adds n eps of the same kind."""
    from pyslam_amd.device import sparse_normal_solve
    J = _sparse_j(n, seed=40 + n)
    H = (J.T @ J).toarray()
    x_true = np.random.default_rng(n).standard_normal(n)
    tol = 1e-12
    kw = dict(r=-(J @ x_true)) if form == 'r' else dict(rhs=H @ x_true)
    dx, its, rel = sparse_normal_solve(J, tol=tol, max_iters=2000, **kw)
    d = np.diag(H)
    Hs = H / np.sqrt(d)[:, None] / np.sqrt(d)[None, :]
    bnd = np.linalg.cond(Hs) * np.sqrt(d.max() / d.min()) * (tol + n * br.EPS)
    want = np.linalg.solve(H, H @ x_true)
    err = float(np.linalg.norm(dx - want) / np.linalg.norm(want))
    print('\nsparse CG n = %4d %-3s: %d iterations, rel %.2e, step error %.2e (bound %.2e)' % (n, form, its, rel, err, bnd))
    assert rel <= tol and (its > 0 or n == 1)
    assert err <= bnd
