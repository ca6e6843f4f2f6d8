"""The numpy restatement of the lagged dense inverse (tests/ldi_restatement.py) checked on its own, without a GPU: the Ritz
values of a CG's coefficients against the spectrum of the operator it ran on, the Newton-Schulz iteration against numpy's
inverse, the input generators of tests/test_gpu_ldi_kernels.py against the bounds that file states -- and that the stand-alone
product tap refuses the shapes its kernel does not take before it looks for a device."""
import numpy as np
import pytest

import ldi_restatement as lr


@pytest.mark.parametrize('cond', [2.5, 50.0, 1e4])
def test_ritz_values_of_a_converged_cg_are_the_operators_extremal_eigenvalues(cond):
    """Preconditioned CG (M = D, a random positive diagonal) run to 1e-13 on A = D^1/2 B D^1/2 with B of 12 distinct
    eigenvalues: the Lanczos matrix of its coefficients is D^-1/2 A D^-1/2 = B projected on the Krylov space, CG converges
    when that space holds all 12 eigenvectors' directions, and then the eigenvalues of T ARE the 12 eigenvalues -- the
    extremal ones to 1e-8 relative, inside [lambda_min, lambda_max] to rounding (interlacing)."""
    B = lr.spd(200, cond, seed=int(cond), distinct=12)
    dh = np.sqrt(np.random.default_rng(5).uniform(0.5, 20.0, 200))
    A = B * dh[:, None] * dh[None, :]
    b = np.random.default_rng(1).standard_normal(200)
    rz, al = lr.cg_coefficients(A, b, 400, minv=lambda r: r / dh ** 2, tol=1e-13)
    m = len(al)
    assert 12 <= m <= 40                                     # (12 in exact arithmetic; rounding costs the ill-conditioned case some more)
    c, lmin, lmax, lo, hi = lr.ritz(rz, al, m, cap=m)
    w = np.linalg.eigvalsh(A / dh[:, None] / dh[None, :])
    print('cond %g: m %d  ritz %.12g %.12g  operator %.12g %.12g' % (cond, m, lmin, lmax, w[0], w[-1]))
    assert w[0] * (1 - 1e-10) <= lmin and lmax <= w[-1] * (1 + 1e-10)
    assert abs(lmin - w[0]) <= 1e-8 * w[0] and abs(lmax - w[-1]) <= 1e-8 * w[-1]
    assert lo <= lmin and lmax <= hi and abs(c - 1.9 / (w[0] + w[-1])) <= 2e-8 * c


def test_ritz_restatement_declines_what_the_kernel_declines():
    assert lr.ritz([1.0], [0.5], 1) == (0.0,) * 5
    assert lr.ritz([1.0, 0.5, 0.1], [0.5, -0.2, 0.3], 3) == (0.0,) * 5
    assert lr.ritz([1.0, 0.0, 0.1], [0.5, 0.2, 0.3], 3) == (0.0,) * 5
    # the first 64 iterations only
    A = lr.spd(200, 1e4, seed=3)
    rz, al = lr.cg_coefficients(A, np.ones(200), 70)
    assert lr.ritz(rz, al, 70) == lr.ritz(rz, al, 64)


@pytest.mark.parametrize('nr,d,bw,k', [(29, 6, 2, 12), (40, 3, 1, 0)])
def test_newton_schulz_contracts_at_every_step_and_ends_at_the_inverse(nr, d, bw, k):
    """From X_0 = c M_0 with eig(c M_0 S^) inside (0, 1.9): ||I - S^ X||_F falls at every step (the residual squares) until it
    reaches rounding, and X ends at inv(S^); the unscaled X_u is then inv(S)."""
    rp, ci, vals, Linv, S = lr.block_banded_spd(nr, d, bw, seed_=nr)
    n, npad = nr * d, lr.pad_of(nr * d)
    Sh, pat, _ = lr.scaled_dense(rp, ci, vals, Linv, npad)
    assert np.allclose(Sh[:n, :n], Sh[:n, :n].T, atol=1e-13) and np.array_equal(Sh[n:, n:], np.eye(npad - n))
    assert not Sh[~pat & ~np.pad(np.zeros((n, n), bool), (0, npad - n), constant_values=True)].any()
    Xt = np.zeros((npad, 16))
    Xt[:n, :k] = 0.3 * np.random.default_rng(2).standard_normal((n, k))
    M0 = np.eye(npad) + Xt @ Xt.T
    ev = np.linalg.eigvals(M0 @ Sh).real
    c = 1.9 / (ev.min() + ev.max())
    assert 0 < c * ev.min() and c * ev.max() < 1.9
    X, fro = lr.seed(Xt, c), []
    for _ in range(40):
        X, f, _ = lr.ns_step(Sh, X)
        fro.append(np.sqrt(f))
        if fro[-1] < 1e-12:
            break
    print('||I - S^ X||_F per step:', ' '.join('%.2e' % f for f in fro))
    assert fro[-1] < 1e-12 and all(b < a for a, b in zip(fro, fro[1:]))
    assert np.abs(X - np.linalg.inv(Sh)).max() <= 1e-11 * np.abs(X).max()
    Xu, _ = lr.unscale(X, Linv, npad)
    ref = np.linalg.inv(S)
    assert np.abs(Xu[:n, :n] - ref).max() <= 1e-10 * np.abs(ref).max()
    assert not Xu[n:].any() and not Xu[:, n:].any()
    # the float32 variant follows the float64 one to float32 rounding of an iteration that corrects itself
    X32, _, _ = lr.seeded_inverse(Sh.astype(np.float32), Xt.astype(np.float32), np.float32(c), len(fro), np.float32)
    assert X32.dtype == np.float32 and np.abs(X32 - X).max() <= 1e-4 * np.abs(X).max()


def test_product_restatement_masks_ranges_and_lower_tiles():
    M = N = 64; K = 48
    A, B, C0 = lr.normal32((M, K), 1), lr.normal32((K, N), 2), np.full((M, N), 7.0, dtype=np.float32)
    kr = [(16, 32), (0, 16)]
    C, bound = lr.gemm(A, B, M, N, K, alpha=-1.0, gamma=1.0, krange=kr, upper_only=True, C0=C0)
    ref = -(A[:32, 16:32].astype(float) @ B[16:32, :32].astype(float)) + np.eye(32)
    assert np.allclose(C[:32, :32], ref, rtol=0, atol=1e-14)
    assert np.all(C[32:, :32] == 7.0) and not bound[32:, :32].any() and np.all(bound[:32] > 0)
    # the float32 product numpy forms itself is inside the stated bound (it is a bound for any summation order)
    C, bound = lr.gemm(A, B, M, N, K, alpha=0.5, beta=1.0, Dm=C0, gamma=1.0)
    C32 = np.float32(0.5) * (A @ B) + C0 + np.eye(M, dtype=np.float32)
    assert np.all(np.abs(C32 - C) <= bound)


def test_generators_keep_the_reference_inside_the_stated_bounds():
    """The GPU test's inputs: the matrices have the condition numbers it names; every CG coefficient up to m = 70 is positive
    (so the kernel must answer); the bisection term of the Ritz bound stays below the fp32 term's order (the bound is decided by
    the output format, not by a wide bracket); a lost K chunk exceeds the product bound a thousandfold."""
    for cond in (2.5, 50.0, 1e4):
        A = lr.spd(200, cond, seed=int(cond))
        w = np.linalg.eigvalsh(A)
        assert abs(w[-1] / w[0] - cond) <= 1e-8 * cond
        rz, al = lr.cg_coefficients(A, np.random.default_rng(int(cond)).standard_normal(200), 70)
        assert len(al) == 70 and np.all(al > 0) and np.all(rz > 0) and np.all(np.isfinite(rz))
        for m in (2, 5, 33, 64, 70):
            c, lmin, lmax, lo, hi = lr.ritz(rz, al, m)
            bmin, bmax, bc = lr.ritz_bounds(lmin, lmax, lo, hi)
            assert w[0] * (1 - 1e-8) <= lmin <= lmax <= w[-1] * (1 + 1e-8) and lo <= lmin and lmax <= hi
            assert (hi - lo) * 65.0 ** -6 <= lr.U23 * lmin and bc <= 4 * lr.U23 * c
    M = N = 64
    for K in (16, 48, 64, 80, 144):
        A, B = lr.normal32((M, K), K), lr.normal32((K, N), K + 1)
        C, bound = lr.gemm(A, B, M, N, K)
        lost = A[:, :16].astype(float) @ B[:16].astype(float)
        assert np.median(np.abs(lost) / bound) > 1e3


def test_product_tap_refuses_bad_shapes_before_it_needs_a_device():
    from pyslam_amd import _native as nat
    from pyslam_amd.device import ldi_gemm
    z = np.zeros((64, 64), dtype=np.float32)
    for kw in (dict(M=48, N=64, K=64), dict(M=64, N=80, K=64), dict(M=64, N=64, K=24), dict(M=64, N=64, K=64, krange=[(8, 64), (0, 64)]),
               dict(M=64, N=64, K=64, krange=[(0, 40), (0, 64)]), dict(M=64, N=64, K=64, krange=[(0, 80), (0, 64)]),
               dict(M=64, N=64, K=64, lda=48), dict(M=64, N=64, K=64, beta=1.0)):
        with pytest.raises(nat.NativeError, match='ps_debug_ldi_gemm'):
            ldi_gemm(z, z, z, need_gpu=False, **kw)
