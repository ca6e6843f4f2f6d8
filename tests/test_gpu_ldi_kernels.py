"""GPU: every kernel of the lagged dense inverse (csrc/ps_k_ldi.h) against the float64 restatement of the same operation
(tests/ldi_restatement.py), through the taps ps_debug_ldi_gemm / ps_debug_ldi_ritz / ps_debug_ldi_read.  The inverse only
PRECONDITIONS -- tests/test_gpu_ldi.py cannot see a wrong one -- so here its numbers are held themselves: the fp32 MFMA
product at the K splits, grids, ranges and modes the Newton-Schulz steps use; the Sturm multisection; and, on live problems,
the scaled matrix, the seed, the Newton-Schulz result, the unscaled inverse, its quality, and z = X_u r.

Every bound is derived (rounding of the formats, the reference's own float32 error), none is fitted to the kernels; each case
prints its figure before it asserts.  Measured on an MI355X (seed in place, `X32` against the float64 restatement):
    30 keyframes (np = 192):  e32 = max|X_np32 - X_f64| = 6.12e-06,  max|X_dev - X_f64| = 1.23e-05   (bound 4 e32 + 2^-23 max|X| = 2.50e-05)
    60 keyframes (np = 384):  e32 = 2.41e-05,  max|X_dev - X_f64| = 3.46e-05   (bound 9.75e-05)
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ldi_restatement as lr

pytestmark = pytest.mark.gpu

U23, U24, U52 = lr.U23, lr.U24, lr.U52
C_SENTINEL, F_SENTINEL = np.float32(123.25), -7.0


# ---------------------------------------------------------------------------------------------------------------------
# k_ldi_gemm
# ---------------------------------------------------------------------------------------------------------------------
def run_gemm(M, N, K, alpha=1.0, beta=0.0, gamma=0.0, lda=None, ldb=None, ldc=None, dm=None, krange=None, upper_only=False,
             dev_scale=None, zero_outside=False, seed=0):
    """One product on the device and its restatement.  dm: None, 'own' (a matrix of its own) or 'A' (the very array A).
    -> dict with the device's C and fro parts, the float64 reference, the per-entry bound, and the inputs."""
    from pyslam_amd.device import ldi_gemm
    lda, ldb, ldc = lda or K, ldb or N, ldc or N
    A, B = lr.normal32((M, lda), 1000 + seed), lr.normal32((K, ldb), 2000 + seed)
    if zero_outside:
        A[:, :K] *= lr.krange_mask(M, K, krange).astype(np.float32)
    Dm = {None: None, 'own': lr.normal32((M, N), 3000 + seed), 'A': A}[dm]
    C0 = np.full((M, ldc), C_SENTINEL, dtype=np.float32)
    Cd, fro = ldi_gemm(A, B, C0, M, N, K, alpha=alpha, beta=beta, Dm=Dm, gamma=gamma, lda=lda, ldb=ldb, ldc=ldc,
                       ldd=None if Dm is None else Dm.shape[1], krange=krange, upper_only=upper_only, dev_scale=dev_scale,
                       fro_sentinel=F_SENTINEL)
    Cref, bound = lr.gemm(A, B, M, N, K, alpha=alpha, beta=beta, Dm=Dm, gamma=gamma, krange=krange, upper_only=upper_only, C0=C0,
                          scale=dev_scale)
    return dict(A=A, B=B, C0=C0, C=Cd, fro=fro, ref=Cref, bound=bound, M=M, N=N, K=K)


def check_gemm(name, r, upper_only=False):
    M, N = r['M'], r['N']
    Cd = r['C'].astype(np.float64)
    err = np.abs(Cd[:, :N] - r['ref'])
    low = lr.lower_tiles(M, N) if upper_only else np.zeros((M, N), dtype=bool)
    ratio = (err[~low] / r['bound'][~low]).max()
    print('%s: max |C - C_ref| = %.3e, worst entry at %.3f of its bound' % (name, err.max(), ratio))
    assert np.all(err[~low] <= r['bound'][~low]), name
    # what the kernel must not touch: columns beyond N of every row, and with upper_only the tiles below the diagonal (bit for bit)
    assert np.array_equal(r['C'][:, N:].view(np.uint32), r['C0'][:, N:].view(np.uint32)), name
    assert np.array_equal(r['C'][:, :N][low].view(np.uint32), r['C0'][:, :N][low].view(np.uint32)), name
    # Frobenius parts: the float64 sum of squares of the very numbers that came back, tile by tile; untouched tiles keep the sentinel
    worst = 0.0
    for ti in range(M // 32):
        for tj in range(N // 32):
            if upper_only and tj < ti:
                assert r['fro'][ti, tj] == F_SENTINEL, (name, ti, tj)
                continue
            want = (Cd[ti * 32:(ti + 1) * 32, tj * 32:(tj + 1) * 32] ** 2).sum()
            worst = max(worst, abs(r['fro'][ti, tj] - want) / want)
            assert abs(r['fro'][ti, tj] - want) <= 32 * 32 * U52 * want, (name, ti, tj)
    print('%s: fro parts to %.2e relative' % (name, worst))


GEMM_CASES = {
    # M = N = 64: one chunk (three idle waves), one idle wave, one chunk each, wave 0 twice (the buffer flips), a buffer reused
    'K16': dict(M=64, N=64, K=16), 'K48': dict(M=64, N=64, K=48), 'K64': dict(M=64, N=64, K=64), 'K80': dict(M=64, N=64, K=80),
    'K144': dict(M=64, N=64, K=144),
    'grid_96x64': dict(M=96, N=64, K=80), 'grid_64x128': dict(M=64, N=128, K=48),
    # the seed product's shape X~ X~^T: lda = K, ldb = N, K < N; with gamma and the device-side scale as the seed has them
    'seed_shape': dict(M=128, N=128, K=16, gamma=1.0, dev_scale=0.37),
    'padded_lds': dict(M=64, N=64, K=48, lda=80, ldb=96, ldc=72, dm='own', beta=-0.5),
    'dm_alias_A': dict(M=64, N=64, K=64, beta=1.0, dm='A'),
    'gamma': dict(M=64, N=96, K=32, alpha=-1.0, gamma=1.0),
    # dev_scale multiplies alpha and gamma and NOT beta
    'dev_scale': dict(M=64, N=64, K=80, alpha=1.5, beta=1.0, dm='own', gamma=1.0, dev_scale=0.37),
}


@pytest.mark.parametrize('name', sorted(GEMM_CASES))
def test_gemm_against_float64(name):
    check_gemm(name, run_gemm(seed=sorted(GEMM_CASES).index(name), **GEMM_CASES[name]))


KR = [(16, 128), (0, 16), (48, 144), (32, 96)]            # per 32-row tile; k_lo > 0, k_hi < K, and the minimal [0, 16)


def test_gemm_k_ranges_equal_the_full_product_when_A_is_zero_outside():
    r = run_gemm(128, 64, 144, alpha=-1.0, gamma=1.0, krange=KR, zero_outside=True, seed=40)
    full, bound = lr.gemm(r['A'], r['B'], 128, 64, 144, alpha=-1.0, gamma=1.0)
    assert np.array_equal(full, r['ref'])                    # (the masked and the full restatement agree: A is zero outside)
    check_gemm('krange, A zero outside', r)


def test_gemm_k_ranges_are_honoured_not_merely_harmless():
    """A is NOT zero outside the ranges: the kernel must give the masked product, and the full one differs by O(1)."""
    r = run_gemm(128, 64, 144, alpha=-1.0, gamma=1.0, krange=KR, zero_outside=False, seed=41)
    check_gemm('krange, A non-zero outside', r)
    full, _ = lr.gemm(r['A'], r['B'], 128, 64, 144, alpha=-1.0, gamma=1.0)
    assert np.median(np.abs(full - r['ref'])) > 1.0


def test_gemm_upper_only_leaves_the_lower_tiles_and_their_fro_slots_alone():
    """T = X + X R as ldi_ns_step launches it: Dm aliases A, upper triangle of tiles only."""
    check_gemm('upper_only', run_gemm(96, 96, 96, beta=1.0, dm='A', upper_only=True, seed=50), upper_only=True)


def test_gemm_is_deterministic():
    a = run_gemm(96, 64, 144, alpha=-1.0, gamma=1.0, seed=60)
    b = run_gemm(96, 64, 144, alpha=-1.0, gamma=1.0, seed=60)
    assert np.array_equal(a['C'].view(np.uint32), b['C'].view(np.uint32)) and np.array_equal(a['fro'], b['fro'])


# ---------------------------------------------------------------------------------------------------------------------
# k_ldi_ritz
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cg_run(cond):
    A = lr.spd(200, cond, seed=int(cond))
    return lr.cg_coefficients(A, np.random.default_rng(int(cond)).standard_normal(200), 70)


@pytest.mark.parametrize('m', [2, 5, 33, 64, 70])
@pytest.mark.parametrize('cond', [2.5, 50.0, 1e4])
def test_ritz_values_against_eigvalsh(cond, m):
    from pyslam_amd.device import ldi_ritz
    rz, al = cg_run(cond)
    out = ldi_ritz(rz, al, m).astype(np.float64)
    c, lmin, lmax, lo, hi = lr.ritz(rz, al, m)                # (m = 70: the first 64)
    bmin, bmax, bc = lr.ritz_bounds(lmin, lmax, lo, hi)
    print('cond %g m %d: ritz %.9g %.9g (ref %.9g %.9g), errors %.2e %.2e of bounds %.2e %.2e; c %.9g err %.2e bound %.2e'
          % (cond, m, out[1], out[2], lmin, lmax, abs(out[1] - lmin), abs(out[2] - lmax), bmin, bmax, out[0], abs(out[0] - c), bc))
    assert abs(out[1] - lmin) <= bmin and abs(out[2] - lmax) <= bmax
    assert abs(out[0] - c) <= bc


def test_ritz_declines_without_a_usable_estimate():
    from pyslam_amd.device import ldi_ritz
    rz, al = cg_run(50.0)
    assert np.array_equal(ldi_ritz(rz, al, 1), np.zeros(3, dtype=np.float32))
    assert np.array_equal(ldi_ritz(rz, al, 0), np.zeros(3, dtype=np.float32))
    bad = al.copy(); bad[3] = -bad[3]
    assert np.array_equal(ldi_ritz(rz, bad, 10), np.zeros(3, dtype=np.float32))
    bad = al.copy(); bad[0] = 0.0
    assert np.array_equal(ldi_ritz(rz, bad, 10), np.zeros(3, dtype=np.float32))
    bad = rz.copy(); bad[2] = 0.0
    assert np.array_equal(ldi_ritz(bad, al, 10), np.zeros(3, dtype=np.float32))
    bad = rz.copy(); bad[9] = -1e-3
    assert np.array_equal(ldi_ritz(bad, al, 10), np.zeros(3, dtype=np.float32))
    assert ldi_ritz(rz, al, 10)[0] > 0                        # (the same coefficients, untouched, do give an estimate)


# ---------------------------------------------------------------------------------------------------------------------
# the inverse of a live problem
# ---------------------------------------------------------------------------------------------------------------------
def solves(dev):
    from pyslam_amd import _native as nat
    i = nat.ProblemInfo()
    nat.check(dev._lib.ps_get_info(dev._h, C.byref(i)))
    return i.ldi_solves


def settle(lp, tol, max_iters, calls=12):
    """The repeated-linearisation-point pattern of test_gpu_ldi.py::test_repeated_linearisation_point with refreshes off: the
    same point again and again until a call has SOLVED with the inverse.  -> (dev, state record, CG iterations per call)."""
    from pyslam_amd import _native as nat
    from pyslam_amd.device import DeviceProblem
    dev = DeviceProblem(lp)
    dev.set_option('lagged_inverse', 1)
    dev.set_option('ldi_refresh_its', 64)
    dev.eval_cost(True)
    with pytest.raises(nat.NativeError):                      # never set up: an error, not garbage
        dev.debug_ldi_read('Xu')
    dev.snapshot()
    its = []
    for _ in range(calls):
        dev.restore()
        before = solves(dev)
        its.append(dev.gn_iteration(0., tol, max_iters, True)[2])
        s = dev.debug_ldi_state()
        if s['state'] in (2, 3) and s['cur'] >= 0 and solves(dev) > before:
            assert dev.debug_ldi_state() == s and solves(dev) == before + 1      # (reading moves nothing)
            return dev, s, its
    raise AssertionError('the inverse never came into use: its %s, state %s' % (its, s))


def ba(kf, lm):
    from pyslam_amd import synthetic
    return synthetic.stereo_ba(num_kf=kf, num_lm=lm, obs_per_lm=6, half_window=8, seed=kf)[0]


def check_product(dev, s):
    """z = X_u r of the last k_ldi_init / k_ldi_update, row by row."""
    n, npad = s['n'], s['np']
    Xu, r, z = dev.debug_ldi_read('Xu')[:n, :n], dev.debug_ldi_read('r'), dev.debug_ldi_read('z')
    ref, bound = lr.matvec(Xu, r, npad)
    ratio = (np.abs(z - ref) / bound).max()
    print('z = X_u r (n = %d, %d iterations): max |z - ref| = %.3e, worst row at %.3f of its bound' % (n, s['last_its'], np.abs(z - ref).max(), ratio))
    assert np.linalg.norm(r) > 0 and np.all(np.abs(z - ref) <= bound)


def check_symmetry(name, Xu):
    asym = np.abs(Xu - Xu.T)
    print('%s: max |Xu - Xu^T| / |Xu| = %.3e' % (name, (asym[Xu != 0] / np.abs(Xu[Xu != 0])).max() if asym.any() else 0.0))
    assert np.all(asym <= U23 * np.abs(Xu))


@pytest.fixture(scope='module', params=[(30, 1500, 174, 192), (60, 6000, 354, 384)], ids=['kf30', 'kf60'])
def seeded(request):
    """A settled stereo-BA problem, everything tapped once, and the restatements computed once (read-only for the tests)."""
    kf, lm, n, npad = request.param
    dev, s, its = settle(ba(kf, lm), 1e-12, 500)
    print('kf %d: CG iterations per call %s' % (kf, its))
    assert (s['n'], s['np'], s['direct']) == (n, npad, 0) and npad - n >= 18
    t = {k: dev.debug_ldi_read(k) for k in ('S32', 'X32', 'Xu', 'Xt', 'Linv', 'coef', 'fro')}
    rp, ci, vals, _ = dev.reduced_system()
    Sdense, _ = dev.reduced_dense()
    steps = s['seed_steps']
    X64, fro64, R64 = lr.seeded_inverse(t['S32'], t['Xt'], t['coef'][0], steps)
    X32, fro32, _ = lr.seeded_inverse(t['S32'], t['Xt'], t['coef'][0], steps, np.float32)
    Xprev64, _, _ = lr.seeded_inverse(t['S32'], t['Xt'], t['coef'][0], steps - 1)
    Xprev32, _, _ = lr.seeded_inverse(t['S32'], t['Xt'], t['coef'][0], steps - 1, np.float32)
    yield dict(dev=dev, s=s, t=t, bsr=(rp, ci, vals), S=Sdense, X64=X64, X32=X32.astype(np.float64), fro64=fro64, fro32=fro32, R64=R64,
               Xprev64=Xprev64, Xprev32=Xprev32.astype(np.float64), its=its)
    dev.close()


def test_scaled_matrix_in_place(seeded):
    """S32 = float32(L^-1 S L^-T) block by block: one fp32 rounding of an fp64 triple product (whose own rounding, 2 D terms
    of 2^-53 on |L^-1||S||L^-T|, is the slack beside it); exactly zero outside the blocks, exactly the identity on the padding."""
    s, t = seeded['s'], seeded['t']
    n, npad, d = s['n'], s['np'], s['dof']
    ref, pat, mag = lr.scaled_dense(*seeded['bsr'], t['Linv'], npad)
    err, bound = np.abs(t['S32'] - ref), U24 * np.abs(ref) + 4 * d * 2.0 ** -53 * mag
    print('S32: max |S32 - ref| = %.3e, worst entry at %.3f of its bound' % (err.max(), (err[pat] / bound[pat]).max()))
    assert np.all(err[pat] <= bound[pat])
    outside = ~pat
    outside[n:, n:] = False
    assert not t['S32'][outside].any()
    assert np.array_equal(t['S32'][n:, n:], np.eye(npad - n))


def test_seed_scale_in_place(seeded):
    c, lmin, lmax = seeded['t']['coef']
    print('coef: c %.9g ritz %.9g %.9g' % (c, lmin, lmax))
    assert 0 < lmin <= lmax and abs(c - 1.9 / (lmin + lmax)) <= U23 * c


def test_newton_schulz_result_in_place(seeded):
    """X32 after the seed and its Newton-Schulz steps against the float64 restatement from the tapped X~, c and S32:
    max|X_dev - X_f64| <= 4 e32 + 2^-23 max|X| with e32 = max|X_np32 - X_f64| the error of numpy's own float32 restatement
    (4: another summation order in the K split).  Measured: np = 192: e32 6.12e-06, device 1.23e-05; np = 384: e32 2.41e-05,
    device 3.46e-05.  Exactly symmetric; the padding block is diagonal."""
    s, X = seeded['s'], seeded['t']['X32']
    n = s['n']
    e32 = np.abs(seeded['X32'] - seeded['X64']).max()
    edev = np.abs(X - seeded['X64']).max()
    bound = 4 * e32 + U23 * np.abs(seeded['X64']).max()
    print('X32 (np = %d, %d steps): e32 = %.3e, max|X_dev - X_f64| = %.3e, bound %.3e' % (s['np'], s['seed_steps'], e32, edev, bound))
    assert edev <= bound
    assert np.array_equal(X, X.T)
    pad = X[n:, n:]
    assert np.array_equal(pad, np.diag(np.diag(pad))) and np.all(np.diag(pad) > 0)
    assert not X[:n, n:].any()


def test_frobenius_word_in_place(seeded):
    """||I - S32 X||_F^2 of the last step, as e32 for X: with efro32 = |fro_np32 - fro_f64| the error of numpy's own float32
    restatement of the same word, |fro_dev - fro_f64| <= 4 efro32 + 2^-23 fro.  Measured: np = 192: efro32 4.2e-07, device
    5.1e-07 (bound 1.7e-06); np = 384: efro32 6.7e-06, device 1.3e-06 (bound 2.7e-05); one lost tile of R would be 1e-2 relative.
    Printed beside it, the worst case no summation order can exceed: the device forms R from ITS X of the step before (within
    tol = 4 e32 + 2^-23 max|X| of the float64 one, e32 measured at that step) by the fp32 product, so per entry
    |dR_ij| <= (|S32| 1)_i tol + the product's rounding bound and d(fro) <= 2 sum |R| |dR| + sum dR^2."""
    s, t = seeded['s'], seeded['t']
    npad = s['np']
    tol = 4 * np.abs(seeded['Xprev32'] - seeded['Xprev64']).max() + U23 * np.abs(seeded['Xprev64']).max()
    _, gb = lr.gemm(t['S32'], seeded['Xprev64'], npad, npad, npad, alpha=-1.0, gamma=1.0)
    dR = np.abs(t['S32']).sum(1)[:, None] * tol + gb
    R = np.abs(seeded['R64'])
    worst_case = 2 * (R * dR).sum() + (dR ** 2).sum()
    fro64, fro32, fro = seeded['fro64'][-1], seeded['fro32'][-1], t['fro'][0]
    bound = 4 * abs(fro32 - fro64) + U23 * fro64
    print('fro (np = %d): device %.9e, float64 %.9e, numpy float32 %.9e; efro32 = %.3e, |dev - f64| = %.3e, bound %.3e '
          '(worst case %.3e; rms %.4f)' % (npad, fro, fro64, fro32, abs(fro32 - fro64), abs(fro - fro64), bound, worst_case, np.sqrt(fro / npad)))
    assert abs(fro - fro64) <= bound
    assert np.sqrt(fro / npad) < s['fro_limit']                # what ldi_decide accepted it under


def test_unscaled_inverse_in_place(seeded):
    """Xu = float32(L^-T X32 L^-1) block by block from the tapped X32 and factors (one fp32 rounding of an fp64 triple
    product); zero on the padding; symmetric to one fp32 unit per entry (the two triangles are computed separately)."""
    s, t = seeded['s'], seeded['t']
    n, npad, d = s['n'], s['np'], s['dof']
    ref, mag = lr.unscale(t['X32'], t['Linv'], npad)
    err, bound = np.abs(t['Xu'] - ref), U24 * np.abs(ref) + 4 * d * 2.0 ** -53 * mag
    print('Xu: max |Xu - ref| = %.3e, worst entry at %.3f of its bound' % (err.max(), (err[:n, :n] / bound[:n, :n]).max()))
    assert np.all(err[:n, :n] <= bound[:n, :n])
    assert not t['Xu'][n:].any() and not t['Xu'][:, n:].any()
    check_symmetry('Xu', t['Xu'])


def test_quality_of_the_inverse_in_place(seeded):
    """The claim behind the README's iteration counts: the rms eigenvalue of I - S X_u (float64, from the tapped X_u and the
    current S; the eigenvalues are those of the symmetric I - C^T X_u C, S = C C^T) is below the limit the host accepted the
    inverse under."""
    s, n = seeded['s'], seeded['s']['n']
    Cf = np.linalg.cholesky(seeded['S'])
    lam = np.linalg.eigvalsh(np.eye(n) - Cf.T @ seeded['t']['Xu'][:n, :n] @ Cf)
    rms = np.sqrt((lam ** 2).mean())
    print('quality (n = %d): rms eigenvalue of I - S Xu = %.3e, extremes %.3e %.3e; limit %.2f; CG iterations per call %s'
          % (n, rms, lam.min(), lam.max(), s['fro_limit'], seeded['its']))
    assert rms < s['fro_limit']


def test_preconditioner_product_in_place(seeded):
    check_product(seeded['dev'], seeded['s'])


def test_preconditioner_product_beyond_one_piece_per_lane():
    """n = 1 074 > 4 * 256: more than one float4 piece of a row per lane is live (z only)."""
    dev, s, its = settle(ba(180, 4000), 1e-12, 500)
    assert s['n'] > 1024
    check_product(dev, s)
    dev.close()


@pytest.mark.parametrize('poses,dof,npad', [(100, 3, 320), (40, 6, 256)])
def test_direct_seed_is_the_inverse(poses, dof, npad):
    """Pose graphs: X_u = S^-1 from the fp64 factorisation, stored in fp32: 2^-23 max|S^-1| for the storage and
    cond(S) 2^-52 max|S^-1| for the factorisation; exactly zero on the padding; symmetric to one fp32 unit."""
    from pyslam_amd import synthetic
    lp, _ = synthetic.pose_graph(num_poses=poses, dof=dof)
    dev, s, its = settle(lp, 1e-13, 2000)
    n = s['n']
    assert (s['np'], s['direct']) == (npad, 1) and npad > n
    Xu = dev.debug_ldi_read('Xu')
    S, _ = dev.reduced_dense()
    ref, cond = lr.inverse(S)
    err, bound = np.abs(Xu[:n, :n] - ref).max(), (U23 + cond * U52) * np.abs(ref).max()
    print('direct seed (n = %d, cond %.3e): max |Xu - inv(S)| = %.3e, bound %.3e; CG iterations per call %s' % (n, cond, err, bound, its))
    assert err <= bound
    assert not Xu[n:].any() and not Xu[:, n:].any()
    check_symmetry('direct Xu', Xu)
    check_product(dev, s)
    dev.close()
