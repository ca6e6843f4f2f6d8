"""Plain numpy restatement of the lagged dense inverse (csrc/ps_k_ldi.h, ps_host_ldi.h): what every kernel of it computes,
in float64 (the Newton-Schulz part also in float32), and the input generators of tests/test_gpu_ldi_kernels.py.
Checked on its own by tests/test_ldi_restatement_host.py."""
import numpy as np

U24, U23, U52 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -52
TILE, CHUNK = 32, 16


# ---- the product C = alpha A B + beta Dm + gamma I --------------------------------------------------------------------
def krange_mask(M, K, krange):
    """(M, K) 0 / 1: the columns of A that row tile i // 32 walks."""
    mask = np.ones((M, K))
    if krange is not None:
        mask[:] = 0.0
        for t, (lo, hi) in enumerate(np.asarray(krange).reshape(-1, 2)):
            mask[t * TILE:(t + 1) * TILE, lo:hi] = 1.0
    return mask


def lower_tiles(M, N):
    """(M, N) bool: entries of tiles strictly below the diagonal (what upper_only leaves untouched)."""
    ti, tj = np.arange(M)[:, None] // TILE, np.arange(N)[None, :] // TILE
    return tj < ti


def gemm(A, B, M, N, K, alpha=1.0, beta=0.0, Dm=None, gamma=0.0, krange=None, upper_only=False, C0=None, scale=None):
    """-> (C, bound) in float64.  bound: the per-entry rounding bound of an fp32 product with fp32 accumulation in any order,
         K 2^-24 |alpha| (|A||B|)_ij + 2^-23 (|alpha (AB)_ij| + |beta Dm_ij| + |gamma|)
    (K - 1 additions and one rounding per product: at most K 2^-24 relative to |A||B| to first order; then alpha times the sum,
    plus beta Dm, plus gamma: one rounding each, every intermediate at most the sum of the three magnitudes).  Entries that
    upper_only leaves alone take C0's value and bound 0.  scale: what dev_scale holds (multiplies alpha and gamma)."""
    A64, B64 = np.asarray(A, dtype=np.float64)[:M, :K], np.asarray(B, dtype=np.float64)[:K, :N]
    if scale is not None:
        s = float(np.float32(scale))
        alpha, gamma = float(np.float32(np.float32(alpha) * np.float32(s))), float(np.float32(np.float32(gamma) * np.float32(s)))
    Am = A64 * krange_mask(M, K, krange)
    P, Pabs = Am @ B64, np.abs(Am) @ np.abs(B64)
    D = np.zeros((M, N)) if Dm is None or beta == 0.0 else np.asarray(Dm, dtype=np.float64)[:M, :N]
    eye = np.eye(M, N)
    Cref = alpha * P + beta * D + gamma * eye
    bound = K * U24 * abs(alpha) * Pabs + U23 * (np.abs(alpha * P) + np.abs(beta * D) + abs(gamma) * eye)
    if upper_only:
        low = lower_tiles(M, N)
        Cref[low] = np.asarray(C0, dtype=np.float64)[:M, :N][low]
        bound[low] = 0.0
    return Cref, bound


def normal32(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


# ---- the seed scale: Lanczos matrix of a CG's coefficients, extremal Ritz values ------------------------------------------
def spd(n, cond, seed, distinct=None):
    """Symmetric positive definite, order n, eigenvalues spread geometrically over [1, cond] (`distinct` values, repeated, if given)."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    w = np.geomspace(1.0, cond, n) if distinct is None else np.geomspace(1.0, cond, distinct)[np.arange(n) % distinct]
    A = (Q * w) @ Q.T
    return 0.5 * (A + A.T)


def cg_coefficients(A, b, iters, minv=None, tol=0.0):
    """Preconditioned CG on A x = b from x = 0: -> (rz, alpha) with rz[k] = r_k . z_k and alpha[k] = rz[k] / p_k . A p_k, as the
    solver's CG leaves them in hist[k] and hist[cap + k].  Stops after `iters` iterations or once rz <= tol^2 rz[0]."""
    minv = (lambda r: r) if minv is None else minv
    x, r = np.zeros_like(b), b.copy()
    z = minv(r)
    p = z.copy()
    rz = [float(r @ z)]
    al = []
    for k in range(iters):
        q = A @ p
        a = rz[k] / float(p @ q)
        al.append(a)
        x += a * p
        r -= a * q
        z = minv(r)
        rz.append(float(r @ z))
        if k + 1 == iters or not rz[k + 1] > tol * tol * rz[0]:
            break
        p = z + (rz[k + 1] / rz[k]) * p
    m = len(al)
    return np.array(rz[:m]), np.array(al)


def lanczos(rz, alpha, m):
    """Diagonal and off-diagonal of T_m: T_kk = 1 / alpha_k + beta_{k-1} / alpha_{k-1}, T_k,k+1 = sqrt(beta_k) / alpha_k,
    beta_k = rz[k+1] / rz[k]."""
    rz, alpha = np.asarray(rz, dtype=np.float64), np.asarray(alpha, dtype=np.float64)
    d, e = np.zeros(m), np.zeros(max(m - 1, 0))
    for k in range(m):
        d[k] = 1.0 / alpha[k] + ((rz[k] / rz[k - 1]) / alpha[k - 1] if k > 0 else 0.0)
        if k + 1 < m:
            e[k] = np.sqrt(rz[k + 1] / rz[k]) / alpha[k]
    return d, e


def ritz(rz, alpha, m, cap=64):
    """-> (c, ritz_min, ritz_max, lo, hi): c = 1.9 / (ritz_min + ritz_max) from the first min(m, cap) iterations, [lo, hi] the
    Gershgorin bracket of T.  All zero when m < 2 or a coefficient is not positive."""
    m = min(m, cap)
    if m < 2 or not (np.all(np.asarray(alpha[:m]) > 0) and np.all(np.asarray(rz[:m]) > 0)):
        return 0.0, 0.0, 0.0, 0.0, 0.0
    d, e = lanczos(rz, alpha, m)
    T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    w = np.linalg.eigvalsh(T)
    rad = np.abs(T).sum(1) - np.abs(d)
    return 1.9 / (w[0] + w[-1]), w[0], w[-1], float((d - rad).min()), float((d + rad).max())


def ritz_bounds(lmin, lmax, lo, hi):
    """Six 65-fold multisections of the Gershgorin bracket and one fp32 rounding: bound of each Ritz value, and of c by first-order
    propagation through 1.9 / (lmin + lmax) plus its own rounding."""
    sect = (hi - lo) * 65.0 ** -6
    bmin, bmax = sect + U23 * abs(lmin), sect + U23 * abs(lmax)
    c = 1.9 / (lmin + lmax)
    return bmin, bmax, c * (2 * sect) / (lmin + lmax - 2 * sect) + U23 * c


# ---- scaling, seed, Newton-Schulz, unscaling ---------------------------------------------------------------------------------
def pad_of(n):
    return (n + 63) // 64 * 64


def scaled_dense(row_ptr, col_idx, vals, Linv, npad):
    """S^ = L^-1 S L^-T block by block (S^_ij = Linv_i S_ij Linv_j^T) in an npad x npad matrix with identity padding; also the
    0 / 1 pattern of the blocks and |Linv_i| |S_ij| |Linv_j|^T (the magnitude its rounding scales with)."""
    nr, d = Linv.shape[0], Linv.shape[1]
    n = nr * d
    S = np.zeros((npad, npad))
    mag = np.zeros((npad, npad))
    pat = np.zeros((npad, npad), dtype=bool)
    for i in range(nr):
        for b in range(row_ptr[i], row_ptr[i + 1]):
            j = col_idx[b]
            sl = (slice(i * d, (i + 1) * d), slice(j * d, (j + 1) * d))
            S[sl] = Linv[i] @ vals[b] @ Linv[j].T
            mag[sl] = np.abs(Linv[i]) @ np.abs(vals[b]) @ np.abs(Linv[j]).T
            pat[sl] = True
    S[n:, n:] = np.eye(npad - n)
    return S, pat, mag


def seed(Xt, c, dtype=np.float64):
    """X_0 = c (I + X~ X~^T)."""
    Xt = np.asarray(Xt, dtype=dtype)
    c = dtype(c)
    return c * (Xt @ Xt.T) + c * np.eye(Xt.shape[0], dtype=dtype)


def ns_step(S, X, dtype=np.float64):
    """R = I - S^ X, T = X + X R, X <- sym(T).  -> (X, ||R||_F^2 in float64, R)."""
    S, X = np.asarray(S, dtype=dtype), np.asarray(X, dtype=dtype)
    R = np.eye(S.shape[0], dtype=dtype) - S @ X
    T = X + X @ R
    return dtype(0.5) * (T + T.T), float((R.astype(np.float64) ** 2).sum()), R


def seeded_inverse(S, Xt, c, steps, dtype=np.float64):
    """X_0 and `steps` Newton-Schulz steps.  -> (X, [||R||_F^2 of every step], the last step's R)."""
    X, fro, R = seed(Xt, c, dtype), [], None
    for _ in range(steps):
        X, f, R = ns_step(S, X, dtype)
        fro.append(f)
    return X, fro, R


def unscale(X, Linv, npad):
    """X_u = L^-T X L^-1 block by block (X_u,ij = Linv_i^T X_ij Linv_j), zero on the padding; and |Linv_i|^T |X_ij| |Linv_j|."""
    nr, d = Linv.shape[0], Linv.shape[1]
    n = nr * d
    # block-diagonal L^-1 once: the product over all blocks is two dense products
    Lb = np.zeros((n, n))
    for i in range(nr):
        Lb[i * d:(i + 1) * d, i * d:(i + 1) * d] = Linv[i]
    Xu, mag = np.zeros((npad, npad)), np.zeros((npad, npad))
    Xu[:n, :n] = Lb.T @ np.asarray(X, dtype=np.float64)[:n, :n] @ Lb
    mag[:n, :n] = np.abs(Lb).T @ np.abs(np.asarray(X, dtype=np.float64)[:n, :n]) @ np.abs(Lb)
    return Xu, mag


def matvec(Xu, r, npad):
    """z = X_u r in float64 and its bound for a float64 sum of npad products: npad 2^-52 (|X_u||r|)_i."""
    return Xu @ r, npad * U52 * (np.abs(Xu) @ np.abs(r))


def inverse(S):
    """-> (inv(S), cond(S)) by numpy."""
    return np.linalg.inv(S), np.linalg.cond(S)


def block_banded_spd(nr, d, bw, seed_):
    """A block-banded symmetric positive definite matrix in BSR form with its block-Jacobi factors: -> (row_ptr, col_idx, vals,
    Linv, dense S).  Linv_i = chol(S_ii)^-1, so S^ has identity diagonal blocks."""
    rng = np.random.default_rng(seed_)
    n = nr * d
    G = np.zeros((n, n))
    for i in range(nr):
        for j in range(max(0, i - bw), i + 1):
            G[i * d:(i + 1) * d, j * d:(j + 1) * d] = rng.standard_normal((d, d)) * (1.0 if i == j else 0.35)
    S = G @ G.T + 0.5 * np.eye(n)                              # band 2 bw in blocks
    row_ptr, col_idx, vals = [0], [], []
    for i in range(nr):
        for j in range(max(0, i - 2 * bw), min(nr, i + 2 * bw + 1)):
            col_idx.append(j); vals.append(S[i * d:(i + 1) * d, j * d:(j + 1) * d].copy())
        row_ptr.append(len(col_idx))
    Linv = np.stack([np.linalg.inv(np.linalg.cholesky(S[i * d:(i + 1) * d, i * d:(i + 1) * d])) for i in range(nr)])
    return np.array(row_ptr, dtype=np.int32), np.array(col_idx, dtype=np.int32), np.stack(vals), Linv, S
