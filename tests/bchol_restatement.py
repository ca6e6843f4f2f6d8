"""Plain numpy restatement of the blocked dense factorisation chain (csrc/ps_host_bchol.h; kernels csrc/ps_k_coarse.h
k_bchol_panel / k_bchol_update / k_btri_inverse / k_btri_merge / k_btri_clear, csrc/ps_k_xcg.h k_xcg_ainv): what every stage must
produce, in float64 by LAPACK (np.linalg.cholesky, scipy.linalg.solve_triangular) and once more in extended precision (the
"truth" that says how wrong LAPACK's own float64 chain is: the figure the device bounds are multiples of); the matrix families
and sizes of tests/test_gpu_bchol_kernels.py; and the panel's slab mapping, old and new.
Checked on its own by tests/test_bchol_host.py."""
import functools

import numpy as np
import scipy.linalg as sla

EPS = 2.0 ** -52
U24 = 2.0 ** -24
W = 24                    # PS_BC_W: columns per factorisation step, the diagonal tiles
S0 = 192                  # PS_BI_S0: diagonal blocks of the triangular inverse, doubled per merge level
SLAB = 1024               # PS_BC_SLAB: panel entries per workgroup at most
LD = np.longdouble

SIZES = (1, 4, 23, 24, 25, 48, 66, 67, 91, 191, 192, 193, 255, 257, 383, 384, 385, 500, 769, 800)
FAMILIES = ('gram', 'chain', 'scaled')

# The device bound on every figure below: MULT times the same figure of LAPACK's float64 chain, with a floor of n EPS.  The
# multiple pays for a different summation order only (blocked right-looking, 24 columns per step, merge levels; LAPACK's own
# blocking on the other side): DESIGN.md section 4 has the measured ratios.
MULT = 8.0


def bound(fig, n):
    return MULT * max(fig, n * EPS)


# ---- matrix families ---------------------------------------------------------------------------------------------------------
def gram(n, seed):
    """(a) a random Gram matrix plus n I: condition number ~5."""
    G = np.random.default_rng(seed).standard_normal((n, n))
    A = G.T @ G + n * np.eye(n)
    return 0.5 * (A + A.T)


def chain(n, seed):
    """(b) a coarse-level look-alike: block tridiagonal, 6 x 6 blocks, a 1-D chain of nodes tied to their neighbours by random
    well-conditioned 6 x 6 information matrices and anchored at node 0 by the identity; the leading n x n part of it (n need not
    be a multiple of 6).  Condition number ~ nodes^2."""
    rng = np.random.default_rng(seed)
    nodes = (n + 5) // 6 + 1
    A = np.zeros((6 * nodes, 6 * nodes))
    A[:6, :6] += np.eye(6)
    for k in range(nodes - 1):
        B = rng.standard_normal((6, 6))
        Wk = B @ B.T / 6.0 + np.eye(6)
        J = np.hstack([-np.eye(6), np.eye(6) + 0.05 * rng.standard_normal((6, 6))])
        A[6 * k:6 * k + 12, 6 * k:6 * k + 12] += J.T @ Wk @ J
    A = A[:n, :n]
    return 0.5 * (A + A.T)


def scaled(n, seed):
    """(c) family (a) scaled by diag(10^k) on both sides, k integers in -4 .. 4: entries spread over 16 decades, the condition
    number of the scaled matrix ~1e16 while the factorisation (invariant under such a scaling up to rounding) stays benign."""
    k = np.random.default_rng(seed + 1000).integers(-4, 5, n)
    d = 10.0 ** k
    A = gram(n, seed) * d[:, None] * d[None, :]
    return 0.5 * (A + A.T)


def family(name, n, seed=None):
    seed = n if seed is None else seed
    return {'gram': gram, 'chain': chain, 'scaled': scaled}[name](n, seed)


def conds(A):
    """(2-norm condition number, the same after scaling to a unit diagonal)."""
    d = 1.0 / np.sqrt(np.diag(A))
    return float(np.linalg.cond(A)), float(np.linalg.cond(A * d[:, None] * d[None, :]))


# ---- what the stages promise ------------------------------------------------------------------------------------------------
def below_tiles(n):
    """(n, n) bool: entries below the 24 x 24 diagonal tiles -- where the working matrix holds L."""
    i = np.arange(n)
    return (i[:, None] // W) > (i[None, :] // W)


def lower(n):
    return np.tril(np.ones((n, n), dtype=bool))


def same_block(n):
    """(n, n) bool: entries of the 192 x 192 diagonal blocks (k_btri_inverse writes them whole, zeros above the diagonal)."""
    i = np.arange(n)
    return (i[:, None] // S0) == (i[None, :] // S0)


def tiles_of(L, dtype=np.float64):
    """The diagonal tiles' inverses, (steps, 24, 24), lower triangular, zero-padded in a last partial tile."""
    n = L.shape[0]
    steps = (n + W - 1) // W
    out = np.zeros((steps, W, W), dtype=dtype)
    for s in range(steps):
        j0, w = s * W, min(W, n - s * W)
        T = L[j0:j0 + w, j0:j0 + w]
        out[s, :w, :w] = tri_inv_ld(T) if dtype is LD else sla.solve_triangular(T, np.eye(w), lower=True)
    return out


# ---- extended precision: the truth LAPACK's float64 chain is measured against ------------------------------------------------------
def chol_ld(A):
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        d = np.sqrt(v[0])
        L[j:, j] = v / d
        L[j, j] = d
    return L


def tri_inv_ld(L):
    L = np.asarray(L, dtype=LD)
    n = L.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for i in range(n):
        X[i, :i] = -(L[i, :i] @ X[:i, :i]) / L[i, i]
        X[i, i] = 1.0 / L[i, i]
    return X


def rel_f(X, T, mask=None):
    """||X - T||_F / ||T||_F over the masked entries, in the precision of T."""
    D = np.asarray(X, dtype=T.dtype) - T
    if mask is not None:
        D, T = D[mask], T[mask]
    den = np.sqrt((T * T).sum())
    return float(np.sqrt((D * D).sum()) / den) if den > 0 else float(np.sqrt((D * D).sum()))


def residual(Li, A):
    """||Li A Li^T - I||_max, evaluated in float64 (the same evaluation for LAPACK's chain and the device's)."""
    n = A.shape[0]
    As = np.tril(A) + np.tril(A, -1).T
    return float(np.abs(Li @ As @ Li.T - np.eye(n)).max())


class Reference:
    """LAPACK's float64 chain on A, the extended-precision truth, and LAPACK's own figures against it."""

    def __init__(self, A):
        n = A.shape[0]
        self.n, self.A = n, A
        self.L = np.linalg.cholesky(A)
        self.Tinv = tiles_of(self.L)
        self.Li = sla.solve_triangular(self.L, np.eye(n), lower=True)
        self.Ainv = self.Li.T @ self.Li
        Lt = chol_ld(A)
        Lit = tri_inv_ld(Lt)
        self.L_true, self.Li_true, self.Tinv_true = Lt, Lit, tiles_of(Lt, LD)
        # (the truth's product in float64 from the truth rounded once: its own error is of the order of the floor n EPS)
        Li64 = Lit.astype(np.float64)
        self.Ainv_true = Li64.T @ Li64
        self.fig = dict(
            L=rel_f(self.L, Lt, below_tiles(n)) if n > W else 0.0,
            Tinv=rel_f(self.Tinv, self.Tinv_true),
            Li=rel_f(self.Li, Lit, lower(n)),
            res=residual(self.Li, A),
            inv=float(np.abs(self.Ainv - self.Ainv_true).max() / np.abs(self.Ainv_true).max()))

    def figures(self, L, Tinv, Li, ainv):
        """The same figures of a device run (working matrix, tiles, L^-1, fp32 inverse n x n)."""
        n = self.n
        return dict(
            L=rel_f(L, self.L_true, below_tiles(n)) if n > W else 0.0,
            Tinv=rel_f(Tinv, self.Tinv_true),
            Li=rel_f(np.where(lower(n), Li, 0.0), self.Li_true, lower(n)),
            res=residual(np.where(lower(n), Li, 0.0), self.A),
            inv=float(np.abs(ainv.astype(np.float64) - self.Ainv_true).max() / np.abs(self.Ainv_true).max()))

    def bounds(self):
        """Device bounds: MULT x LAPACK's figure (floor n EPS); the fp32 inverse adds its storage rounding 2^-24."""
        b = {k: bound(v, self.n) for k, v in self.fig.items()}
        b['inv'] += U24
        return b


@functools.lru_cache(maxsize=None)
def reference(name, n):
    return Reference(family(name, n))


# ---- the panel's slab mapping ------------------------------------------------------------------------------------------------
def grid_of(m, w):
    """Workgroups of a panel launch: whole rows per workgroup, 1024 // w of them."""
    return -(-m // (SLAB // w)) if m > 0 else 1


def new_slab_ranges(m, w):
    rows = SLAB // w
    return [(min(b * rows, m), min((b + 1) * rows, m)) for b in range(grid_of(m, w))]


def old_slab_ranges(m, w):
    """The mapping this replaced, kept as the negative example: workgroup b owned the 1024 consecutive ENTRIES
    [1024 b, 1024 (b + 1)) of the row-major panel, entry idx at row idx // w -- so the rows it touched were these."""
    total = m * w
    grid = max(1, -(-total // SLAB))
    out = []
    for b in range(grid):
        lo, hi = min(b * SLAB, total), min((b + 1) * SLAB, total)
        out.append((lo // w, -(-hi // w)) if hi > lo else (0, 0))
    return out


def check_slab_partition(ranges, m, w):
    """The row ranges of a launch's workgroups partition [0, m): consecutive, no row in two of them, none above 1024 entries."""
    at = 0
    for lo, hi in ranges:
        if hi == lo:
            continue
        assert lo == at, 'row %d is owned %s' % (min(lo, at), 'twice' if lo < at else 'by nobody')
        assert hi > lo
        at = hi
    assert at == m, 'rows from %d on are owned by nobody' % at
    for lo, hi in ranges:
        assert (hi - lo) * w <= SLAB, 'a workgroup with %d entries' % ((hi - lo) * w)
