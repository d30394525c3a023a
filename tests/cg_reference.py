"""Plain-numpy references of the frozen-mesh solve's inner workings, shared by the tests (not a conftest): block-sparse
products that work in ``np.longdouble`` (scipy's sparse types do not), the PCG recursion in the order the driver of
csrc/cg.hip runs it, the smoothed-aggregation V-cycle as ``cycle_level`` of csrc/tri3_amg.hip runs it, the scalar
Chebyshev coefficients of ``amg_power_finish_kernel``, and the helpers of the numeric-setup restatement
(``_bsr``, ``_power``, ``_mgs``; test_gpu_amg.py imports them back).

Every function takes ``dtype`` = ``np.float64`` or ``np.longdouble``.  The tests run a reference twice, once in each, and
hold a kernel to a multiple of the gap between the two runs (``allowed``): the float64 run carries the same kind of rounding
the kernel does, the longdouble run (80-bit on x86-64, eps 1.08e-19) stands in for exact arithmetic."""
import numpy as np
import scipy.sparse as sp

EPS64 = float(np.finfo(np.float64).eps)
# per-level coefficient record of csrc/tri3_amg.hip
K_LAM, K_INV_THETA, K_C1, K_C2, K_OMEGA, K_SCALE, K_NORM = range(7)
# status record of csrc/hfem_amg.h
ST_ITER, ST_RNORM, ST_FNORM, ST_RHO, ST_REASON, ST_ALPHA, ST_BETA, ST_PQ, ST_TOL, ST_MAXITER, ST_HALTED, ST_RTOLWINS = range(12)


def assert_longdouble_is_wider():
    """The references need a type wider than double; a platform whose long double is double fails here, it is not skipped."""
    assert np.finfo(np.longdouble).eps < 1e-3 * EPS64, np.finfo(np.longdouble)


def allowed(dev):
    """What a kernel may deviate where the float64 reference deviates ``dev`` from the longdouble one: 32 x for another
    summation order and FMA contraction, and a floor of 64 eps for a step at which the two numpy runs happen to agree."""
    return 32.0 * dev + 64.0 * EPS64


def rel(a, b):
    """max|a - b| / max|b| as a float (b the reference; 0 when both vanish)."""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    num = np.abs(a - b).max()
    return 0.0 if num == 0 else float(num / np.abs(b).max())


# ---------------------------------------------------------------- block-sparse products in any dtype
class Bsr:
    """Block CSR matrix with ``rb x cb`` blocks: ``ptr`` [nb + 1], ``col`` [nnz], ``vals`` [nnz, rb, cb], ``ncols`` block
    columns.  ``rb = cb = 1`` is plain CSR.  Products sum each row's blocks in storage order with ``np.add.reduceat``."""

    def __init__(self, vals, ptr, col, rb, cb, ncols):
        self.ptr = np.asarray(ptr, dtype=np.int64)
        self.col = np.asarray(col, dtype=np.int64)
        self.vals = np.asarray(vals).reshape(-1, rb, cb)
        self.rb, self.cb, self.ncols = int(rb), int(cb), int(ncols)
        self.nb = len(self.ptr) - 1
        assert self.vals.shape[0] == len(self.col) == self.ptr[-1] and self.ptr[0] == 0
        assert len(self.col) == 0 or (0 <= self.col.min() and self.col.max() < self.ncols)

    @classmethod
    def from_dense(cls, M, rb, cb):
        """The blocks of a dense matrix that hold a nonzero, row by row."""
        nb, nc = M.shape[0] // rb, M.shape[1] // cb
        blocks = M.reshape(nb, rb, nc, cb).transpose(0, 2, 1, 3)
        keep = np.abs(blocks).max(axis=(2, 3)) > 0
        rows, cols = np.nonzero(keep)
        return cls(blocks[rows, cols], np.concatenate([[0], np.cumsum(keep.sum(axis=1))]), cols, rb, cb, nc)

    @property
    def shape(self):
        return (self.nb * self.rb, self.ncols * self.cb)

    def astype(self, dtype):
        return Bsr(self.vals.astype(dtype), self.ptr, self.col, self.rb, self.cb, self.ncols)

    def matvec(self, x):
        """y = A x in the common type of the blocks and x."""
        x = np.asarray(x).reshape(self.ncols, self.cb)
        dt = np.result_type(self.vals.dtype, x.dtype)
        y = np.zeros((self.nb, self.rb), dtype=dt)
        if len(self.col):
            prod = (self.vals.astype(dt) * x.astype(dt)[self.col][:, None, :]).sum(axis=2)        # [nnz, rb]
            full = np.nonzero(self.ptr[1:] > self.ptr[:-1])[0]                                    # reduceat needs non-empty runs
            y[full] = np.add.reduceat(prod, self.ptr[:-1][full], axis=0)
        return y.reshape(-1)

    def transpose(self):
        order = np.argsort(self.col, kind="stable")
        rows = np.repeat(np.arange(self.nb), np.diff(self.ptr))
        ptr = np.concatenate([[0], np.cumsum(np.bincount(self.col, minlength=self.ncols))])
        return Bsr(np.ascontiguousarray(self.vals[order].transpose(0, 2, 1)), ptr, rows[order], self.cb, self.rb, self.nb)

    def diagonal_blocks(self):
        """[nb, rb, rb]: the diagonal block of every block row (zero where the pattern has none)."""
        assert self.rb == self.cb
        out = np.zeros((self.nb, self.rb, self.rb), dtype=self.vals.dtype)
        rows = np.repeat(np.arange(self.nb), np.diff(self.ptr))
        on = rows == self.col
        out[rows[on]] = self.vals[on]
        return out

    def to_dense(self):
        out = np.zeros((self.nb, self.rb, self.ncols, self.cb), dtype=self.vals.dtype)
        rows = np.repeat(np.arange(self.nb), np.diff(self.ptr))
        out[rows, :, self.col, :] = self.vals
        return out.reshape(self.shape)


def csr_matvec(ptr, col, vals, x):
    """y = A x for a scalar CSR matrix with as many columns as x has entries."""
    return Bsr(vals, ptr, col, 1, 1, len(x)).matvec(x)


def block_diag_matvec(D, x):
    """y_i = D_i x_i for [n, bs, bs] blocks."""
    n, bs, _ = D.shape
    return (D * np.asarray(x).reshape(n, 1, bs)).sum(axis=2).reshape(-1)


def _apply(op, x):
    """Operators of ``pcg_steps``: None (identity), a callable, a ``Bsr`` or a dense array."""
    if op is None:
        return x.copy()
    if callable(op):
        return op(x)
    if isinstance(op, Bsr):
        return op.matvec(x)
    return op @ x


# ---------------------------------------------------------------- the PCG recursion, in the driver's order
def pcg_steps(K, M, g0, gz, n, dtype=np.longdouble, u0=None):
    """``n`` iterations of the driver's recursion on ``K u = f`` from ``u0`` (default 0): ``g0`` = dE/du at ``u0``, ``gz`` =
    dE/du at 0 (so |f| = |gz|).  Start: r = -g0, z = M r, rho = r.z, p = 0.  Step: p = z + beta p, q = K p, pq = p.q,
    alpha = rho / pq, u += alpha p, r -= alpha q, z = M r, rho' = r.z, beta = rho' / rho.  Returns n + 1 records (the first
    is the start) of what the status record holds after that iteration: iter, alpha, pq, rho, beta, rnorm, and u; the first
    also has fnorm.  No stopping rule: the caller reads the |r| sequence."""
    g0 = np.asarray(g0, dtype=dtype).reshape(-1)
    gz = np.asarray(gz, dtype=dtype).reshape(-1)
    u = np.zeros_like(g0) if u0 is None else np.array(u0, dtype=dtype).reshape(-1)
    r = -g0
    z = _apply(M, r)
    rho = r @ z
    p = np.zeros_like(r)
    beta = dtype(0.0)
    out = [dict(iter=0, alpha=dtype(0.0), pq=dtype(0.0), rho=rho, beta=beta, rnorm=np.sqrt(r @ r), fnorm=np.sqrt(gz @ gz),
                u=u.copy())]
    for k in range(1, n + 1):
        p = z + beta * p
        q = _apply(K, p)
        pq = p @ q
        alpha = rho / pq
        u = u + alpha * p
        r = r - alpha * q
        z = _apply(M, r)
        rho_new = r @ z
        beta = rho_new / rho
        rho = rho_new
        out.append(dict(iter=k, alpha=alpha, pq=pq, rho=rho, beta=beta, rnorm=np.sqrt(r @ r), u=u.copy()))
    return out


SCALARS = ("alpha", "pq", "rho", "beta", "rnorm")


def pcg_deviation(lo, hi):
    """Per step k, per quantity: the largest relative deviation of the float64 run ``lo`` from the longdouble run ``hi`` up to
    step k (scalars relative to their own size, u relative to max|u|)."""
    run = {q: 0.0 for q in SCALARS + ("u",)}
    out = []
    for a, b in zip(lo, hi):
        for q in SCALARS:
            if b[q] != 0:
                run[q] = max(run[q], float(abs(np.longdouble(a[q]) - b[q]) / abs(b[q])))
        run["u"] = max(run["u"], rel(a["u"], b["u"]))
        out.append(dict(run))
    return out


def block_jacobi(diag, dtype, identity=False):
    """M of the block-Jacobi preconditioner from the solver's ``diag`` rows {K_xx, K_xy, K_yy}: the adjugate inverse of every
    2x2 block, the identity for ``precond="none"`` or a block that is not positive definite (store_jacobi_block, csrc/hfem_cg_dev.h)."""
    d = np.asarray(diag, dtype=dtype)
    a, b, c = d[:, 0], d[:, 1], d[:, 2]
    det = a * c - b * b
    ok = (det > 0) & np.isfinite(det) & (not identity)
    safe = np.where(ok, det, dtype(1.0))
    D = np.empty((len(d), 2, 2), dtype=dtype)
    D[:, 0, 0] = np.where(ok, c / safe, 1.0)
    D[:, 0, 1] = D[:, 1, 0] = np.where(ok, -b / safe, 0.0)
    D[:, 1, 1] = np.where(ok, a / safe, 1.0)
    return lambda r: block_diag_matvec(D, r)


# ---------------------------------------------------------------- the V-cycle, as cycle_level runs it
def _smooth(L, x, b):
    """The two Chebyshev steps: d = (1 / theta) D^-1 r, x += d; then d = c1 d + c2 D^-1 r, x += d (x None: from zero)."""
    A, Dinv, coef = L["A"], L["Dinv"], L["coef"]
    r = b if x is None else b - A.matvec(x)
    d = coef[K_INV_THETA] * block_diag_matvec(Dinv, r)
    x = d if x is None else x + d
    r = b - A.matvec(x)
    d = coef[K_C1] * d + coef[K_C2] * block_diag_matvec(Dinv, r)
    return x + d


def vcycle(levels, coarse_inv, b, dtype=np.longdouble, level=0):
    """z = M b: per level two Chebyshev steps from zero, the residual, b_c = P^T r, the coarser levels, x += P x_c, the same
    two steps again; the coarsest level is ``coarse_inv @ b``.  ``levels``: one dict per level but the coarsest with ``A``
    (``Bsr``), ``Dinv`` ([n, bs, bs]), ``coef`` (the coefficient record) and ``P`` (``Bsr``); use ``cast_levels`` once to
    convert them to ``dtype``."""
    b = np.asarray(b, dtype=dtype).reshape(-1)
    if level == len(levels):
        return np.asarray(coarse_inv, dtype=dtype) @ b
    L = levels[level]
    assert L["A"].vals.dtype == dtype, "cast_levels(levels, dtype) first"
    x = _smooth(L, None, b)
    r = b - L["A"].matvec(x)
    bc = L["PT"].matvec(r)
    x = x + L["P"].matvec(vcycle(levels, coarse_inv, bc, dtype, level + 1))
    return _smooth(L, x, b)


def cast_levels(levels, dtype):
    out = []
    for L in levels:
        P = L["P"].astype(dtype)
        out.append(dict(A=L["A"].astype(dtype), Dinv=np.asarray(L["Dinv"], dtype=dtype),
                        coef=np.asarray(L["coef"], dtype=dtype), P=P, PT=P.transpose()))
    return out


# ---------------------------------------------------------------- scalar coefficients (amg_power_finish_kernel)
def cheb_coefficients(lam, dtype=np.float64):
    """The coefficient record's scalars from lambda_hat, operation by operation as the kernel forms them."""
    lam = dtype(lam)
    lo = lam / dtype(30.0)
    theta = dtype(0.5) * (lam + lo)
    delta = dtype(0.5) * (lam - lo)
    sigma = theta / delta
    rho0 = dtype(1.0) / sigma
    rho1 = dtype(1.0) / (dtype(2.0) * sigma - rho0)
    return dict(lo=lo, theta=theta, delta=delta, sigma=sigma, rho0=rho0, rho1=rho1, inv_theta=dtype(1.0) / theta,
                c1=rho1 * rho0, c2=dtype(2.0) * rho1 / delta, omega=dtype(4.0) / (dtype(3.0) * lam))


def cheb_residual_polynomial(c, t):
    """What the two smoothing steps leave of an error component with eigenvalue ``t`` of D^-1 A:
    e2 = (1 - c2 t)(1 - t / theta) - (c1 / theta) t (from d0 = t e0 / theta, e1 = e0 - d0, d1 = c1 d0 + c2 t e1)."""
    return (1 - c["c2"] * t) * (1 - t * c["inv_theta"]) - c["c1"] * c["inv_theta"] * t


# ---------------------------------------------------------------- helpers of the numeric-setup restatement
def _bsr(vals, ptr, col, rb, cb, ncols):
    nb = len(ptr) - 1
    return sp.bsr_matrix((vals.reshape(-1, rb, cb), col, ptr), shape=(nb * rb, ncols * cb)).tocsr()


def _power(A, Dinv, n_rows):
    i = np.arange(n_rows, dtype=np.uint64)
    h = ((i + 1) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    v = (h >> np.uint64(8)).astype(np.float64) / 16777216.0 - 0.5
    v /= np.linalg.norm(v)
    nrm = 0.0
    for _ in range(30):
        w = Dinv @ (A @ v)
        nrm = np.linalg.norm(w)
        v = w / nrm
    return 1.1 * nrm


def _mgs(B, tol_rel=1e-10):
    Q = B.copy()
    R = np.zeros((3, 3))
    n0 = np.linalg.norm(Q[:, 0])
    for j in range(3):
        for k in range(j):
            R[k, j] = Q[:, k] @ Q[:, j]
            Q[:, j] -= R[k, j] * Q[:, k]
        nj = np.linalg.norm(Q[:, j])
        if j > 0 and not nj > tol_rel * n0:
            Q[:, j] = 0.0
            R[j, :] = 0.0
        else:
            R[j, j] = nj
            Q[:, j] /= nj
    return Q, R
