"""Plain-numpy statement of one L-BFGS iteration, shared by the tests (not a conftest): what ``torch/optim/lbfgs.py`` does
with its defaults and no line search -- memory update if y.s > 1e-10, H_diag = y.s / y.y, the two-loop recursion on the
VECTORS (q = -g; q -= al_i y_i newest to oldest; r = H q; r += (al_i - be_i) s_i oldest to newest), first step
t = min(1, 1 / |g|_1) lr, the break tests -- written from that file, not from csrc/lbfgs.hip: the kernels run the recursion
on inner products (coefficient space), this file never forms a Gram matrix.

``LbfgsReference(history, dtype)``: ``dtype`` (``np.float64`` or ``np.longdouble``) is the type of every dot, coefficient
and axpy; the vectors' own type T (float64 or float32) is whatever the gradient comes in.  A test that holds the kernels
to it runs two instances on the same inputs, one per dtype (``cg_reference.allowed``: the kernel may deviate a multiple of
the gap between the two runs from the longdouble one), and feeds each iteration the previous direction and step AS READ
BACK FROM THE DEVICE: the pair it stores, y = T(g_k - g_{k-1}) computed in T and s = T(double(d_{k-1}) t), then has the bits
the kernels store, and only the arithmetic of the direction differs.  With ``d_prev`` / ``t_prev`` left out an instance runs
free on its own direction (tests/test_lbfgs_reference_host.py: against ``torch.optim.LBFGS`` itself).

Status record (``hfem_lbfgs_check``'s comment, csrc/lbfgs.hip): loss, flags, max|g|, g.d, t, history count, n_iter, H_diag;
flags: bit 0 max|g| <= tolerance_grad, 1 max|d| |t| <= tolerance_change, 2 |loss - prev_loss| < tolerance_change, 3 the
last direction stopped on g.d > -tolerance_change, 4 (sharded flow only) no direction was computed."""
from fractions import Fraction

import numpy as np

EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
ST_LOSS, ST_FLAGS, ST_GMAX, ST_GTD, ST_T, ST_COUNT, ST_NITER, ST_HDIAG = range(8)
F_OPT, F_STEP, F_LOSS, F_GTD, F_NODIR = 1, 2, 4, 8, 16


def assert_longdouble_is_wider():
    """The two-run tolerance needs a type wider than double; a platform whose long double is double fails, it is not skipped."""
    assert np.finfo(np.longdouble).eps < 1e-3 * EPS64, np.finfo(np.longdouble)


def allowed(dev, margin=32.0):
    """``cg_reference.allowed``: what a kernel may deviate from the longdouble run where the float64 run deviates ``dev``."""
    return margin * dev + 64.0 * EPS64


def _dot(a, b):
    return (a * b).sum()                                  # numpy's pairwise sum, in the operands' type


class LbfgsReference:
    def __init__(self, history, dtype=np.float64, lr=1.0, tolerance_grad=1e-7, tolerance_change=1e-9):
        self.history, self.dtype = int(history), dtype
        self.lr, self.tolerance_grad, self.tolerance_change = float(lr), float(tolerance_grad), float(tolerance_change)
        self.S, self.Y, self.ro = [], [], []              # old_stps, old_dirs (oldest first, in ``dtype``: exact copies of the T
        self.H_diag = dtype(1.0)                          # vectors), ro
        self.n_iter = 0
        self.prev_g = self.prev_loss = self.loss = None
        self.d = self.r = None                            # the last direction: in T, and before the rounding to T
        self.t, self.gtd, self.stop_gtd = dtype(0.0), dtype(0.0), False
        self.al, self.be = [], []

    # ---- the three places the host tests mutate
    def _accept(self, ys):
        return ys > 1e-10

    def _first_loop(self, m):
        return range(m - 1, -1, -1)

    def _refreshed_h(self, ys, yy):
        return ys / yy

    @property
    def count(self):
        return len(self.S)

    def _prev(self, d_prev, t_prev):
        return (self.d if d_prev is None else d_prev), (float(self.t) if t_prev is None else float(t_prev))

    def _break_flags(self, g, loss, d_prev, t_prev, after_update):
        gmax = float(np.abs(g).max())
        f = F_OPT if gmax <= self.tolerance_grad else 0
        if after_update:
            d_prev, t_prev = self._prev(d_prev, t_prev)
            if float(np.abs(d_prev).max()) * abs(t_prev) <= self.tolerance_change:
                f |= F_STEP
            if abs(float(loss) - float(self.prev_loss)) < self.tolerance_change:
                f |= F_LOSS
        return gmax, f

    def _record(self, flags, gmax):
        return [float(self.loss), float(flags), gmax, self.gtd, self.t, float(self.count), float(self.n_iter), self.H_diag]

    def check(self, g, loss, d_prev=None, t_prev=None, after_update=True):
        """The break tests that follow a closure evaluation; the record still has g.d, t, count, n_iter, H_diag of the LAST
        direction (the unsharded flow checks first, then calls ``direction``)."""
        self.loss = float(loss)
        gmax, f = self._break_flags(g, loss, d_prev, t_prev, after_update)
        if after_update and self.stop_gtd:
            f |= F_GTD
        return self._record(f, gmax)

    def direction(self, g, d_prev=None, t_prev=None, tolerance_change=None):
        """Memory update and direction for the gradient ``check`` saw last.  Returns a dict: accepted (None on the first
        iteration), count, H_diag, d (in T), gtd (= g.r, r the direction before its rounding to T), stop_gtd, t."""
        w, T = self.dtype, g.dtype
        tol = self.tolerance_change if tolerance_change is None else float(tolerance_change)
        self.n_iter += 1
        gw = g.astype(w)
        accepted = None
        if self.n_iter == 1:
            self.S, self.Y, self.ro, self.H_diag = [], [], [], w(1.0)
        else:
            d_prev, t_prev = self._prev(d_prev, t_prev)
            y = g - self.prev_g                                                   # flat_grad.sub(prev_flat_grad), in T
            s = (d_prev.astype(np.float64) * np.float64(t_prev)).astype(T)        # d.mul(t): one rounding to T
            yw, sw = y.astype(w), s.astype(w)
            ys = _dot(yw, sw)
            accepted = bool(self._accept(ys))
            if accepted:
                if len(self.S) == self.history:
                    self.S.pop(0), self.Y.pop(0), self.ro.pop(0)
                self.S.append(sw), self.Y.append(yw), self.ro.append(w(1.0) / ys)
                self.H_diag = self._refreshed_h(ys, _dot(yw, yw))
        m = len(self.S)
        if not (accepted is False and g is self.prev_g):   # (a dropped pair and the same gradient: the same direction again)
            al, be = [w(0.0)] * m, [w(0.0)] * m
            q = -gw
            for i in self._first_loop(m):
                al[i] = _dot(self.S[i], q) * self.ro[i]
                q -= al[i] * self.Y[i]
            r = q * self.H_diag
            for i in range(m):
                be[i] = _dot(self.Y[i], r) * self.ro[i]
                r += (al[i] - be[i]) * self.S[i]
            self.al, self.be, self.r, self.d = al, be, r, r.astype(T)
        r = self.r
        self.prev_g, self.prev_loss = g, self.loss
        self.t = w(min(w(1.0), w(1.0) / np.abs(gw).sum()) * w(self.lr)) if self.n_iter == 1 else w(self.lr)
        self.gtd = _dot(gw, r)
        self.stop_gtd = bool(self.gtd > -tol)
        return dict(accepted=accepted, count=m, H_diag=self.H_diag, d=self.d, gtd=self.gtd, stop_gtd=self.stop_gtd, t=self.t)

    def iterate(self, g, loss, d_prev=None, t_prev=None, tolerance_change=None):
        """One iteration of the unsharded flow: ``check`` then ``direction``; the record under ``status``."""
        rec = self.check(g, loss, d_prev, t_prev, after_update=self.n_iter > 0)
        out = self.direction(g, d_prev, t_prev, tolerance_change)
        out["status"] = rec
        return out

    def shard_iterate(self, g, loss, d_prev=None, t_prev=None, after_update=True, want_direction=True, tolerance_change=None):
        """The sharded flow's order of events: the break tests come BEFORE the pair is accepted; if one fires, or the caller
        wants no direction, nothing of the optimiser's state moves (ring, n_iter, prev_flat_grad, prev_loss) and bit 4 is set;
        else the iteration above, and the record has g.d, t and bit 3 of the direction just computed."""
        self.loss = float(loss)
        gmax, f = self._break_flags(g, loss, d_prev, t_prev, after_update)
        if f or not want_direction:
            return dict(accepted=None, count=self.count, H_diag=self.H_diag, d=None, gtd=self.gtd, stop_gtd=self.stop_gtd,
                        t=self.t, status=self._record(f | F_NODIR, gmax))
        tol = self.tolerance_change if tolerance_change is None else float(tolerance_change)
        out = self.direction(g, d_prev, t_prev, tol)
        out["status"] = self._record(f | (F_GTD if self.stop_gtd else 0), gmax)
        return out

    def term_magnitudes(self, g):
        """|H g_i| + sum_j (|H al_j Y_ji| + |(al_j - be_j) S_ji|) of the last direction, in float64: what an element of d is
        summed from (d cancels at some elements: errors are measured against this, not against |d_i|)."""
        H = abs(float(self.H_diag))
        out = H * np.abs(g.astype(np.float64))
        for a, b, s, y in zip(self.al, self.be, self.S, self.Y):
            out += abs(H * float(a)) * np.abs(y).astype(np.float64) + abs(float(a - b)) * np.abs(s).astype(np.float64)
        return out


# ---------------------------------------------------------------- the parameter update
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    def split(v):
        c = 134217729.0 * v                               # Veltkamp, 2^27 + 1
        hi = c - (c - v)
        return hi, v - hi
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def apply_update(x, d, t, fused=False):
    """T(double(x) + t double(d)).  ``fused=False``: the product rounded to double, then the sum.  ``fused=True``: ONE rounding
    to double (what a compiler that contracts the expression into a fused multiply-add computes), from error-free
    transformations: exact except within ~1e-16 ulp of a rounding tie, where ``apply_update_exact`` decides."""
    x64, d64, t = x.astype(np.float64), d.astype(np.float64), np.float64(t)
    if not fused:
        return (x64 + t * d64).astype(x.dtype)
    p, e = _two_prod(np.full_like(d64, t), d64)
    s, e1 = _two_sum(p, x64)
    return (s + (e1 + e)).astype(x.dtype)


def apply_update_exact(x, d, t):
    """One element of the fused form in rational arithmetic (``float`` of a ``Fraction`` is correctly rounded)."""
    v = float(Fraction(float(x)) + Fraction(float(t)) * Fraction(float(d)))
    return type(x)(v) if isinstance(x, np.floating) else v


# ---------------------------------------------------------------- the test problems of tests/test_gpu_lbfgs_lengths.py / _histories.py
class ChainProblem:
    """f(x) = 1/2 sum a_i x_i^2 + 1/2 c sum (x_{i+1} - x_i)^2 - b.x with a ~ U(0.5, 2.5), c = 0.5, b ~ N(0, 1), x0 ~ N(0, 1):
    convex, every L-BFGS pair is accepted, |g0|_1 >> 1 so the first step takes the 1 / |g|_1 branch.  Loss and gradient in
    float64 on the host, then cast to the vectors' type.

    ``stiff=True``: the same chain with a ~ 10 ** U(0, 5) (the same draws of the generator: b and x0 do not change).  The
    default converges before 20 pairs are kept (the g.d stop fires at iteration 17 of a free run); with a condition number of
    1e5 L-BFGS keeps accepting pairs for hundreds of iterations, so a history of 257 fills and the ring turns
    (tests/test_lbfgs_reference_host.py asserts that for every case of ``HISTORY_UNSHARDED`` / ``HISTORY_SHARDED``)."""

    def __init__(self, n, seed=20240611, stiff=False):
        rng = np.random.default_rng(seed)
        self.n, self.c = int(n), 0.5
        self.a = 10.0 ** rng.uniform(0.0, 5.0, n) if stiff else rng.uniform(0.5, 2.5, n)
        self.b = rng.standard_normal(n)
        self.x0 = rng.standard_normal(n)

    def loss_and_grad(self, x):
        """(loss as a float64 that is exactly representable in x's type, gradient in x's type)."""
        x64 = x.astype(np.float64)
        dx = np.diff(x64)
        g = self.a * x64 - self.b
        g[:-1] -= self.c * dx
        g[1:] += self.c * dx
        loss = 0.5 * _dot(self.a * x64, x64) + 0.5 * self.c * _dot(dx, dx) - _dot(self.b, x64)
        return float(x.dtype.type(loss)), g.astype(x.dtype)


# ---------------------------------------------------------------- the cases of tests/test_gpu_lbfgs_histories.py
STIFF_SEED = 1
_TWO_TURNS = (65, 100, 129)          # 2 (history + 1) + 3 iterations: head passes through every slot with a full ring


def stiff_chain(n):
    return ChainProblem(n, seed=STIFF_SEED, stiff=True)


# (n, T, history, applied iterations)
HISTORY_UNSHARDED = [(1031, T, h, 2 * (h + 1) + 3 if h in _TWO_TURNS else h + 3)
                     for h in (64, 65, 100, 128, 129, 256, 257) for T in (np.float64, np.float32)]
# (local lengths, T, history, iterations): world 1, and two handles in one process
HISTORY_SHARDED = ([((1030,), T, h, h + 3) for h in (100, 257) for T in (np.float64, np.float32)]
                   + [((686, 344), T, 129, 132) for T in (np.float64, np.float32)])
# FusedLBFGS through its Python driver: one step of max_iter iterations, two parameter tensors
HISTORY_FUSED = dict(n=1031, first_segment=37, history=100, max_iter=106)


# ---------------------------------------------------------------- the recursion in coefficient space
def coefficient_direction(S, Y, g):
    """The direction from inner products alone, in float64 -- the FORM csrc/lbfgs.hip evaluates, restated from its header
    comment (not from its kernels): with B = [S | Y | g] and the Gram matrix G = B^T B,
      al_i = ro_i (-s_i.g - sum_{j newer} al_j s_i.y_j),                       newest to oldest
      be_i = ro_i (H (-y_i.g - sum_j al_j y_i.y_j) + sum_{j older} c_j s_j.y_i),  c_i = al_i - be_i,  oldest to newest
      d = B r with r = (c, -H al, -H),  g.d = r . (B^T g),  ro_i = 1 / s_i.y_i,  H = s_m.y_m / y_m.y_m of the newest pair.
    S, Y: the kept pairs, oldest first.  Returns (d in float64, g.d, H)."""
    m = len(S)
    g64 = g.astype(np.float64)
    if m == 0:
        return -g64, -float(g64 @ g64), 1.0
    B = np.stack([np.asarray(v, dtype=np.float64) for v in list(S) + list(Y)] + [g64])
    G = B @ B.T
    SY, YY, Sg, Yg = G[:m, m:2 * m], G[m:2 * m, m:2 * m], G[:m, 2 * m], G[m:2 * m, 2 * m]
    ro = 1.0 / np.diag(SY)
    H = SY[m - 1, m - 1] / YY[m - 1, m - 1]
    al, c = np.zeros(m), np.zeros(m)
    for i in range(m - 1, -1, -1):
        al[i] = ro[i] * (-Sg[i] - al[i + 1:] @ SY[i, i + 1:])
    for i in range(m):
        be = ro[i] * (H * (-Yg[i] - al @ YY[i]) + c[:i] @ SY[:i, i])
        c[i] = al[i] - be
    r = np.concatenate([c, -H * al, [-H]])
    return r @ B, float(r @ G[:, 2 * m]), float(H)
