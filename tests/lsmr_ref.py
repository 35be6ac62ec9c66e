"""The LSMR iteration of include/bis_hip.h (bis_lsmr_*) restated in numpy, line by line, with the dot function as an
argument, and the inputs the LSMR tests share.  Not a test file.

The header's "one fma per element" lines are restated with `fma` below: the product of two doubles split without error
(Veltkamp / Dekker), added to the third operand with the rounding error of that sum carried along.  It differs from a
hardware fma by a double rounding in rare cases (one unit in the last place); what it keeps is the property the small cases
need -- a difference that a fused multiply-add gives exactly, such as t - c u of a 1 x 1 system, is not rounded to zero
first.  The scalar lines round every operation separately, as the device's one lane does."""
import numpy as np

from oracle.pyoracle import CRS

REASONS = {0: "live", 1: "tol_r", 2: "tol_ar", 3: "breakdown", 4: "non-finite"}


# ---- inputs ------------------------------------------------------------------------------------------------------------
def banded(m, n, per_row, seed, boost=4.0):
    """Row i: per_row entries at the columns clip(i n // m + integers(-6, 7), 0, n - 1) with values uniform(-1, 1) from
    default_rng(seed), repeated positions summed, `boost` added at (i, i n // m); ascending columns inside a row."""
    rng = np.random.default_rng(seed)
    centre = (np.arange(m, dtype=np.int64) * n) // m
    cols = np.clip(centre[:, None] + rng.integers(-6, 7, size=(m, per_row)), 0, n - 1)
    vals = rng.uniform(-1.0, 1.0, size=(m, per_row))
    rows = np.repeat(np.arange(m, dtype=np.int64), per_row + 1)
    cols = np.concatenate([cols, centre[:, None]], axis=1).ravel()
    vals = np.concatenate([vals, np.full((m, 1), boost)], axis=1).ravel()
    return from_triplets(m, n, rows, cols, vals)


def from_triplets(m, n, rows, cols, vals):
    """CRS with ascending columns inside a row; repeated positions are summed in the order given."""
    key = np.asarray(rows, dtype=np.int64) * n + np.asarray(cols, dtype=np.int64)
    uniq, inv = np.unique(key, return_inverse=True)
    val = np.zeros(len(uniq))
    np.add.at(val, inv, np.asarray(vals, dtype=np.float64))
    row_ptr = np.zeros(m + 1, dtype=np.int64)
    np.add.at(row_ptr, uniq // n + 1, 1)
    return CRS(m, np.cumsum(row_ptr), (uniq % n).astype(np.int32), val, n_cols=n)


def dense_of(A):
    D = np.zeros((A.n_rows, A.n_cols))
    rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
    np.add.at(D, (rows, A.col), A.val)
    return D


def transposed(A):
    """A^T on the host, ascending columns inside a row (the order bis_mat_transpose gives for such an A)."""
    rows = np.repeat(np.arange(A.n_rows, dtype=np.int64), np.diff(A.row_ptr))
    order = np.lexsort((rows, A.col))
    row_ptr = np.zeros(A.n_cols + 1, dtype=np.int64)
    np.add.at(row_ptr, np.asarray(A.col, dtype=np.int64) + 1, 1)
    return CRS(A.n_cols, np.cumsum(row_ptr), rows[order].astype(np.int32), A.val[order], n_cols=A.n_rows)


def scale_columns(A, s):
    return CRS(A.n_rows, A.row_ptr, A.col, A.val * s[A.col], n_cols=A.n_cols)


def host_spmv(A, x):
    rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
    return np.bincount(rows, weights=A.val * x[A.col], minlength=A.n_rows)


def rhs(m):
    return np.random.default_rng(3).uniform(-1.0, 1.0, m)


# the issue's table: name -> (m, n, per_row, seed, condition number, iterations with damping 0 and 0.5)
TABLE = {"T": (1301, 700, 5, 1, 3.0, (30, 29)), "W": (700, 1301, 5, 2, 2.6, (26, 26)), "S": (1025, 1025, 7, 3, 6.9, (45, 43))}
DAMPS = (0.0, 0.5)


def table_matrix(name):
    m, n, per_row, seed = TABLE[name][:4]
    return banded(m, n, per_row, seed)


def badly_scaled_T():
    """T with its columns multiplied by 10^uniform(-2, 2) from default_rng(11)."""
    A = table_matrix("T")
    return scale_columns(A, 10.0 ** np.random.default_rng(11).uniform(-2.0, 2.0, A.n_cols))


def col_norms(A):
    """Column norms as bis_mat_row_norms of the transpose sums them: in ascending row order, from 0."""
    s = np.zeros(A.n_cols)
    np.add.at(s, A.col, A.val * A.val)
    return np.sqrt(s)


# ---- dots --------------------------------------------------------------------------------------------------------------
def dot_np(a, b):
    return np.float64(np.dot(a, b))


def dot_long(a, b):
    return np.float64(np.sum(a.astype(np.longdouble) * b.astype(np.longdouble)))


def dot_blocks(a, b):
    s = np.float64(0.0)
    for i in range(0, len(a), 256):
        s = s + np.float64(np.dot(a[i:i + 256], b[i:i + 256]))
    return s


DOTS = dict(np=dot_np, long=dot_long, blocks=dot_blocks)


# ---- arithmetic --------------------------------------------------------------------------------------------------------
def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def fma(a, b, c):
    """a b + c with the product kept exactly (see the module's text); a is a scalar or a vector, b and c vectors."""
    a, b, c = np.float64(a) if np.ndim(a) == 0 else a, np.asarray(b), np.asarray(c)
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    out = s + (err + e)
    return np.where(np.isfinite(out), out, s)


def div0(a, b):
    """a / b, and 0 where b is 0: the reciprocal of zero is never formed."""
    return np.float64(0.0) if b == 0 else np.float64(a) / np.float64(b)


def rot(a, b):
    """den = sqrt(a^2 + b^2), c = a / den, s = b / den; den = 0 gives c = 1, s = 0."""
    den = np.sqrt(a * a + b * b)
    if den == 0:
        return np.float64(1.0), np.float64(0.0), den
    return a / den, b / den, den


# ---- the iteration -----------------------------------------------------------------------------------------------------
class Scalars:
    """The scalar state of one solve and the lines of the last arriver's lane 0: made from beta1 and alpha1, `step` takes
    an iteration's beta and alpha and returns the coefficients of pass H.  Also what a loop made of the library's
    single-vector calls keeps on the host."""

    def __init__(self, beta, alpha, damp=0.0, tol_r=1e-10, tol_ar=None):
        f8 = np.float64
        beta, alpha = f8(beta), f8(alpha)
        self.lam = f8(damp)
        self.ib, self.ia = div0(1.0, beta), div0(1.0, alpha)
        self.zetabar, self.alphabar = alpha * beta, alpha
        self.rho, self.rhobar, self.cbar, self.sbar = f8(1), f8(1), f8(1), f8(0)
        self.betadd, self.betad, self.rhodold, self.tautildeold, self.thetatilde, self.zeta, self.dsum = beta, f8(0), f8(1), f8(0), f8(0), f8(0), f8(0)
        self.cu = alpha * self.ib
        self.hist, self.hist_r = [self.zetabar], [beta]
        self.thr_r, self.thr_ar = f8(tol_r) * beta, f8(tol_r if tol_ar is None else tol_ar) * self.zetabar
        self.iters, self.converged, self.reason = 0, False, 0
        if self.zetabar == 0:
            self.converged, self.reason = True, 3
        elif not np.isfinite(self.zetabar) or not np.isfinite(beta):
            self.reason = 4

    def set_beta(self, beta):
        """after pass U"""
        self.beta = np.float64(beta)
        self.ib = div0(1.0, self.beta)

    def step(self, alpha):
        """after pass V: returns (c_hbar, c_x, c_h); ia, cu, the histories and the stop test are updated"""
        with np.errstate(all="ignore"):
            alpha, beta = np.float64(alpha), self.beta
            self.ia = div0(1.0, alpha)
            chat, shat, alphahat = rot(self.alphabar, self.lam)
            rhoold = self.rho
            c, s, self.rho = rot(alphahat, beta)
            thetanew = s * alpha
            self.alphabar = c * alpha
            rhobarold, zetaold = self.rhobar, self.zeta
            thetabar = self.sbar * self.rho
            self.cbar, self.sbar, self.rhobar = rot(self.cbar * self.rho, thetanew)
            self.zeta = self.cbar * self.zetabar
            self.zetabar = -self.sbar * self.zetabar
            c_hbar = div0(thetabar * self.rho, rhoold * rhobarold)
            c_x = div0(self.zeta, self.rho * self.rhobar)
            c_h = div0(thetanew, self.rho)
            betaacute = chat * self.betadd
            betacheck = -shat * self.betadd
            betahat = c * betaacute
            self.betadd = -s * betaacute
            thetatildeold = self.thetatilde
            ctildeold, stildeold, rhotildeold = rot(self.rhodold, thetabar)
            self.thetatilde = stildeold * self.rhobar
            self.rhodold = ctildeold * self.rhobar
            self.betad = -stildeold * self.betad + ctildeold * betahat
            self.tautildeold = div0(zetaold - thetatildeold * self.tautildeold, rhotildeold)
            taud = div0(self.zeta - self.thetatilde * self.tautildeold, self.rhodold)
            self.dsum = self.dsum + betacheck * betacheck
            diff = self.betad - taud
            normr = np.sqrt(self.dsum + diff * diff + self.betadd * self.betadd)
            normar = np.abs(self.zetabar)
            self.cu = alpha * self.ib
            self.hist.append(normar)
            self.hist_r.append(normr)
            self.iters += 1
            if not (np.isfinite(normar) and np.isfinite(normr)):
                self.reason = 4
            elif beta == 0 or alpha == 0:
                self.converged, self.reason = True, 3
            elif normr < self.thr_r:
                self.converged, self.reason = True, 1
            elif normar < self.thr_ar:
                self.converged, self.reason = True, 2
        return c_hbar, c_x, c_h

    def result(self, x):
        return dict(iters=self.iters, converged=self.converged, reason=self.reason, hist=np.array(self.hist),
                    hist_r=np.array(self.hist_r), x=x)


def lsmr(A, At, b, x0=None, damp=0.0, d=None, tol_r=1e-10, tol_ar=None, iters=400, dot=dot_np, spmv=host_spmv, track=False):
    """bis_lsmr_init + bis_lsmr_iterate(iters) + bis_lsmr_status.  A, At: host CRS (At = A^T); d: the column scaling or
    None.  Returns dict(iters, converged, reason, hist (the ar column), hist_r, x); with track=True also `xs`, the iterate
    after every step."""
    with np.errstate(all="ignore"):
        x = np.zeros(A.n_cols) if x0 is None else np.array(x0, dtype=np.float64)
        u = b - spmv(A, x)                                    # u~ = beta u
        beta = np.sqrt(dot(u, u))
        p = spmv(At, u) * div0(1.0, beta)
        if d is not None:
            p = p * d
        alpha = np.sqrt(dot(p, p))
        S = Scalars(beta, alpha, damp, tol_r, tol_ar)
        v = p * S.ia
        h, hbar = v.copy(), np.zeros(A.n_cols)
        xs = [x.copy()]
        while S.reason == 0 and S.iters < iters:
            w = v if d is None else d * v
            u = fma(-S.cu, u, spmv(A, w))                     # pass U
            S.set_beta(np.sqrt(dot(u, u)))
            p = spmv(At, u) * S.ib                            # pass V
            if d is not None:
                p = p * d
            vt = fma(-S.beta, v, p)
            c_hbar, c_x, c_h = S.step(np.sqrt(dot(vt, vt)))   # the last arriver's lane 0
            v = vt * S.ia                                     # pass H
            hbar = fma(-c_hbar, hbar, h)
            x = fma(c_x, hbar if d is None else d * hbar, x)
            h = fma(-c_h, h, v)
            if track:
                xs.append(x.copy())
    out = S.result(x)
    if track:
        out["xs"] = xs
    return out


def lstsq_damped(A, b, damp=0.0):
    """The minimum-norm solution of min ||A x - b||^2 + damp^2 ||x||^2 from numpy.linalg.lstsq on the stacked system."""
    D = dense_of(A)
    if damp:
        D = np.vstack([D, damp * np.eye(A.n_cols)])
        b = np.concatenate([b, np.zeros(A.n_cols)])
    return np.linalg.lstsq(D, b, rcond=None)[0]
