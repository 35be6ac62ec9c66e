"""numpy restatement of the Chebyshev smoother of the multigrid hierarchy (bis_mg_set_smoother, include/bis_hip.h): the
spectrum bound of W A, the power iteration that tightens it, the coefficients, the polynomial sweep, and the cycle with
either smoother.  No GPU is needed to import or run it.

The cycle here is the one of tests/test_gpu_mg.py (plain transfers) and tests/spgemm_ref.py (smoothed transfers) with the
sweep passed in: the transfers are theirs (base.run_sums, ref.restrict, ref.prolong), and the W and K steps are
ref.coarse_solve itself, bound to this module's cycle so that its recursion smooths as configured.  As there, SpMV row sums
and dot products are taken in np.longdouble and rounded once; everything else is the stated fp64 operation."""
import types

import numpy as np

import spgemm_ref as ref
import test_gpu_mg as base

LD = np.longdouble
JACOBI, CHEBYSHEV = 0, 1
V, W, K, KGCR = ref.V, ref.W, ref.K, 3
host_spmv, ldot = base.host_spmv, ref.ldot
f64 = np.float64


# ---- spectrum --------------------------------------------------------------------------------------------------------

def bound(A, w):
    """max_i w_i (sum_j |a_ij| left to right from 0): the product rounded, the maximum exact."""
    return f64(np.max(w * ref.abs_row_sums(A)))


def start_vector(n):
    """v_i = hash32(i) / 2^32 - 0.5 (exact in fp64)."""
    return np.array([base.hash32(i) for i in range(n)], dtype=np.float64) / 4294967296.0 - 0.5


def power_estimates(A, w, steps):
    """lambda_1 .. lambda_steps of the power iteration on W A in the W^-1 inner product."""
    v = start_vector(A.n_rows)
    out = []
    with np.errstate(all="ignore"):
        for _ in range(steps):
            y = host_spmv(A, v)
            out.append(ldot(v, y) / ldot(v, v / w))
            v = w * y
            v = v * (f64(1.0) / np.sqrt(ldot(v, v)))
    return out


def lambda_max_rule(bnd, estimate, safety):
    """(estimate as it counts, lambda_max): an estimate that is not finite or not positive counts as 0."""
    if not (np.isfinite(estimate) and estimate > 0.0):
        estimate = f64(0.0)
    if estimate == 0.0:
        return f64(0.0), f64(bnd)
    return f64(estimate), min(f64(bnd), f64(safety) * f64(estimate))


def spectrum(A, w, ratio, est_steps, safety):
    """dict(bound, estimate, lambda_max, lambda_min) of one level."""
    bnd = bound(A, w)
    est = power_estimates(A, w, est_steps)[-1] if est_steps > 0 else f64(0.0)
    est, lmax = lambda_max_rule(bnd, est, safety)
    return dict(bound=bnd, estimate=est, lambda_max=lmax, lambda_min=lmax / f64(ratio))


# ---- coefficients and the sweep -----------------------------------------------------------------------------------------

def coeffs(lambda_max, lambda_min, degree):
    """(c1, c2), arrays of `degree`, every operation one rounded fp64 step."""
    lmax, lmin = f64(lambda_max), f64(lambda_min)
    theta = (lmax + lmin) / f64(2.0)
    delta = (lmax - lmin) / f64(2.0)
    sigma = theta / delta
    rho = f64(1.0) / sigma
    c1, c2 = np.zeros(degree), np.zeros(degree)
    c2[0] = f64(1.0) / theta
    for k in range(1, degree):
        rho_new = f64(1.0) / (f64(2.0) * sigma - rho)
        c1[k] = rho_new * rho
        c2[k] = (f64(2.0) * rho_new) / delta
        rho = rho_new
    return c1, c2


def cheb_sweep(A, w, b, x, c1, c2):
    """One polynomial of degree len(c1) applied to x; x None: from x = 0, without the first SpMV."""
    d = None
    for k in range(len(c1)):
        if x is None:
            d = c2[0] * (w * b)
            x = d
            continue
        u = w * (b - host_spmv(A, x))
        d = c2[k] * u if k == 0 else (c1[k] * d) + (c2[k] * u)
        x = x + d
    return x


def jacobi_sweep(A, w, b, x):
    return w * b if x is None else x + w * (b - host_spmv(A, x))


def smoother(levels, degree=2, ratio=30.0, est_steps=10, safety=1.1, lambda_max=None):
    """What cfg["cheb"] takes: per level (c1, c2).  lambda_max: per level values to use in place of the restated ones (the
    device's own, where a test attributes a deviation to the cycle and not to the estimate)."""
    out = []
    for l, L in enumerate(levels):
        lmax = spectrum(L["A"], L["w"], ratio, est_steps, safety)["lambda_max"] if lambda_max is None else f64(lambda_max[l])
        out.append(coeffs(lmax, lmax / f64(ratio), degree))
    return out


# ---- the cycle -------------------------------------------------------------------------------------------------------

def config(cheb=None, **kw):
    """ref.config plus `cheb`: None (Jacobi) or smoother()'s list."""
    return dict(ref.config(**kw), cheb=cheb)


def cycle(levels, b, cfg=None, l=0):
    """One cycle of a plain or smoothed hierarchy for the right-hand side b, smoothing as cfg["cheb"] says."""
    cfg = cfg or config()
    L = levels[l]
    A, w = L["A"], L["w"]
    cheb = cfg.get("cheb")
    if cheb is None:
        def sweep(x):
            return jacobi_sweep(A, w, b, x)
    else:
        def sweep(x):
            return cheb_sweep(A, w, b, x, *cheb[l])

    x = sweep(None)
    if l + 1 == len(levels):
        for _ in range(cfg["coarse_sweeps"] - 1):
            x = sweep(x)
        return x
    for _ in range(cfg["nu"] - 1):
        x = sweep(x)
    d = b - host_spmv(A, x)
    if L.get("R") is not None:
        rc = ref.restrict(L["R"], d)
    else:
        agg = L["agg"]
        order = np.argsort(agg, kind="stable")
        ptr = np.searchsorted(agg[order], np.arange(int(agg.max()) + 2))
        rc = base.run_sums(d[order], ptr[:-1], ptr[1:])
    ec = coarse_solve(levels, rc, l, cfg)
    x = ref.prolong(L["P"], x, ec, cfg["coarse_scale"]) if L.get("P") is not None else x + cfg["coarse_scale"] * ec[L["agg"]]
    for _ in range(cfg["nu"]):
        x = sweep(x)
    return x


# ref.coarse_solve's code with `cycle` resolved here: the header's V, W and K steps, not restated a third time
coarse_solve = types.FunctionType(ref.coarse_solve.__code__, dict(vars(ref), cycle=cycle), "coarse_solve")
