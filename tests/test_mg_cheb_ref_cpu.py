"""CPU: the numpy restatement of the Chebyshev smoother (tests/mg_cheb_ref.py) against independent arithmetic: the polynomial
of the restated coefficients against the closed-form Chebyshev residual polynomial, the bound and the power iteration
against numpy.linalg.eigvalsh on a small dense SPD matrix, the fall-back of a Rayleigh quotient that is not positive, the
cycle with the Jacobi sweep passed in against the two restatements it extends (bit for bit), and the one-level polynomial
preconditioner in a numpy PCG on HPCG 16^3."""
import numpy as np
import pytest

import mg_cheb_ref as cheb
import spgemm_ref as ref
import test_gpu_mg as base
import test_gpu_mg_cycle as cyc

LD = np.longdouble


def closed_form(lam, lmax, lmin, m):
    """T_m((theta - lam) / delta) / T_m(sigma) in longdouble by the three-term recurrence."""
    lam, lmax, lmin = lam.astype(LD), LD(lmax), LD(lmin)
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2

    def T(t):
        a, b = np.ones_like(t), t
        if m == 0:
            return a
        for _ in range(m - 1):
            a, b = b, 2 * t * b - a
        return b
    return T((theta - lam) / delta) / T(np.array([theta / delta], dtype=LD))[0]


@pytest.mark.parametrize("ratio", [4.0, 30.0])
@pytest.mark.parametrize("degree", range(1, 9))
def test_the_coefficients_give_the_chebyshev_residual_polynomial(degree, ratio):
    """On [1 / ratio, 1]: the sweep from x = 0 for the scalar systems lam x = 1 (A = diag(lam), w = 1, b = 1) leaves the
    residual 1 - lam x = T_m((theta - lam) / delta) / T_m(sigma).  Gate: 1e-12 of the polynomial's value at 0, which is 1
    (every step of the recurrence rounds at 1.1e-16 of |lam x| <= 1 whatever the size of the residual, so the error is
    absolute: a few 1e-16 per step times at most `ratio` steps' growth; a wrong coefficient changes the residual in the
    first digits)."""
    lmax, lmin = 1.0, 1.0 / ratio
    c1, c2 = cheb.coeffs(lmax, lmin, degree)
    assert c1[0] == 0.0 and c2[0] == 1.0 / ((lmax + lmin) / 2.0)
    lam = np.linspace(lmin, lmax, 200)
    A = ref.crs(200, 200, np.arange(201), np.arange(200), lam)
    x = cheb.cheb_sweep(A, np.ones(200), np.ones(200), None, c1, c2)
    got = 1.0 - lam * x
    want = closed_form(lam, lmax, lmin, degree)
    err = float(np.max(np.abs(got.astype(LD) - want)))
    print(f"degree {degree} ratio {ratio:g}: max |r - closed form| = {err:.3e}, max |closed form| = {float(np.max(np.abs(want))):.3e}")
    assert err <= 1e-12
    # the general step (an SpMV at k = 0 too) from the x a first polynomial left: the residual polynomial squared
    x2 = cheb.cheb_sweep(A, np.ones(200), np.ones(200), x, c1, c2)
    assert np.max(np.abs((1.0 - lam * x2).astype(LD) - want * want)) <= 1e-12


def small_spd(n=40, seed=3):
    rng = np.random.default_rng(seed)
    B = rng.uniform(-1, 1, (n, n)) * (rng.random((n, n)) < 0.3)
    M = B @ B.T + 0.5 * np.eye(n)
    return M


def wa_spectrum(M, w):
    s = np.sqrt(w)
    return np.linalg.eigvalsh(s[:, None] * M * s[None, :])


@pytest.mark.parametrize("omega", [0.0, 0.7])
def test_bound_and_estimates_on_a_small_dense_spd_matrix(omega):
    M = small_spd()
    A = base.crs_from_dense(M)
    w = base.weights_reference(A, omega)
    lmax = wa_spectrum(M, w)[-1]
    bnd = cheb.bound(A, w)
    est = cheb.power_estimates(A, w, 30)
    print(f"omega {omega}: lambda_max(W A) = {lmax:.15e}, bound {bnd:.15e}, estimates {est[0]:.6e} .. {est[9]:.6e} .. {est[-1]:.15e}")
    assert bnd >= lmax
    assert abs(bnd - np.max(w * np.abs(M).sum(axis=1))) <= 1e-14 * bnd  # (numpy's row sum adds in another order)
    assert all(e <= lmax * (1 + 1e-12) for e in est)
    assert all(b >= a * (1 - 1e-12) for a, b in zip(est, est[1:])), "the Rayleigh quotients decrease"
    assert est[-1] >= 0.9 * lmax
    s = cheb.spectrum(A, w, 4.0, 10, 1.1)
    assert s["bound"] == bnd and s["estimate"] == est[9]
    assert s["lambda_max"] == min(bnd, np.float64(1.1) * est[9]) and s["lambda_min"] == s["lambda_max"] / 4.0
    s0 = cheb.spectrum(A, w, 4.0, 0, 1.1)
    assert s0["estimate"] == 0.0 and s0["lambda_max"] == bnd


def test_a_rayleigh_quotient_that_is_not_positive_falls_back_to_the_bound():
    for bad in (-0.3, 0.0, float("nan"), float("inf"), -float("inf")):
        est, lmax = cheb.lambda_max_rule(0.8, bad, 1.1)
        assert est == 0.0 and lmax == 0.8, bad
    assert cheb.lambda_max_rule(0.8, 0.5, 1.1) == (0.5, np.float64(1.1) * 0.5)
    assert cheb.lambda_max_rule(0.8, 0.79, 1.1) == (0.79, 0.8)
    # a negative definite matrix with its (positive) l1 weights: every quotient is negative
    M = -small_spd()
    A = base.crs_from_dense(M)
    w = base.weights_reference(A, 0.0)
    assert all(e < 0 for e in cheb.power_estimates(A, w, 5))
    s = cheb.spectrum(A, w, 4.0, 5, 1.1)
    assert s["estimate"] == 0.0 and s["lambda_max"] == s["bound"] == cheb.bound(A, w)


def hpcg(n):
    from oracle.pyoracle import Oracle
    A = Oracle().gen_hpcg(n)
    return ref.crs(A.n_rows, A.n_rows, A.row_ptr, A.col, A.val)


def test_with_the_jacobi_sweep_the_cycle_is_the_one_it_extends():
    """cheb.cycle with cheb=None against test_gpu_mg's V, test_gpu_mg_cycle's W / K and spgemm_ref's smoothed cycles."""
    A = hpcg(8)
    grid = (8, 8, 8, 1)
    v = np.random.default_rng(2).uniform(-1, 1, A.n_rows)
    plain = base.hierarchy_reference(A, grid, coarse_limit=8)
    smoothed = ref.hierarchy(A, grid, coarse_limit=8)
    assert len(plain) == 3 and len(smoothed) == 3
    assert base.same_bits(cheb.cycle(plain, v, cheb.config(nu=2, coarse_scale=1.5)), base.cycle_reference(plain, v, nu=2, coarse_scale=1.5))
    for c in (cheb.W, cheb.K, cheb.KGCR):
        assert base.same_bits(cheb.cycle(plain, v, cheb.config(cycle=c)), cyc.cycle_reference(plain, v, cyc.config(cycle=c))), c
    for c in (cheb.V, cheb.W, cheb.K):
        assert base.same_bits(cheb.cycle(smoothed, v, cheb.config(cycle=c, nu=2)), ref.cycle(smoothed, v, ref.config(cycle=c, nu=2))), c
    # and the Chebyshev sweep is another operator, in every one of them
    sm = cheb.smoother(plain, degree=2, ratio=4.0)
    for c in (cheb.V, cheb.W, cheb.K):
        a, b = cheb.cycle(plain, v, cheb.config(cheb=sm, cycle=c)), cheb.cycle(plain, v, cheb.config(cycle=c))
        assert np.max(np.abs(a - b)) > 1e-6 * np.max(np.abs(b))


def test_the_one_level_polynomial_preconditioner_beats_plain_cg_on_hpcg16():
    A = hpcg(16)
    b = base.host_spmv(A, np.ones(A.n_rows))
    one = base.hierarchy_reference(A, (16, 16, 16, 1), max_levels=1)
    assert len(one) == 1
    sm = cheb.smoother(one, degree=4, ratio=4.0, est_steps=10, safety=1.1)
    hp, _ = base.numpy_pcg(A, lambda r: cheb.cycle(one, r, cheb.config(cheb=sm, coarse_sweeps=1)), b, 1e-10, 300)
    hn, _ = base.numpy_pcg(A, lambda r: r.copy(), b, 1e-10, 300)
    print(f"HPCG 16^3: one level, Chebyshev degree 4, coarse_sweeps 1: {len(hp) - 1} iterations; unpreconditioned {len(hn) - 1}")
    assert hp[-1] < 1e-10 * hp[0] and hn[-1] < 1e-10 * hn[0]
    assert len(hp) < len(hn)
