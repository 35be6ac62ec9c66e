"""CPU: the numpy restatement of LSMR (tests/lsmr_ref.py, the iteration of include/bis_hip.h) against numpy.linalg.lstsq,
and how far the order of the sums moves its histories -- the figure that licenses the gate of tests/test_gpu_lsmr.py.

Inputs: T = banded(1301, 700, 5, 1), W = banded(700, 1301, 5, 2), S = banded(1025, 1025, 7, 3) (condition numbers 3.0, 2.6,
6.9), damping 0 and 0.5, b uniform(-1, 1) from default_rng(3), x0 = 0, tol 1e-10 for both tests.  Measured when the file
was written: 30 / 29, 26 / 26, 45 / 43 iterations; x against lstsq on the stacked system [A; damp I] 8e-11 .. 2e-10; the
histories of the three sum orders within 1.4e-16 hist[0]; the ar estimate at the stop equal to the explicit norm to six
digits, the r estimate to 2e-7."""
import numpy as np
import pytest

import lsmr_ref as L

CASES = [(name, damp) for name in L.TABLE for damp in L.DAMPS]


@pytest.fixture(scope="module")
def runs():
    """Every (input, damping) once, with the three dots."""
    out = {}
    for name in L.TABLE:
        A = L.table_matrix(name)
        At, b = L.transposed(A), L.rhs(A.n_rows)
        for damp in L.DAMPS:
            out[(name, damp)] = dict(A=A, b=b, lstsq=L.lstsq_damped(A, b, damp),
                                     res={k: L.lsmr(A, At, b, damp=damp, dot=f) for k, f in L.DOTS.items()})
    return out


def relerr(x, want):
    return np.linalg.norm(x - want) / np.linalg.norm(want)


def test_transposed_and_banded_are_what_they_say():
    for name, (m, n, per_row, _, cond, _) in L.TABLE.items():
        A = L.table_matrix(name)
        D = L.dense_of(A)
        assert (A.n_rows, A.n_cols) == (m, n) and np.all(np.diff(A.row_ptr) <= per_row + 1) and np.all(np.diff(A.row_ptr) >= 1)
        for i in (0, m // 2, m - 1):
            cols = A.col[A.row_ptr[i]:A.row_ptr[i + 1]]
            assert np.all(np.diff(cols) > 0) and i * n // m in cols
        assert np.array_equal(L.dense_of(L.transposed(A)), D.T)
        got = np.linalg.cond(D)
        print(f"{name}: condition number {got:.2f} (stated {cond})")
        assert abs(got - cond) < 0.06


@pytest.mark.parametrize("name,damp", CASES)
def test_restatement_against_lstsq(runs, name, damp):
    e = runs[(name, damp)]
    for k, r in e["res"].items():
        err = relerr(r["x"], e["lstsq"])
        print(f"{name} damp {damp} dot {k}: {r['iters']} iterations, reason {L.REASONS[r['reason']]}, |x - lstsq| / |lstsq| = {err:.2e}")
        assert r["converged"] and r["reason"] in (1, 2)
        assert err <= 1e-8
    assert e["res"]["np"]["iters"] == L.TABLE[name][5][L.DAMPS.index(damp)]


@pytest.mark.parametrize("name,damp", CASES)
def test_estimates_against_explicit_norms(runs, name, damp):
    e = runs[(name, damp)]
    D, r = L.dense_of(e["A"]), e["res"]["np"]
    res = e["b"] - D @ r["x"]
    ar = np.linalg.norm(D.T @ res - damp * damp * r["x"])
    rr = np.sqrt(res @ res + damp * damp * (r["x"] @ r["x"]))
    d_ar, d_r = abs(r["hist"][-1] - ar) / ar, abs(r["hist_r"][-1] - rr) / rr
    print(f"{name} damp {damp}: ar estimate {r['hist'][-1]:.6e} explicit {ar:.6e} ({d_ar:.1e}); r estimate {r['hist_r'][-1]:.6e} "
          f"explicit {rr:.6e} ({d_r:.1e})")
    assert d_ar <= 1e-4 and d_r <= 1e-5
    assert np.all(np.diff(r["hist"]) <= 0), "the ar history never increases"
    assert r["hist"][0] == np.linalg.norm(D.T @ e["b"]) or abs(r["hist"][0] - np.linalg.norm(D.T @ e["b"])) <= 1e-13 * r["hist"][0]
    assert abs(r["hist_r"][0] - np.linalg.norm(e["b"])) <= 1e-14 * r["hist_r"][0]


@pytest.mark.parametrize("name,damp", CASES)
def test_sum_order_moves_the_histories_by_rounding_only(runs, name, damp):
    res = runs[(name, damp)]["res"]
    base = res["np"]
    spread = 0.0
    for col in ("hist", "hist_r"):
        for r in res.values():
            k = min(len(r[col]), len(base[col]))
            spread = max(spread, np.max(np.abs(r[col][:k] - base[col][:k])) / base[col][0])
    print(f"{name} damp {damp}: largest deviation between np.dot, long double and block sums {spread:.2e} of entry 0")
    assert spread <= 1e-12
    assert len({r["iters"] for r in res.values()}) == 1


def test_wide_system_gives_the_minimum_norm_solution(runs):
    e = runs[("W", 0.0)]
    D, x = L.dense_of(e["A"]), e["res"]["np"]["x"]
    want = np.linalg.pinv(D) @ e["b"]
    print(f"W: |x - pinv(A) b| / |.| = {relerr(x, want):.2e}, |A x - b| = {np.linalg.norm(D @ x - e['b']):.2e}")
    assert relerr(x, want) <= 1e-8
    # any other solution is longer: x is orthogonal to the null space
    null = np.linalg.svd(D)[2][D.shape[0]:]
    assert np.max(np.abs(null @ x)) <= 1e-9 * np.linalg.norm(x)


def test_rank_deficient_system_gives_the_minimum_norm_solution():
    A = L.table_matrix("T")
    D = L.dense_of(A)
    D[:, 10] = D[:, 11]
    rows, cols = np.nonzero(D)
    B = L.from_triplets(A.n_rows, A.n_cols, rows, cols, D[rows, cols])
    assert np.linalg.matrix_rank(D) == A.n_cols - 1
    b = L.rhs(A.n_rows)
    r = L.lsmr(B, L.transposed(B), b)
    want = np.linalg.pinv(D) @ b
    print(f"rank-deficient T: {r['iters']} iterations, reason {L.REASONS[r['reason']]}, |x - pinv(A) b| / |.| = {relerr(r['x'], want):.2e}, "
          f"x[10] - x[11] = {r['x'][10] - r['x'][11]:.2e}")
    assert r["converged"] and relerr(r["x"], want) <= 1e-8
    assert abs(r["x"][10] - r["x"][11]) <= 1e-12 * np.linalg.norm(r["x"])


def test_column_scaling_repairs_a_badly_scaled_matrix():
    A = L.badly_scaled_T()
    At, b = L.transposed(A), L.rhs(A.n_rows)
    scaled = L.lsmr(A, At, b, d=1.0 / L.col_norms(A))
    plain = L.lsmr(A, At, b, iters=400)
    err = relerr(scaled["x"], L.lstsq_damped(A, b))
    print(f"badly scaled T: {scaled['iters']} iterations with d = 1 / column norms (|x - lstsq| {err:.2e}); without: "
          f"ar = {plain['hist'][-1] / plain['hist'][0]:.2e} ar0 after {plain['iters']}")
    assert scaled["converged"] and scaled["iters"] == 22 and err <= 1e-7
    assert not plain["converged"] and plain["iters"] == 400 and plain["hist"][-1] > 1e-4 * plain["hist"][0]


def test_breakdown_and_optimal_start():
    # three columns of one entry each, b along one of them: beta = 0 in iteration 1, exactly (every value a power of two)
    A = L.from_triplets(5, 3, [0, 2, 4], [0, 1, 2], [2.0, 2.0, 2.0])
    At = L.transposed(A)
    r = L.lsmr(A, At, np.array([2.0, 0, 0, 0, 0]))
    assert (r["iters"], r["converged"], r["reason"]) == (1, True, 3) and r["hist"][1] == 0 and np.array_equal(r["x"], [1.0, 0, 0])
    # x0 optimal with a residual that is not zero: rows 1 and 3 are not in the range
    r = L.lsmr(A, At, np.array([2.0, 1, 4, 1, 6]), x0=[1.0, 2, 3])
    assert (r["iters"], r["converged"], r["reason"]) == (0, True, 3) and r["hist"][0] == 0 and np.array_equal(r["x"], [1.0, 2, 3])
    r = L.lsmr(A, At, np.zeros(5))
    assert (r["iters"], r["converged"], r["reason"]) == (0, True, 3) and np.array_equal(r["x"], np.zeros(3))
    # a tolerance of 0 never fires: the solve runs on through rounding noise
    r = L.lsmr(A, At, np.array([1.0, 0.3, -0.7, 0.2, 0.9]), tol_r=0.0, iters=6)
    assert r["reason"] in (0, 3) and (r["reason"] == 3 or r["iters"] == 6)


def test_fma_restatement_keeps_what_a_fused_multiply_add_keeps():
    rng = np.random.default_rng(0)
    a, b = rng.uniform(-1, 1, 1000), rng.uniform(-1, 1, 1000)
    exact = L.fma(a, b, -(a * b))  # the rounding error of the product: lost without the fusion
    assert np.count_nonzero(exact) > 900 and np.all(np.abs(exact) <= 2.0 ** -53 * np.abs(a * b))
    lo = a.astype(np.longdouble) * b.astype(np.longdouble) - (a * b).astype(np.longdouble)
    assert np.max(np.abs(exact - lo.astype(np.float64))) <= 2.0 ** -60 * np.max(np.abs(a * b))


def test_against_scipy(runs):
    sla = pytest.importorskip("scipy.sparse.linalg")
    for (name, damp), e in runs.items():
        D = L.dense_of(e["A"])
        x = sla.lsmr(D, e["b"], damp=damp, atol=1e-12, btol=1e-12, maxiter=400)[0]
        err = relerr(e["res"]["np"]["x"], x)
        print(f"{name} damp {damp}: |x - scipy lsmr| / |.| = {err:.2e}")
        assert err <= 1e-8
