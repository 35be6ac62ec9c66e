"""CPU: the numpy restatement of bis_svds_* (tests/svds_ref.py) on its own -- the one-wave dense SVD, the method against
numpy.linalg.svd on every row of the table, the margins that make "equal restart counts" a fair demand on the device, and
how far the restatement moves between three orders of the sums, which is what licenses the GPU test's history gate.
Each test prints what it measured before it asserts."""
import numpy as np
import pytest

import svds_ref as S
from helpers import HIST_TOL

TOL = 1e-10
GATE = HIST_TOL["cg"]
MAX_CYCLES = 400


class Cache:
    def __init__(self):
        self.sys, self.runs = {}, {}

    def system(self, name):
        if name not in self.sys:
            A = S.make_input(name)
            D = S.dense_of(A)
            self.sys[name] = dict(A=A, At=S.transposed(A), D=D, sv=np.linalg.svd(D, compute_uv=False), norm1=S.norm1_of(A))
        return self.sys[name]

    def run(self, name, dots="np"):
        if (name, dots) not in self.runs:
            e = self.system(name)
            which, k, ncv = S.TABLE[name][2:5]
            self.runs[(name, dots)] = S.svds(e["A"], e["At"], k, ncv, which, TOL, max_cycles=MAX_CYCLES, dots=S.DOTS[dots])
        return self.runs[(name, dots)]


@pytest.fixture(scope="module")
def cache():
    return Cache()


# ---- the dense SVD of the restart ----------------------------------------------------------------------------------------
def restart_shaped(m, l, seed):
    """A matrix of the restart's shape: l kept values with their couplings in column l, then a bidiagonal."""
    rng = np.random.default_rng(seed)
    return S.assemble_B(np.sort(rng.uniform(0.5, 4.0, m))[::-1].copy(), rng.uniform(-1e-3, 1e-3, m), rng.uniform(0.5, 4.0, m),
                        rng.uniform(0.1, 2.0, m), l, m)


def dense_cases():
    for m in (2, 3, 20, 64):
        yield f"bidiagonal m={m}", restart_shaped(m, 0, m), False
        yield f"arrow m={m}", restart_shaped(m, S.keep_count(1, m), 100 + m), False
    for m in (2, 3, 20, 64):  # an alpha breakdown: the last diagonal entry is 0, so is the last row
        B = restart_shaped(m, 0, 200 + m)
        B[m - 1, m - 1] = 0.0
        yield f"zero last row m={m}", B, False
        B = restart_shaped(m, 0, 300 + m)
        B[:, 0] = 0.0
        yield f"zero column m={m}", B, True


@pytest.mark.parametrize("tag,B,zero_col", list(dense_cases()), ids=[c[0] for c in dense_cases()])
def test_dense_svd(tag, B, zero_col):
    m = B.shape[0]
    sigma, X, Y, sweeps, ok = S.jacobi_svd(B)
    ref = np.linalg.svd(B, compute_uv=False)
    smax = ref[0]
    live = sigma > 0.0
    ex = np.max(np.abs(X[:, live].T @ X[:, live] - np.eye(int(np.sum(live)))))
    ey = np.max(np.abs(Y.T @ Y - np.eye(m)))
    es = np.max(np.abs(np.sort(sigma)[::-1] - ref))
    eb = np.max(np.abs(B - (X * sigma) @ Y.T))
    print(f"{tag}: sweeps {sweeps}, ||X^T X - I|| {ex:.2e}, ||Y^T Y - I|| {ey:.2e}, |sigma - numpy| / sigma_max {es / smax:.2e}, "
          f"||B - X S Y^T|| / sigma_max {eb / smax:.2e}, zero columns of X {int(np.sum(~live))}")
    assert ok and sweeps <= S.MAX_SWEEPS
    assert ex <= 1e-13 and ey <= 1e-13
    assert es <= 1e-13 * smax and eb <= 1e-13 * smax
    if zero_col:
        assert not np.all(live) and np.all(X[:, ~live] == 0.0)


def test_round_robin_meets_every_pair_once():
    for me in (1, 2, 3, 7, 20, 63, 64):
        n2 = (me + 1) & ~1
        seen = [pq for r in range(n2 - 1) for pq in S.round_pairs(me, r)]
        assert sorted(seen) == [(p, q) for p in range(me) for q in range(p + 1, me)], me
        for r in range(n2 - 1):
            flat = [i for pq in S.round_pairs(me, r) for i in pq]
            assert len(flat) == len(set(flat)), (me, r)


# ---- the method ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.ROWS)
def test_against_numpy_svd(cache, name):
    e, got = cache.system(name), cache.run(name)
    which, k, ncv = S.TABLE[name][2:5]
    smax = e["sv"][0]
    w = S.wanted(e["sv"], k, which)
    res = S.residuals(e["D"], got["values"], got["U"], got["V"])
    dval = np.max(np.abs(got["values"] - w))
    ou, ov = S.orth_defect(got["U"]), S.orth_defect(got["V"])
    print(f"{name} k={k} ncv={ncv}: restarts {got['restarts']} products {got['products']} reason {S.REASONS[got['reason']]} nconv "
          f"{got['nconv']} max sweeps {max(got['sweeps'])} sigma_ref / sigma_max {got['sigma_ref'] / smax:.6f}; |sigma - numpy| / "
          f"sigma_max {dval / smax:.2e}; max residual / sigma_max {np.max(res) / smax:.2e}; U, V orthonormal to {ou:.2e}, {ov:.2e}")
    assert got["stopped"] and got["converged"] and got["nconv"] == k
    assert max(got["sweeps"]) <= S.MAX_SWEEPS
    assert dval <= 1e-12 * smax
    assert np.all(res <= 4 * TOL * smax)
    assert ou <= 1e-12 and ov <= 1e-12


@pytest.mark.parametrize("name", S.ROWS)
def test_margins(cache, name):
    """On a row that stops by CONVERGED the deciding ratio is at most 0.5 at the last restart and at least 2 before it."""
    got = cache.run(name)
    r = got["ratios"]
    print(f"{name}: reason {S.REASONS[got['reason']]}, restarts {got['restarts']}, products {got['products']}, last ratios "
          f"{[f'{x:.3g}' for x in r[-2:]]}")
    if got["reason"] != S.CONVERGED:
        assert got["reason"] == S.INVARIANT and got["restarts"] == 1 and got["products"] == 2 * S.TABLE[name][4]
        return
    assert r[-1] <= 0.5
    assert len(r) >= 2 and r[-2] >= 2.0


def test_the_table_covers_the_edges():
    shapes = {n: S.make_input(n) for n in S.ROWS}
    ncvs = [S.TABLE[n][4] for n in S.ROWS]
    assert any(a.n_rows > a.n_cols for a in shapes.values()) and any(a.n_rows < a.n_cols for a in shapes.values())
    assert any(a.n_rows == a.n_cols for a in shapes.values())
    assert any(min(a.n_rows, a.n_cols) & 1 for a in shapes.values()) and any(not max(a.n_rows, a.n_cols) & 1 for a in shapes.values())
    assert 64 in ncvs and any(16 < m < 64 for m in ncvs)  # a cycle of m steps walks every group count up to ceil(m / 8)
    assert any(S.TABLE[n][4] == min(shapes[n].n_rows, shapes[n].n_cols) for n in S.ROWS)
    assert "B3x2-LM" in S.TABLE and S.TABLE["B3x2-LM"][3:5] == (1, 2)


def test_sum_order_sensitivity(cache):
    """How far histories and values move between numpy's sums, long-double sums and sums over blocks of 256: the GPU test's
    gate (HIST_TOL["cg"], relative to entry 0 of the history) must exceed that by a factor 100 at least."""
    worst_h = worst_v = 0.0
    for name in S.ROWS:
        e, base = cache.system(name), cache.run(name)
        scale = S.hist_scale(base["hist"], e["norm1"])
        for dots in ("long", "blocks"):
            other = cache.run(name, dots)
            for key in ("restarts", "products", "reason", "nconv"):
                assert other[key] == base[key], (name, dots, key)
            dh = float(np.max(np.abs(other["hist"] - base["hist"]))) / scale
            dv = float(np.max(np.abs(other["values"] - base["values"]))) / base["sigma_ref"]
            print(f"{name} np against {dots}: max |d hist| / scale {dh:.2e}, max |d sigma| / sigma_ref {dv:.2e}")
            worst_h, worst_v = max(worst_h, dh), max(worst_v, dv)
    print(f"worst: histories {worst_h:.2e}, values {worst_v:.2e}; the gate {GATE:.1e} is {GATE / max(worst_h, 1e-300):.1e} times the "
          f"first, 2 tol = {2 * TOL:.1e} is {2 * TOL / max(worst_v, 1e-300):.1e} times the second")
    assert GATE >= 100 * worst_h
    assert 2 * TOL >= 100 * worst_v
