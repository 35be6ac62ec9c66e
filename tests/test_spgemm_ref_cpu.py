"""CPU: the numpy restatement of bis_spgemm, bis_mat_transpose and smoothed aggregation (tests/spgemm_ref.py) against
independent arithmetic: the product against a dense numpy product, the transpose against itself, and the smoothed
hierarchy with the restated cycle in a numpy PCG on HPCG 16^3 and 32^3 -- the property the feature exists for: fewer
iterations than unsmoothed aggregation, and a count that does not grow with the grid.

The gate of the product is 1e-14 |.|_inf of the dense result (rows of at most a few dozen products of O(1) numbers, each
rounding 1.1e-16 relative: the bound is an order of magnitude above what a row can accumulate)."""
import numpy as np
import pytest

import spgemm_ref as ref
import test_gpu_mg as base


def random_crs(rng, n, m, per_row, sort=True, repeats=False):
    rp, col, val = [0], [], []
    for _ in range(n):
        k = int(rng.integers(0, per_row + 1))
        c = rng.choice(m, size=min(k, m), replace=False)
        if repeats and len(c) > 1:
            c = np.concatenate([c, c[:1]])
        if sort and not repeats:
            c = np.sort(c)
        col.extend(c.tolist())
        val.extend(rng.uniform(-1, 1, len(c)).tolist())
        rp.append(len(col))
    return ref.crs(n, m, rp, col, val)


def check_product(A, B, tag):
    C = ref.spgemm(A, B)
    D = ref.to_dense(A) @ ref.to_dense(B)
    assert C.n_rows == A.n_rows and C.n_cols == B.n_cols
    lens = np.diff(C.row_ptr)
    inner = np.ones(C.nnz, dtype=bool)
    inner[C.row_ptr[:-1][lens > 0]] = False
    assert np.all(np.diff(C.col.astype(np.int64))[inner[1:]] > 0), f"{tag}: columns do not ascend strictly"
    err = np.max(np.abs(ref.to_dense(C) - D)) if D.size else 0.0
    scale = np.max(np.abs(D)) if D.size else 0.0
    print(f"{tag}: nnz {C.nnz}, |C - dense|_inf = {err:.3e}, |dense|_inf = {scale:.3e}")
    assert err <= 1e-14 * scale
    # the pattern: exactly the positions some product lands on
    reach = (ref.to_dense(ref.crs(A.n_rows, A.n_cols, A.row_ptr, A.col, np.ones(A.nnz))) @
             ref.to_dense(ref.crs(B.n_rows, B.n_cols, B.row_ptr, B.col, np.ones(B.nnz)))) > 0
    got = np.zeros_like(reach)
    got[ref.rows_of(C), C.col] = True
    assert np.array_equal(got, reach), f"{tag}: pattern"
    return C


def test_product_square_rectangular_unsorted_and_repeated():
    rng = np.random.default_rng(1)
    A = random_crs(rng, 60, 60, 9)
    check_product(A, A, "square")
    check_product(random_crs(rng, 40, 17, 6), random_crs(rng, 17, 53, 8), "rectangular")
    check_product(random_crs(rng, 30, 20, 5, repeats=True), random_crs(rng, 20, 25, 6, sort=False), "repeats and unsorted rows")
    check_product(ref.crs_from_dense(base.band600()), ref.crs_from_dense(base.band600()), "band600")
    E = ref.spgemm(ref.crs(3, 4, [0, 0, 0, 0], [], []), random_crs(rng, 4, 5, 3))
    assert E.nnz == 0 and E.n_rows == 3 and E.n_cols == 5 and not E.row_ptr.any()


def cancelling_pair():
    """Row 0 of A B has 1 * 2 + 2 * (-1) = 0 at column 0: an entry of the pattern with the value 0."""
    A = ref.crs_from_dense(np.array([[1.0, 2.0, 0.0], [0.0, 1.0, 3.0], [0.5, 0.0, -0.5]]))
    B = ref.crs_from_dense(np.array([[2.0, 1.0, 0.0, 0.0], [-1.0, 0.0, 4.0, 0.0], [0.0, 0.0, 8.0, 0.0]]))
    return A, B


def test_cancelling_entries_stay_in_the_pattern():
    A, B = cancelling_pair()
    C = check_product(A, B, "cancelling")
    assert C.col[:3].tolist() == [0, 1, 2] and C.val[:3].tolist() == [0.0, 1.0, 8.0] and C.row_ptr[1] == 3


def test_transpose_twice_returns_the_original():
    rng = np.random.default_rng(2)
    A = random_crs(rng, 45, 31, 7)
    T = ref.transpose(A)
    assert T.n_rows == 31 and T.n_cols == 45 and np.array_equal(ref.to_dense(T), ref.to_dense(A).T)
    TT = ref.transpose(T)
    assert np.array_equal(TT.row_ptr, A.row_ptr) and np.array_equal(TT.col, A.col) and base.same_bits(TT.val, A.val)
    # repeats of a column inside a row stay adjacent, in that row's order
    R = ref.crs(2, 3, [0, 3, 4], [2, 0, 2, 2], [1.0, 2.0, 3.0, 4.0])
    Rt = ref.transpose(R)
    assert Rt.row_ptr.tolist() == [0, 1, 1, 4] and Rt.col.tolist() == [0, 0, 0, 1] and Rt.val.tolist() == [2.0, 1.0, 3.0, 4.0]


def scipy_product(A, B):
    C = (A.to_scipy() @ B.to_scipy()).tocsr()
    C.sort_indices()
    return ref.crs(A.n_rows, B.n_cols, C.indptr, C.indices, C.data)


def hpcg(n):
    from oracle.pyoracle import Oracle
    A = Oracle().gen_hpcg(n)
    return ref.crs(A.n_rows, A.n_rows, A.row_ptr, A.col, A.val)


def test_restriction_and_prolongation_are_the_matrix_products():
    rng = np.random.default_rng(3)
    P = random_crs(rng, 300, 40, 8)
    R = ref.transpose(P)
    d, e, x = rng.uniform(-1, 1, 300), rng.uniform(-1, 1, 40), rng.uniform(-1, 1, 300)
    rc = ref.restrict(R, d)
    assert np.max(np.abs(rc - ref.to_dense(R) @ d)) <= 1e-14 * np.max(np.abs(d)) * 300
    out = ref.prolong(P, x, e, 1.5)
    assert np.max(np.abs(out - (x + 1.5 * (ref.to_dense(P) @ e)))) <= 1e-14 * 8


COUNTS = {}


@pytest.mark.parametrize("n", [16, 32])
def test_smoothed_counts_are_lower_and_mesh_independent(n):
    A = hpcg(n)
    grid = (n, n, n, 1)
    b = base.host_spmv(A, np.ones(A.n_rows))
    smoothed = ref.hierarchy(A, grid, coarse_limit=64, product=scipy_product)
    plain = base.hierarchy_reference(A, grid, coarse_limit=64)
    hs, _ = base.numpy_pcg(A, lambda r: ref.cycle(smoothed, r), b, 1e-10, 200)
    hp, _ = base.numpy_pcg(A, lambda r: base.cycle_reference(plain, r), b, 1e-10, 200)
    its, itp = len(hs) - 1, len(hp) - 1
    rows = [L["A"].n_rows for L in smoothed]
    nnz = [L["A"].nnz for L in smoothed]
    print(f"HPCG {n}^3: smoothed V {its} iterations, unsmoothed V {itp}; smoothed rows {rows}, nnz {nnz}, "
          f"operator complexity {sum(nnz) / nnz[0]:.3f}, omega_l {[L['omega_l'] for L in smoothed[:-1]]}")
    assert hs[-1] < 1e-10 * hs[0] and hp[-1] < 1e-10 * hp[0]
    assert its < itp
    COUNTS[n] = its
    if len(COUNTS) == 2:
        assert abs(COUNTS[16] - COUNTS[32]) <= 2, COUNTS
