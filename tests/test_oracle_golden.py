"""CPU: the oracle (C restatement) against the reference's golden vectors and
the known-answer vectors of the reference's own unit tests."""
import os

import numpy as np
import pytest

from helpers import (GOLDEN, GOLDEN_MATS, check_history, crs_of, has_repeated_column, load_golden, load_histories,
                     load_histories_mid, load_histories_r4, load_ilu_edges, gen_from_cli_arg, parse_hist_key, relerr)
from oracle.pyoracle import CRS

KTOL = 1e-13  # kernel-level relative tolerance (SURVEY.md 8d parity gate)


@pytest.mark.parametrize("name", ["FDM-2d-16", "matrix_band_klein"])
def test_mtx_reader_crs_bit_exact(oracle, name):
    """read_from_mtx + convert_coo_to_crs ordering (sparse_matrix.hpp:225-357):
    symmetric expansion, stable sort by row only -> bit-exact CRS."""
    g = load_golden(name)
    A = oracle.read_mtx(os.path.join(GOLDEN, name + ".mtx"))
    assert np.array_equal(A.row_ptr, g["A_rp"])
    assert np.array_equal(A.col, g["A_col"])
    assert np.array_equal(A.val, g["A_val"])


def test_band_klein_rows_not_sorted():
    """SURVEY defect 7: the general-format fixture has non-ascending rows; the
    kernels must not assume sorted columns."""
    g = load_golden("matrix_band_klein")
    rp, col = g["A_rp"], g["A_col"]
    unsorted = sum(1 for r in range(len(rp) - 1)
                   if np.any(np.diff(col[rp[r]:rp[r + 1]]) < 0))
    assert unsorted == 99


@pytest.mark.parametrize("name", GOLDEN_MATS)
def test_split_and_peel_bit_exact(oracle, name):
    g = load_golden(name)
    A = crs_of(g, "A")
    L, Ls, U, Us = oracle.split_LU(A)
    for k, M in zip(("L", "Ls", "U", "Us"), (L, Ls, U, Us)):
        assert np.array_equal(M.row_ptr, g[k + "_rp"]), k
        assert np.array_equal(M.col, g[k + "_col"]), k
        assert np.array_equal(M.val, g[k + "_val"]), k
    D, Dinv, st = oracle.peel_diag(L)
    assert st == 0
    D2, _, st2 = oracle.peel_diag(U)
    assert st2 == 0
    assert np.array_equal(D, g["A_D"]) and np.array_equal(Dinv, g["A_D_inv"])
    assert np.array_equal(D2, g["A_D"])
    assert np.array_equal(L.col, g["Lpeeled_col"])
    assert np.array_equal(L.val, g["Lpeeled_val"])
    assert np.array_equal(U.col, g["Upeeled_col"])
    assert np.array_equal(U.val, g["Upeeled_val"])
    s, st = oracle.extract_scale(A)
    assert st == 0 and np.array_equal(s, g["scale"])


@pytest.mark.parametrize("name", GOLDEN_MATS)
def test_kernels_vs_golden(oracle, name):
    g = load_golden(name)
    A, Ls, Us = crs_of(g, "A"), crs_of(g, "Ls"), crs_of(g, "Us")
    x, y, D, Dinv = g["x"], g["y"], g["A_D"], g["A_D_inv"]
    assert relerr(oracle.spmv(A, x), g["spmv"]) <= KTOL
    assert relerr(oracle.sptrsv(Ls, D, y), g["sptrsv"]) <= KTOL
    assert relerr(oracle.sptrsv(Us, D, y, backward=True), g["bsptrsv"]) <= KTOL
    inpl = y.copy()
    assert relerr(oracle.sptrsv(Ls, D, inpl, x=inpl), g["sptrsv_inplace"]) <= KTOL
    # elementwise kernels: bit-exact (fma form == the compiled reference)
    assert np.array_equal(oracle.subtract_vectors(x, y, 0.37), g["sub"])
    assert np.array_equal(oracle.sum_vectors(x, y, -1.25), g["sum"])
    assert np.array_equal(oracle.elemwise_mult_vectors(x, y, -1.0), g["mul"])
    assert np.array_equal(oracle.elemwise_div_vectors(x, D, 1.0), g["div"])
    assert np.array_equal(oracle.scale(x, 1.0 / 3.0), g["scale_vec"])
    assert abs(oracle.dot(x, y) - g["dot"][0]) <= KTOL * np.abs(x).dot(np.abs(y))
    assert abs(oracle.norm(x) - g["norm"][0]) <= KTOL * g["norm"][0]
    assert relerr(oracle.compute_residual(A, x, y), g["residual"]) <= KTOL
    assert relerr(oracle.normalize_x(g["spmv"], x, D, y), g["normalize_x"]) <= KTOL
    ones = np.ones(A.n_rows)
    for pc in ("none", "j", "gs", "bgs", "sgs", "2st", "s2st"):
        out = oracle.apply_preconditioner(pc, Ls, Us, D, Dinv, ones, ones, y)
        assert relerr(out, g["pc_" + pc]) <= KTOL, pc
    out = oracle.apply_preconditioner("gs", Ls, Us, D, Dinv, ones, ones, y,
                                      inplace=True)
    assert relerr(out, g["pc_gs_inplace"]) <= KTOL
    for pc in ("j", "gs", "sgs", "2st", "s2st"):
        out = oracle.apply_preconditioner(pc, Ls, Us, D, Dinv, ones, ones, y,
                                          outer=2, inner=2)
        assert relerr(out, g["pc22_" + pc]) <= 1e-12, pc
    assert relerr(oracle.multi_axpy(g["V"], g["yy"], 5), g["multi_axpy5"]) <= KTOL


@pytest.mark.parametrize("name", GOLDEN_MATS)
def test_ilu0_factors_vs_golden(oracle, name):
    """Serial ILU(0), factor_ILU0_old (LU_factors.hpp:320-539)."""
    g = load_golden(name)
    A = crs_of(g, "A")
    Ls, L_D, Us, U_D = oracle.factor_ilu0(A)
    assert np.array_equal(Ls.row_ptr, g["iluLs_rp"])
    assert np.array_equal(Ls.col, g["iluLs_col"])
    assert np.array_equal(Us.row_ptr, g["iluUs_rp"])
    assert np.array_equal(Us.col, g["iluUs_col"])
    assert relerr(Ls.val, g["iluLs_val"]) <= KTOL
    assert relerr(Us.val, g["iluUs_val"]) <= KTOL
    assert relerr(U_D, g["iluUD"]) <= KTOL
    assert np.array_equal(L_D, g["iluLD"])
    out = oracle.apply_preconditioner("ilu0", Ls, Us, g["A_D"], g["A_D_inv"],
                                      L_D, U_D, g["y"])
    assert relerr(out, g["pc_ilu0"]) <= 1e-12


_ILU_EDGES = load_ilu_edges()


@pytest.mark.parametrize("name", sorted(_ILU_EDGES))
def test_ilu0_edge_cases_vs_golden(oracle, name):
    """factor_ILU0_old on the adversarial catalogue (missing / zero / -0.0 / near-tolerance diagonals, empty rows, entries
    that cancel to 0, unsorted and unsymmetric rows, long rows, repeated columns, a long chain): the oracle, which the
    GPU tests use as the specification where the reference is absent, is the reference -- patterns and L_D / U_D exactly,
    values bit for bit where every operation is exact and within 1e-13 elsewhere; the ILU(0) apply within 1e-12."""
    c = _ILU_EDGES[name]
    Ls, L_D, Us, U_D = oracle.factor_ilu0(c["A"])
    for got, want in ((Ls, c["Ls"]), (Us, c["Us"])):
        assert np.array_equal(got.row_ptr, want.row_ptr) and np.array_equal(got.col, want.col)
        if c["exact"]:
            assert np.array_equal(got.val.view(np.uint64), want.val.view(np.uint64))
        else:
            assert relerr(got.val, want.val) <= KTOL
    assert np.array_equal(L_D, c["L_D"]) and np.array_equal(U_D.view(np.uint64), c["U_D"].view(np.uint64))
    out = oracle.apply_preconditioner("ilu0", Ls, Us, None, None, L_D, U_D, c["y"])
    assert relerr(out, c["pc_ilu0"]) <= 1e-12


def test_mtx_reader_keeps_repeated_entries(oracle):
    """ilu_dups.mtx splits five entries over two lines: the reader keeps every line (stable sort by row), as the
    reference's reader built the fixture's CRS."""
    A = oracle.read_mtx(os.path.join(GOLDEN, "ilu_dups.mtx"))
    want = _ILU_EDGES["mtx_dups"]["A"]
    assert np.array_equal(A.row_ptr, want.row_ptr) and np.array_equal(A.col, want.col) and np.array_equal(A.val, want.val)
    assert has_repeated_column(A) and A.nnz == 100


def test_ilu0_edge_catalogue_covers_the_issue():
    """The catalogue keeps its adversarial content: repeated columns, rows at and past the wave kernels' 1024-entry limit,
    rows longer than 64, empty rows, missing diagonals, unsorted rows, and cases whose factors are compared bit for bit."""
    lens = {k: np.diff(c["A"].row_ptr) for k, c in _ILU_EDGES.items()}
    assert lens["row_1024"].max() == 1024 and lens["row_1025"].max() == 1025
    assert all(has_repeated_column(_ILU_EDGES[k]["A"]) for k in _ILU_EDGES if k.startswith("dup_") or k == "mtx_dups")
    assert not any(has_repeated_column(_ILU_EDGES[k]["A"]) for k in ("row_1024", "long_rows", "chain_2500"))
    assert any(v.max() > 128 for v in lens.values()) and any((v == 0).any() for v in lens.values())
    assert sum(c["exact"] for c in _ILU_EDGES.values()) >= 10
    A = _ILU_EDGES["unsorted_reverse"]["A"]
    assert np.any(np.diff(A.col[A.row_ptr[5]:A.row_ptr[6]]) < 0)
    A = _ILU_EDGES["no_diag"]["A"]
    assert 1 not in A.col[A.row_ptr[1]:A.row_ptr[2]]


_H = load_histories()


@pytest.mark.parametrize("key", sorted(_H))
def test_residual_history_vs_golden(oracle, key):
    """Iteration schedules (methods/*.hpp): residual tables within
    1e-10 * r0 of the reference, iteration counts equal."""
    e = _H[key]
    name, solver, pc, kw = parse_hist_key(key)
    A = crs_of(load_golden(name), "A")
    r = oracle.solve(A, solver, pc, **kw)
    check_history(r, e, solver)


_HM = load_histories_mid()


@pytest.mark.parametrize("key", sorted(k for k in _HM if _HM[k]["rows"] <= 40000))
def test_mid_size_residual_history_vs_golden(oracle, key):
    """The same gate on the mid-size inputs (generator strings; HPCG-32, Anderson-32, the FEM stand-in) whose
    reference histories tests/golden/histories_mid.json holds; the largest (HPCG-48) is left to the GPU suite."""
    e = _HM[key]
    name, solver, pc, kw = parse_hist_key(key)
    r = oracle.solve(gen_from_cli_arg(oracle, e["cli"]), solver, pc, **kw)
    check_history(r, e, solver)


_H4 = load_histories_r4()


@pytest.mark.parametrize("key", sorted(_H4))
def test_round4_residual_history_vs_golden(oracle, key):
    """Raw (indefinite) Anderson: the first 100 CG iterations of the reference (SURVEY 8d parity gate item ii; with the
    Jacobi preconditioner over the rounding-independent window); the unstructured config-5 input with -bi -p ilu0,
    -gm -p gs, -cg -p sgs, -gs to convergence."""
    e = _H4[key]
    name, solver, pc, kw = parse_hist_key(key)
    r = oracle.solve(gen_from_cli_arg(oracle, e["cli"]), solver, pc, **kw)
    if "max_iters" in kw:
        n = min(len(e["hist"]), e["stable_len"], len(r["hist"]))
        assert n >= min(e["stable_len"], 101) and len(r["hist"]) == len(e["hist"])
        g = np.array(e["hist"][:n])
        # (a window cut by `stable_len` is by definition the part on which differently rounded runs agree to 1e-9 r0)
        assert np.max(np.abs(np.asarray(r["hist"][:n]) - g)) / g[0] <= (1e-10 if n == len(e["hist"]) else 1e-9)
        return
    check_history(r, e, solver)


def test_unstr_generator_is_the_permuted_fem_matrix(oracle):
    """orc_gen_unstr = P A P^T of orc_gen_fem for perm = orc_unstr_perm, ascending columns, same values."""
    from helpers import permute_crs
    A = oracle.gen_fem(5, 4, 3, keep=70, seed=9)
    B = oracle.gen_unstr(5, 4, 3, keep=70, seed=9)
    perm = oracle.unstr_perm(A.n_rows, 9)
    assert sorted(perm) == list(range(A.n_rows)) and not np.array_equal(perm, np.arange(A.n_rows))
    P = permute_crs(A, perm)
    assert np.array_equal(P.row_ptr, B.row_ptr)
    for r in range(B.n_rows):
        s, t = B.row_ptr[r], B.row_ptr[r + 1]
        o = np.argsort(P.col[s:t], kind="stable")
        assert np.array_equal(P.col[s:t][o], B.col[s:t]) and np.array_equal(P.val[s:t][o], B.val[s:t])
        assert np.all(np.diff(B.col[s:t]) > 0)


# ---- the reference's own unit-test vectors (tests/test_kernels.cpp,
# tests/test_utilities.cpp, tests/test_solvers.cpp) ---------------------------
def test_ref_unit_spmv(oracle):
    A = CRS(3, [0, 1, 2, 3], [0, 1, 2], [1.0, 2.0, 3.0])
    assert np.allclose(oracle.spmv(A, np.ones(3)), [1, 2, 3], atol=1e-9)
    A = CRS(3, [0, 3, 6, 9], [0, 1, 2] * 3, np.arange(1.0, 10.0))
    assert np.allclose(oracle.spmv(A, np.array([1.0, 2.0, 3.0])), [14, 32, 50], atol=1e-9)


def test_ref_unit_sptrsv(oracle):
    Ls = CRS(3, [0, 0, 1, 3], [0, 0, 1], [1.0, -2.0, 1.0])
    D = np.array([2.0, 3.0, 4.0])
    x = oracle.sptrsv(Ls, D, np.array([2.0, 7.0, 12.0]))
    assert np.allclose(x, [1, 2, 3], atol=1e-9)
    Us = CRS(3, [0, 2, 3, 3], [1, 2, 2], [1.0, -2.0, 1.0])
    x = oracle.sptrsv(Us, D, np.array([-2.0, 9.0, 12.0]), backward=True)
    assert np.allclose(x, [1, 2, 3], atol=1e-9)


def test_ref_unit_vector_ops(oracle):
    a = np.array([1.0, 2.0, 3.0, 4.0])
    b = np.array([0.5, 1.5, 2.5, 3.5])
    assert np.allclose(oracle.subtract_vectors(a, b, 2.0), a - 2 * b, atol=1e-9)
    assert np.allclose(oracle.sum_vectors(a, b, 3.0), a + 3 * b, atol=1e-9)
    assert abs(oracle.dot(a, b) - 25.0) < 1e-9
    assert np.allclose(oracle.scale(a, 5.0), 5 * a, atol=1e-9)
    assert abs(oracle.norm(np.array([3.0, 4.0])) - 5.0) < 1e-9
    assert abs(oracle.norm(np.array([-1.0, 2.0, -2.0])) - 3.0) < 1e-9
    assert oracle.norm(np.zeros(0)) == 0.0  # empty vector


def test_ref_unit_coo_to_crs(oracle):
    A = oracle.coo_to_crs(3, [0, 0, 1, 2, 2, 2], [0, 2, 1, 0, 1, 2],
                          [10, 20, 30, 40, 50, 60])
    assert list(A.row_ptr) == [0, 2, 3, 6]
    assert list(A.col) == [0, 2, 1, 0, 1, 2]
    assert list(A.val) == [10, 20, 30, 40, 50, 60]


@pytest.mark.parametrize("solver,pc", [("cg", "none"), ("cg", "j"), ("bi", "none"),
                                       ("bi", "j"), ("j", "none"), ("gs", "none"),
                                       ("sgs", "none")])
def test_ref_unit_solvers_3x3(oracle, solver, pc):
    """tridiag(-1,2,-1), b={0,0,4}, x0=0 -> x*={1,2,3} (test_solvers.cpp:49-91).
    The oracle's b is a constant vector, so use the equivalent check through a
    scaled system: solve with b_val and compare against numpy."""
    A = CRS(3, [0, 2, 5, 7], [0, 1, 0, 1, 2, 1, 2],
            [2.0, -1.0, -1.0, 2.0, -1.0, -1.0, 2.0])
    r = oracle.solve(A, solver, pc, init_x=0.0, b_val=1.0, tol=1e-12)
    xs = np.linalg.solve(A.to_scipy().toarray(), np.ones(3))
    assert r["converged"]
    assert np.allclose(r["x"], xs, atol=1e-7)


def test_fem_generator_properties(oracle):
    """FEM-like stand-in for config 5 (oracle/bis_oracle.c orc_gen_fem): symmetric,
    strictly diagonally dominant with positive diagonal (SPD), ascending columns,
    ragged rows, and any row range equals the same rows of the full matrix."""
    import scipy.sparse as sp
    A = oracle.gen_fem(6, 5, 4, keep=85, seed=3)
    n = A.n_rows
    assert n == 3 * 6 * 5 * 4
    M = sp.csr_matrix((A.val, A.col, A.row_ptr), shape=(n, n))
    assert abs(M - M.T).max() == 0.0
    d = M.diagonal()
    off = np.asarray(abs(M).sum(axis=1)).ravel() - np.abs(d)
    assert (d > 0).all() and (d - off > 0.999).all()
    lens = np.diff(A.row_ptr)
    assert lens.min() < lens.max() and lens.max() <= 81 and (lens % 3 == 0).all()
    for r in range(n):
        c = A.col[A.row_ptr[r]:A.row_ptr[r + 1]]
        assert (np.diff(c) > 0).all()
    B = oracle.gen_fem(6, 5, 4, keep=85, seed=3, row0=100, row1=200)
    assert np.array_equal(B.col, A.col[A.row_ptr[100]:A.row_ptr[200]])
    assert np.array_equal(B.val, A.val[A.row_ptr[100]:A.row_ptr[200]])
    full = oracle.gen_fem(3, 3, 3, keep=100)
    assert np.diff(full.row_ptr).max() == 81 and np.diff(full.row_ptr).min() == 24
