"""GPU: the FSAI preconditioner (bis_mat_fsai, BIS_PC_FSAI / "fsai") -- the factor's values against a longdouble
restatement of the definition in include/bis_hip.h, the pattern, the transpose, the fallback rows, the error table, the
apply on one and on several vectors, the fused CG against a numpy PCG on the downloaded factor, the three lock-step
solvers column by column, and the CLI.

Reference: `fsai_reference` below, in np.longdouble with its own Cholesky factorisation and back substitution (not
np.linalg: LAPACK's solve sits 4e-12 from the longdouble values on the scaled band, the definition's fp64 Cholesky 5e-16).
Gate for the values: max over the rows of |g_dev - g_ref|_inf / |g_ref|_inf <= 1e-13, the project's gate for ILU(0) values.

One row of the error table has no test: a row-range view cannot be made through the public interface (bis_mat_row_view is
internal to the library), so BIS_ERR_INVALID for a view is covered by the code only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import HIST_TOL, OptionScope, hist_dev
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

LD = np.longdouble
GATE = 1e-13
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "basic_iterative_solvers_amd", "host", "basic_iterative_solvers")


# ---- host side: inputs and the reference ---------------------------------------------------------------------------

def crs_from_dense(M, keep=None):
    """CRS of the entries of M that are non-zero (or of the mask `keep`), ascending columns."""
    keep = (M != 0.0) if keep is None else keep
    n = M.shape[0]
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    r, c = np.nonzero(keep)
    return CRS(n, rp, c.astype(np.int32), M[r, c], n_cols=M.shape[1])


def band_dense(n, half, density, seed):
    """Symmetric band of half-width `half`, each off-diagonal pair present with probability `density`, values uniform in
    [-1, 1], strictly dominant diagonal: SPD."""
    rng = np.random.default_rng(seed)
    M = np.zeros((n, n))
    for d in range(1, half + 1):
        v = rng.uniform(-1, 1, n - d) * (rng.random(n - d) < density)
        M[np.arange(d, n), np.arange(n - d)] = v
        M[np.arange(n - d), np.arange(d, n)] = v
    M[np.arange(n), np.arange(n)] = np.abs(M).sum(axis=1) * rng.uniform(1.1, 1.5, n) + 1e-3
    return M


def band600():
    return band_dense(600, 20, 0.5, 7)


def band600_scaled():
    """The same band under a symmetric scaling by 10^U(-3,3): plain CG stalls on it, any diagonal-aware preconditioner does not."""
    s = 10.0 ** np.random.default_rng(8).uniform(-3, 3, 600)
    L = np.tril(band600()) * s[:, None] * s[None, :]
    return L + np.tril(L, -1).T  # (symmetric bit for bit)


def full_band(lower_len):
    """Full band whose longest row, up to the diagonal, has exactly lower_len entries."""
    return band_dense(lower_len + 30, lower_len - 1, 1.1, 100 + lower_len)


def shuffled_rows(A, seed):
    """The same matrix with the entries inside every row in a random order."""
    rng = np.random.default_rng(seed)
    col, val = A.col.copy(), A.val.copy()
    for i in range(A.n_rows):
        s, e = A.row_ptr[i], A.row_ptr[i + 1]
        p = rng.permutation(e - s)
        col[s:e], val[s:e] = A.col[s:e][p], A.val[s:e][p]
    return CRS(A.n_rows, A.row_ptr, col, val)


def dense_of(A, dtype=np.float64):
    M = np.zeros((A.n_rows, A.n_cols), dtype=dtype)
    rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
    M[rows, A.col] = A.val
    return M


def lower_pattern(A):
    """Per row the ascending columns <= row."""
    out = []
    for i in range(A.n_rows):
        c = np.sort(A.col[A.row_ptr[i]:A.row_ptr[i + 1]])
        out.append(c[c <= i])
    return out


def chol_last_row(S):
    """g = C^-T e_m for S = C C^T, in S's dtype, from the lower triangle of S; None when a pivot is <= 0 or not finite."""
    m = len(S)
    Cf = np.zeros_like(S)
    for j in range(m):
        d = S[j, j] - np.dot(Cf[j, :j], Cf[j, :j])
        if not (d > 0) or not np.isfinite(d):
            return None
        Cf[j, j] = np.sqrt(d)
        if j + 1 < m:
            Cf[j + 1:, j] = (S[j + 1:, j] - Cf[j + 1:, :j] @ Cf[j, :j]) / Cf[j, j]
    g = np.zeros(m, dtype=S.dtype)
    for p in range(m - 1, -1, -1):
        g[p] = ((1 if p == m - 1 else 0) - np.dot(Cf[p + 1:, p], g[p + 1:])) / Cf[p, p]
    return g


def fsai_reference(A, dtype=LD):
    """The definition, row by row: (rows of G as (J, g) pairs, the indices of the fallback rows)."""
    L = np.tril(dense_of(A, dtype))  # only entries with column <= row are read
    rows, fallback = [], []
    for i, J in enumerate(lower_pattern(A)):
        assert len(J) and J[-1] == i
        S = L[np.ix_(J, J)]
        g = chol_last_row(S)
        if g is None:
            fallback.append(i)
            g = np.zeros(len(J), dtype=dtype)
            g[-1] = 1 / np.sqrt(np.abs(L[i, i]))
        rows.append((J, g))
    return rows, fallback


def host_spmv(A, x):
    rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
    return np.bincount(rows, weights=A.val * x[A.col], minlength=A.n_rows)


def numpy_pcg(A, G, b, tol, max_iters):
    """Preconditioned CG with M^-1 = G^T G from the downloaded factor, x0 = 0; the residual history and x."""
    Gt_apply = dense_of(G).T
    Gd = dense_of(G)
    x = np.zeros_like(b)
    r = b.copy()
    z = Gt_apply @ (Gd @ r)
    p = z.copy()
    rz = r @ z
    hist = [np.linalg.norm(r)]
    while len(hist) - 1 < max_iters and not hist[-1] < tol * hist[0]:
        Ap = host_spmv(A, p)
        alpha = rz / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        z = Gt_apply @ (Gd @ r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
        hist.append(np.linalg.norm(r))
    return np.array(hist), x


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- device side ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


def host_crs(dA):
    return CRS(dA.n_rows, *dA.download())


VALUE_CASES = {
    "hpcg876": (lambda c: c.gen_hpcg(8, 7, 6), 16),
    "fem666": (lambda c: c.gen_fem(6, 6, 6), 64),
    "band600": (lambda c: c.matrix(crs_from_dense(band600())), 32),
    "band600_scaled": (lambda c: c.matrix(crs_from_dense(band600_scaled())), 32),
    "diagonal": (lambda c: c.matrix(crs_from_dense(np.diag(np.random.default_rng(3).uniform(-2, 2, 300) + 3.0))), 16),
    "one_row": (lambda c: c.matrix(CRS(1, np.array([0, 1], dtype=np.int64), np.zeros(1, np.int32), np.array([2.5]))), 16),
    "lower16": (lambda c: c.matrix(crs_from_dense(full_band(16))), 16),
    "lower17": (lambda c: c.matrix(crs_from_dense(full_band(17))), 32),
    "lower32": (lambda c: c.matrix(crs_from_dense(full_band(32))), 32),
    "lower33": (lambda c: c.matrix(crs_from_dense(full_band(33))), 64),
    "lower64": (lambda c: c.matrix(crs_from_dense(full_band(64))), 64),
}


@pytest.fixture(scope="module")
def built(ctx):
    """Per case, computed once and left alone: the matrix, its host copy, the factors and their downloads, the reference."""
    cache = {}

    def get(name):
        if name not in cache:
            make, M = VALUE_CASES[name]
            dA = make(ctx)
            A = host_crs(dA)
            G, Gt, nf = ctx.fsai(dA)
            cache[name] = dict(dA=dA, A=A, n=A.n_rows, dG=G, dGt=Gt, nf=nf, G=host_crs(G), Gt=host_crs(Gt), M=M,
                               ref=fsai_reference(A))
        return cache[name]
    return get


def row_errors(G, ref_rows):
    """Per row |g_dev - g_ref|_inf / |g_ref|_inf (longdouble arithmetic); the pattern must be the reference's."""
    errs = np.zeros(len(ref_rows))
    for i, (J, g) in enumerate(ref_rows):
        s, e = G.row_ptr[i], G.row_ptr[i + 1]
        assert np.array_equal(G.col[s:e], J), f"row {i}: pattern {G.col[s:e]} instead of {J}"
        errs[i] = float(np.max(np.abs(G.val[s:e].astype(LD) - g)) / np.max(np.abs(g)))
    return errs


@pytest.mark.parametrize("name", sorted(VALUE_CASES))
def test_values_pattern_transpose_and_unit_diagonal(ctx, built, name):
    e = built(name)
    A, G, Gt, n = e["A"], e["G"], e["Gt"], e["n"]
    ref_rows, ref_fallback = e["ref"]
    assert e["nf"] == 0 and not ref_fallback
    longest = max(len(J) for J, _ in ref_rows)
    rp = 64 if e["dA"].rp_width == 8 else 32
    print(f"{name}: n {n}, longest lower row {longest}, kernel {e['dG'].fsai_kernel()!r}")
    assert e["dG"].fsai_kernel() == f"fsai_rows_kernel M={e['M']} RP={rp}"
    assert e["dGt"].fsai_kernel() == "" and e["dA"].fsai_kernel() == ""
    assert e["dG"].rp_width == e["dA"].rp_width == e["dGt"].rp_width
    # values (row_errors also holds the pattern of G to the sorted lower pattern of A)
    errs = row_errors(G, ref_rows)
    print(f"{name}: max row error {errs.max():.3e} (gate {GATE:.0e})")
    assert errs.max() <= GATE
    # Gt is the transpose of G bit for bit, with ascending columns
    Gd, Gtd = dense_of(G), dense_of(Gt)
    assert same_bits(Gtd, Gd.T)
    for i in range(n):  # ... on the sorted upper pattern of A
        c = np.sort(A.col[A.row_ptr[i]:A.row_ptr[i + 1]])
        assert np.array_equal(Gt.col[Gt.row_ptr[i]:Gt.row_ptr[i + 1]], c[c >= i]), i
    # diag(G A G^T) = 1 for the symmetric matrix the lower triangle defines (the products in longdouble numpy: the
    # check's own rounding stays out of the gate)
    L = np.tril(dense_of(A, LD))
    Asym = L + np.tril(L, -1).T
    GL = Gd.astype(LD)
    dev = np.abs(np.sum((GL @ Asym) * GL, axis=1) - 1)
    print(f"{name}: max |diag(G A G^T) - 1| {float(dev.max()):.3e}")
    assert float(dev.max()) <= GATE
    # two calls, the same bits
    G2, Gt2, nf2 = ctx.fsai(e["dA"])
    g2, gt2 = host_crs(G2), host_crs(Gt2)
    G2.free(); Gt2.free()
    assert nf2 == 0 and np.array_equal(g2.col, G.col) and same_bits(g2.val, G.val)
    assert np.array_equal(gt2.col, Gt.col) and same_bits(gt2.val, Gt.val) and np.array_equal(gt2.row_ptr, Gt.row_ptr)


def test_64_bit_row_pointers(ctx, built):
    e = built("fem666")
    with OptionScope(ctx, force_rp64=1):
        dA = ctx.gen_fem(6, 6, 6)
        assert dA.rp_width == 8
        G, Gt, nf = ctx.fsai(dA)
    assert G.fsai_kernel() == "fsai_rows_kernel M=64 RP=64" and G.rp_width == 8 and Gt.rp_width == 8 and nf == 0
    g, gt = host_crs(G), host_crs(Gt)
    errs = row_errors(g, e["ref"][0])
    print(f"fem666 rp64: max row error {errs.max():.3e}")
    assert errs.max() <= GATE
    # the row-pointer width changes nothing else
    assert np.array_equal(g.row_ptr, e["G"].row_ptr) and np.array_equal(g.col, e["G"].col) and same_bits(g.val, e["G"].val)
    assert np.array_equal(gt.row_ptr, e["Gt"].row_ptr) and np.array_equal(gt.col, e["Gt"].col) and same_bits(gt.val, e["Gt"].val)
    for m in (G, Gt, dA):
        m.free()


@pytest.mark.parametrize("name", ["band600", "band600_scaled"])
def test_order_inside_the_rows_does_not_matter(ctx, built, name):
    e = built(name)
    dS = ctx.matrix(shuffled_rows(e["A"], 5))
    assert not np.array_equal(host_crs(dS).col, e["A"].col)
    G, Gt, nf = ctx.fsai(dS)
    g, gt = host_crs(G), host_crs(Gt)
    assert nf == 0 and G.fsai_kernel() == e["dG"].fsai_kernel()
    assert np.array_equal(g.row_ptr, e["G"].row_ptr) and np.array_equal(g.col, e["G"].col) and same_bits(g.val, e["G"].val)
    assert np.array_equal(gt.row_ptr, e["Gt"].row_ptr) and np.array_equal(gt.col, e["Gt"].col) and same_bits(gt.val, e["Gt"].val)
    for m in (G, Gt, dS):
        m.free()


def test_upper_triangle_is_not_read(ctx, built):
    """Only entries with column <= row are read: other values right of the diagonal (same pattern) give the same bits."""
    e = built("band600")
    M = band600()
    U = np.triu(M, 1)
    M2 = np.tril(M) + np.where(U != 0, U * 3.0 + 0.25, 0.0)
    dB = ctx.matrix(crs_from_dense(M2))
    G, Gt, nf = ctx.fsai(dB)
    g = host_crs(G)
    assert nf == 0 and np.array_equal(g.col, e["G"].col) and same_bits(g.val, e["G"].val)
    for m in (G, Gt, dB):
        m.free()


def test_fallback_rows(ctx):
    t = 300
    M = band600()
    M[t, t] = -M[t, t]
    A = crs_from_dense(M)
    dA = ctx.matrix(A)
    G, Gt, nf = ctx.fsai(dA)
    g, gt = host_crs(G), host_crs(Gt)
    expected = [i for i in range(t, 600) if M[i, t] != 0.0]  # their pivot at t is a negative number minus squares
    ref_rows, ref_fallback = fsai_reference(A)
    print(f"fallback: {nf} rows on the device, {len(expected)} expected: {expected}")
    assert len(expected) > 1 and ref_fallback == expected
    assert nf == len(expected)
    for i in expected:
        s, e = g.row_ptr[i], g.row_ptr[i + 1]
        want = np.zeros(e - s)
        want[-1] = 1.0 / np.sqrt(np.abs(M[i, i]))
        assert g.col[e - 1] == i and same_bits(g.val[s:e], want), i
    errs = row_errors(g, ref_rows)
    others = np.setdiff1d(np.arange(600), expected)
    print(f"fallback: max row error of the other rows {errs[others].max():.3e}")
    assert errs[others].max() <= GATE
    assert same_bits(dense_of(gt), dense_of(g).T)
    for m in (G, Gt, dA):
        m.free()


def raw_fsai(ctx, A_handle, with_g=True, with_gt=True):
    g, gt = C.c_void_p(), C.c_void_p()
    nf = C.c_int64(-7)
    st = ctx.lib.bis_mat_fsai(ctx.h, A_handle, C.byref(g) if with_g else None, C.byref(gt) if with_gt else None, C.byref(nf))
    return st, g, gt, nf.value


def test_errors(ctx):
    INVALID, ZERO_DIAG, UNSUPPORTED = 2, 4, 6
    base = band_dense(40, 3, 1.1, 1)
    keep = base != 0.0

    def status_of(M, mask=None, crs=None):
        dA = ctx.matrix(crs if crs is not None else crs_from_dense(M, mask))
        st, g, gt, nf = raw_fsai(ctx, dA.h)
        assert not g and not gt, "out-parameters written on an error"
        dA.free()
        return st

    # BIS_ERR_INVALID: not square, null arguments
    assert status_of(None, crs=crs_from_dense(np.hstack([base, np.zeros((40, 2))]))) == INVALID
    dA = ctx.matrix(crs_from_dense(base))
    assert raw_fsai(ctx, None)[0] == INVALID
    st, g, gt, _ = raw_fsai(ctx, dA.h, with_g=False)
    assert st == INVALID and not gt
    st, g, gt, _ = raw_fsai(ctx, dA.h, with_gt=False)
    assert st == INVALID and not g
    st, g, gt, nf = raw_fsai(ctx, dA.h)  # (the matrix itself is fine)
    assert st == 0 and g and gt and nf == 0
    ctx.lib.bis_mat_destroy(ctx.h, g)
    ctx.lib.bis_mat_destroy(ctx.h, gt)
    # n_fallback_rows may be NULL
    g, gt = C.c_void_p(), C.c_void_p()
    assert ctx.lib.bis_mat_fsai(ctx.h, dA.h, C.byref(g), C.byref(gt), None) == 0 and g and gt
    ctx.lib.bis_mat_destroy(ctx.h, g)
    ctx.lib.bis_mat_destroy(ctx.h, gt)
    dA.free()
    # BIS_ERR_ZERO_DIAG: a row without a diagonal entry, a stored zero on the diagonal
    no_diag = keep.copy()
    no_diag[17, 17] = False
    assert status_of(base, no_diag) == ZERO_DIAG
    zero = base.copy()
    zero[23, 23] = 0.0
    assert status_of(zero, keep) == ZERO_DIAG
    # BIS_ERR_UNSUPPORTED: a lower row of 65 entries (64 passes: test_values..."lower64")
    assert status_of(full_band(65)) == UNSUPPORTED
    # ... a column repeated inside a row
    A = crs_from_dense(base)
    r = 20
    s = A.row_ptr[r]
    rp = A.row_ptr.copy()
    rp[r + 1:] += 1
    dup = CRS(40, rp, np.insert(A.col, s, A.col[s]), np.insert(A.val, s, 0.5))
    assert status_of(None, crs=dup) == UNSUPPORTED
    # ... a pattern that is not structurally symmetric: an upper entry without its mirror, a lower entry without its
    # mirror (the counts differ), and one of each (the counts agree, the transpose lookup misses)
    for drop in ([(10, 12)], [(12, 10)], [(10, 12), (31, 30)]):
        m = keep.copy()
        for rc in drop:
            assert m[rc]
            m[rc] = False
        assert status_of(base, m) == UNSUPPORTED, drop
    # n = 0
    empty = ctx.matrix(CRS(0, np.zeros(1, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0)))
    G, Gt, nf = ctx.fsai(empty)
    assert (G.n_rows, G.nnz, Gt.n_rows, Gt.nnz, nf) == (0, 0, 0, 0, 0)
    for m in (G, Gt, empty):
        m.free()


APPLY_CASES = {"hpcg": lambda c: c.gen_hpcg(16, 12, 10), "fem666": lambda c: c.gen_fem(6, 6, 6),
               "band600": lambda c: c.matrix(crs_from_dense(band600()))}


@pytest.fixture(scope="module")
def apply_systems(ctx):
    out = {}
    for name, make in APPLY_CASES.items():
        dA = make(ctx)
        G, Gt, nf = ctx.fsai(dA)
        assert nf == 0
        out[name] = dict(dA=dA, n=dA.n_rows, G=G, Gt=Gt)
    return out


@pytest.mark.parametrize("name", sorted(APPLY_CASES))
def test_apply_is_two_spmvs(ctx, apply_systems, name):
    from basic_iterative_solvers_amd import BisError
    e = apply_systems[name]
    n, G, Gt = e["n"], e["G"], e["Gt"]
    x = np.random.default_rng(11).uniform(-1, 1, n)
    dx, t, want, out, tmp = ctx.upload(x), ctx.alloc(n), ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
    ctx.spmv(G, dx, t)
    ctx.spmv(Gt, t, want)
    w = want.to_host()
    assert np.all(np.isfinite(w)) and np.any(w != 0.0)
    # against the downloaded factors in numpy: the apply really is Gt (G x)
    g, gt = host_crs(G), host_crs(Gt)
    hw = host_spmv(gt, host_spmv(g, x))
    assert np.max(np.abs(w - hw)) <= 1e-13 * np.max(np.abs(hw))
    ctx.init_vector(out, -7.0)
    ctx.apply_preconditioner("fsai", n, G, Gt, None, None, None, None, out, dx, tmp, None)
    assert same_bits(out.to_host(), w)
    assert same_bits(dx.to_host(), x)
    inout = ctx.upload(x)  # output aliasing input
    ctx.apply_preconditioner("fsai", n, G, Gt, None, None, None, None, inout, inout, tmp, None)
    assert same_bits(inout.to_host(), w)
    # tmp is required and distinct from input and output; both factors are required
    for bad_tmp, o, i in ((None, out, dx), (dx, out, dx), (out, out, dx)):
        with pytest.raises(BisError, match="status 2"):
            ctx.apply_preconditioner("fsai", n, G, Gt, None, None, None, None, o, i, bad_tmp, None)
    for ls, us in ((None, Gt), (G, None)):
        with pytest.raises(BisError, match="status 2"):
            ctx.apply_preconditioner("fsai", n, ls, us, None, None, None, None, out, dx, tmp, None)
    for v in (dx, t, want, out, tmp, inout):
        v.free()


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("name", sorted(APPLY_CASES))
def test_multi_vector_apply_column_by_column(ctx, apply_systems, name, k):
    from basic_iterative_solvers_amd import BisError
    e = apply_systems[name]
    n, G, Gt = e["n"], e["G"], e["Gt"]
    X = np.random.default_rng(12).uniform(-1, 1, (n, k)) * (10.0 ** np.arange(-k // 2, k - k // 2))[None, :k]
    dX, dOut, dTmp = ctx.upload(X.ravel()), ctx.alloc(n * k), ctx.alloc(n * k)
    ctx.init_vector(dOut, -7.0)
    ctx.mapply_preconditioner("fsai", n, k, G, Gt, None, None, None, None, dOut, dX, dTmp, None)
    got = dOut.to_host().reshape(n, k)
    col, out, tmp = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
    for j in range(k):
        col.set(X[:, j].copy())
        ctx.apply_preconditioner("fsai", n, G, Gt, None, None, None, None, out, col, tmp, None)
        assert same_bits(got[:, j], out.to_host()), (name, k, j)
    # (column-by-column equality is promised wherever the SpMV is not the wave-per-row kernel)
    assert "wave_per_row" not in G.spmv_kernel() and "wave_per_row" not in Gt.spmv_kernel(), (G.spmv_kernel(), Gt.spmv_kernel())
    # OUT may alias IN; TMP may not be missing or alias either; outer_iters != 1 stays unsupported
    dIO = ctx.upload(X.ravel())
    ctx.mapply_preconditioner("fsai", n, k, G, Gt, None, None, None, None, dIO, dIO, dTmp, None)
    assert same_bits(dIO.to_host().reshape(n, k), got)
    for bad in (None, dX, dOut):
        with pytest.raises(BisError, match="status 2"):
            ctx.mapply_preconditioner("fsai", n, k, G, Gt, None, None, None, None, dOut, dX, bad, None)
    with pytest.raises(BisError, match="status 6"):
        ctx.mapply_preconditioner("fsai", n, k, G, Gt, None, None, None, None, dOut, dX, dTmp, None, outer=2)
    for v in (dX, dOut, dTmp, col, out, tmp, dIO):
        v.free()


CG_TOL = 1e-10
CG_CASES = {"hpcg": lambda c: c.gen_hpcg(16, 12, 10), "fem666": lambda c: c.gen_fem(6, 6, 6),
            "band600": lambda c: c.matrix(crs_from_dense(band600())),
            "band600_scaled": lambda c: c.matrix(crs_from_dense(band600_scaled()))}


def device_cg(ctx, dA, b, pc=None, budget=400, **kw):
    """The fused CG from x0 = 0 to CG_TOL or `budget` iterations."""
    db, dx = ctx.upload(b), ctx.upload(np.zeros_like(b))
    cg = ctx.cg(dA, db, dx)
    if pc is not None:
        cg.set_preconditioner(pc, **kw)
    cg.init(CG_TOL)
    cg.iterate(budget)
    iters, conv, hist = cg.status()
    x = dx.to_host()
    cg.free(); db.free(); dx.free()
    return dict(iters=iters, conv=conv, hist=hist, x=x)


@pytest.mark.parametrize("name", sorted(CG_CASES))
def test_cg_against_numpy_pcg_on_the_downloaded_factor(ctx, name):
    dA = CG_CASES[name](ctx)
    A = host_crs(dA)
    G, Gt, nf = ctx.fsai(dA)
    assert nf == 0
    b = host_spmv(A, np.ones(A.n_rows))
    run = device_cg(ctx, dA, b, "fsai", Ls=G, Us=Gt)
    ref_hist, _ = numpy_pcg(A, host_crs(G), b, CG_TOL, 400)
    r0 = ref_hist[0]
    dev = hist_dev(run["hist"], ref_hist)
    res = np.linalg.norm(b - host_spmv(A, run["x"]))
    print(f"{name}: device {run['iters']} iterations conv {run['conv']}, numpy {len(ref_hist) - 1}, hist dev {dev:.3e}, "
          f"true residual {res:.6e}, last history entry {run['hist'][-1]:.6e}, r0 {r0:.6e}")
    assert run["conv"] and ref_hist[-1] < CG_TOL * r0
    assert dev <= HIST_TOL["cg"]
    assert abs(run["iters"] - (len(ref_hist) - 1)) <= 2
    assert res <= run["hist"][-1] + 1e-10 * r0
    if name == "band600":
        plain = device_cg(ctx, dA, b)
        print(f"{name}: unpreconditioned {plain['iters']} iterations conv {plain['conv']}")
        assert plain["conv"] and run["iters"] < plain["iters"]
    if name == "band600_scaled":
        plain = device_cg(ctx, dA, b, budget=2000)
        print(f"{name}: unpreconditioned {plain['iters']} iterations conv {plain['conv']}, last entry / r0 {plain['hist'][-1] / plain['hist'][0]:.3e}")
        assert not plain["conv"] and plain["iters"] == 2000
    for m in (G, Gt, dA):
        m.free()


@pytest.fixture(scope="module")
def lockstep_system(ctx):
    """gen_fem(6,6,6) with the FSAI factors in the slots the lock-step test files' pc_args hands to any type that is not
    none / j / gs / sgs (their ILU slots), and those files' columns."""
    import test_gpu_mcg_precond as tc
    dA = ctx.gen_fem(6, 6, 6)
    n = dA.n_rows
    A = host_crs(dA)
    G, Gt, nf = ctx.fsai(dA)
    assert nf == 0
    B, X0 = tc.columns(A, 3, seed=103)
    return dict(dA=dA, A=A, n=n, iLs=G, iUs=Gt, iLD=None, iUinv=None, iUD=None, B=B, X0=X0)


def test_lockstep_cg(ctx, lockstep_system):
    import test_gpu_mcg_precond as tc
    e, k = lockstep_system, 3
    run = tc.run_mcg(ctx, e, "fsai", 0, e["B"].copy(), e["X0"].copy())[0]
    for j in range(k):
        single = tc.run_cg(ctx, e, "fsai", 0, e["B"][:, j].copy(), e["X0"][:, j].copy())
        tc.check_column(f"fem666 fsai mcg k={k} j={j}", e["A"], e["B"][:, j], run["iters"][j], run["conv"][j], run["hist"][j],
                        run["X"][:, j], single)
    assert all(run["conv"])


def test_lockstep_bicgstab(ctx, lockstep_system):
    import test_gpu_mbicgstab as tb
    e, k = lockstep_system, 3
    run = tb.run_mbi(ctx, e, "fsai", 0, e["B"].copy(), e["X0"].copy())[0]
    for j in range(k):
        single = tb.run_single(ctx, e, "fsai", 0, e["B"][:, j].copy(), e["X0"][:, j].copy())
        tb.check_column(f"fem666 fsai mbicgstab k={k} j={j}", e["A"], e["B"][:, j], run["iters"][j], run["conv"][j],
                        run["hist"][j], run["X"][:, j], single)
    assert all(run["conv"])


def test_lockstep_gmres(ctx, lockstep_system):
    import test_gpu_mgmres as tg
    e, k, m = lockstep_system, 3, 10
    run = tg.run_mgm(ctx, e, "fsai", 0, e["B"].copy(), e["X0"].copy(), m=m)[0]
    for j in range(k):
        single = tg.run_single(ctx, e, "fsai", 0, e["B"][:, j].copy(), e["X0"][:, j].copy(), m)
        tg.check_column(ctx, f"fem666 fsai mgmres k={k} m={m} j={j}", e, "fsai", 0, j, run["iters"][j], run["conv"][j],
                        run["hist"][j], run["X"][:, j], single)
    assert all(run["conv"])


def test_lockstep_set_preconditioner_needs_the_factors_only(ctx, lockstep_system):
    from basic_iterative_solvers_amd import BisError
    e, k = lockstep_system, 3
    dB, dX = ctx.upload(e["B"].ravel()), ctx.upload(e["X0"].ravel())
    for make in (lambda: ctx.mcg(e["dA"], dB, dX, k), lambda: ctx.mbicgstab(e["dA"], dB, dX, k), lambda: ctx.mgmres(e["dA"], dB, dX, k),
                 lambda: ctx.cg(e["dA"], dB, dX)):
        s = make()
        for ls, us in ((None, e["iUs"]), (e["iLs"], None)):
            with pytest.raises(BisError, match="status 2"):
                s.set_preconditioner("fsai", Ls=ls, Us=us)
        s.set_preconditioner("fsai", Ls=e["iLs"], Us=e["iUs"])  # no diagonals
        s.free()
    dB.free(); dX.free()


RES = re.compile(r"\|\|A\*x_(\d+) - b\|\|_2 = (\S+)")


def run_cli(args):
    assert os.path.exists(BIN), "host binary not built (make -C basic_iterative_solvers_amd/host)"
    out = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"(converged in: |did not converge after )(\d+) iterations", out.stdout)
    assert m, out.stdout[-1500:]
    return dict(iters=int(m.group(2)), converged=m.group(1).startswith("converged"), stdout=out.stdout)


def test_cli_cg(ctx):
    r = run_cli(["hpcg:16", "-cg", "-p", "fsai"])
    assert r["converged"] and "factorized sparse approximate inverse" in r["stdout"]
    # the Python solve of the same system: b = 1, x0 = 0.1, tolerance 1e-14 (the CLI's B_VAL, INIT_X_VAL, TOL)
    dA = ctx.gen_hpcg(16)
    n = dA.n_rows
    G, Gt, nf = ctx.fsai(dA)
    db, dx = ctx.upload(np.full(n, 1.0)), ctx.upload(np.full(n, 0.1))
    cg = ctx.cg(dA, db, dx)
    cg.set_preconditioner("fsai", Ls=G, Us=Gt)
    cg.init(1e-14)
    cg.iterate(400)
    iters, conv, _ = cg.status()
    print(f"hpcg:16 -cg -p fsai: CLI {r['iters']} iterations, Python {iters}")
    assert conv and abs(iters - r["iters"]) <= 2
    cg.free()
    for v in (db, dx, G, Gt, dA):
        v.free()


def test_cli_bicgstab_reordered():
    r = run_cli(["fem:8,8,8", "-bi", "-p", "fsai", "-perm", "rcm"])
    assert r["converged"] and "factorized sparse approximate inverse" in r["stdout"]
    assert "reverse Cuthill-McKee" in r["stdout"]
