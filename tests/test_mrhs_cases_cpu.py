"""CPU: the generators of tests/mrhs_cases.py have the properties the GPU tests of the multi-right-hand-side layer rely on
(tests/test_gpu_mrhs_scale.py, tests/test_gpu_spmm_edges.py), and every size constant used there crosses the cap it is
named for on a device of 256 compute units."""
import numpy as np
import pytest

import mrhs_cases as mc

N_CUS = 256


def same_crs(A, B):
    return (A.n_rows == B.n_rows and A.n_cols == B.n_cols and np.array_equal(A.row_ptr, B.row_ptr) and
            np.array_equal(A.col, B.col) and np.array_equal(A.val.view(np.uint64), B.val.view(np.uint64)))


def test_spd_band_is_the_row_loop_version_entry_for_entry():
    from test_gpu_mcg import spd_band
    for n, half, seed in ((1921, 3, 1), (7, 3, 5), (4, 3, 5), (40, 1, 2)):
        assert same_crs(mc.spd_band(n, half, seed), spd_band(n, half, seed)), (n, half, seed)
    A = mc.spd_band(1921, 3, 1)
    x = np.random.default_rng(0).uniform(-1, 1, 1921)
    got = mc.band_matvec(1921, mc.spd_band_diagonals(1921, 3, 1), x, dtype=np.float64)
    rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
    want = np.bincount(rows, weights=A.val * x[A.col], minlength=A.n_rows)
    assert np.max(np.abs(got - want)) <= 1e-14 * np.max(np.abs(want))


def test_rhs_columns_is_the_mcg_recipe():
    from test_gpu_mcg import columns, host_spmv
    A = mc.spd_band(1921, 3, 1)
    for k in (3, 8):
        B, X0 = mc.rhs_columns(lambda v: host_spmv(A, v), 1921, k, seed=100 + k)
        Bw, X0w = columns(A, k, seed=100 + k)
        assert np.array_equal(B, Bw) and np.array_equal(X0, X0w)


@pytest.mark.parametrize("widths,fan", [(mc.WAVE_WIDTHS, 4), (mc.WAVE_WIDTHS_SMALL, 4), ([mc.level_w0(N_CUS), 2000], 3),
                                        ([1, 2, 1, 5, 3], 4), ([3], 2)])
def test_layered_lower_has_the_levels_it_is_built_for(widths, fan):
    T, D = mc.layered_lower(widths, fan, seed=11)
    n = sum(widths)
    rp = np.asarray(T.row_ptr)
    assert T.n_rows == n and len(D) == n and rp[-1] == len(T.col) == len(T.val)
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert np.all(T.col < rows), "not strictly lower"
    assert np.all(np.diff(T.col.astype(np.int64))[rows[1:] == rows[:-1]] > 0), "columns do not ascend (or repeat)"
    assert mc.level_widths(T) == list(widths)
    U = mc.mirror(T)
    urows = np.repeat(np.arange(n), np.diff(U.row_ptr))
    assert np.all(U.col > urows), "the mirror is not strictly upper"
    assert mc.level_widths(U, backward=True) == list(widths)
    # every row of level l > 0 holds a column of level l - 1, and min(fan, rows before the level) columns in all
    starts = np.concatenate([[0], np.cumsum(widths)])
    lens = np.diff(rp)
    for l in range(1, len(widths)):
        r = np.arange(starts[l], starts[l + 1])
        assert np.all(lens[r] == min(fan, starts[l])), l
        last = T.col[rp[r + 1] - 1]  # columns ascend: the largest one is the deepest dependency
        assert np.all((last >= starts[l - 1]) & (last < starts[l])), l
    assert np.all(lens[:widths[0]] == 0)
    assert np.all((D > 0) & np.isfinite(D)) and np.all(np.isfinite(T.val))
    # the scaling of ragged_lower: |entry| < scale / (count + 1) and scale <= D <= 2 scale, scale = 10^(-6..6)
    assert np.all(np.abs(T.val) * np.repeat(lens + 1, lens) <= np.repeat(D, lens))
    assert D.min() >= 1e-6 and D.max() <= 2e6


def test_mirror_is_the_row_loop_version():
    from test_gpu_sptrsm import mirror, ragged_lower
    L, _ = ragged_lower(200, 4)
    assert same_crs(mc.mirror(L), mirror(L))
    T, _ = mc.layered_lower([5, 7, 3, 9], 3, seed=2)
    assert same_crs(mc.mirror(T), mirror(T))
    assert same_crs(mc.mirror(mc.mirror(T)), T)


@pytest.mark.parametrize("K", range(2, 9))
def test_rows_at_cap_lengths_and_alignments(K):
    cap = mc.spmm_cap(K)
    assert cap == {2: 1916, 3: 1276, 4: 956, 5: 764, 6: 636, 7: 544, 8: 476}[K]
    for extra in (0, 1):
        A, long_rows = mc.rows_at_cap(K, seed=K, extra=extra)
        lens = np.diff(A.row_ptr)
        assert 3900 <= A.n_cols <= 4100 and A.col.min() >= 0 and A.col.max() < A.n_cols
        assert int(lens.max()) == cap - 3 + extra
        assert [int(lens[r]) for r in long_rows] == [cap - 3 + extra] * 4
        assert [int(A.row_ptr[r]) % 4 for r in long_rows] == [0, 1, 2, 3]
        others = np.delete(lens, long_rows)
        assert others.max() <= 3 and (others == 0).any()
        for r in long_rows:
            c = A.col[A.row_ptr[r]:A.row_ptr[r + 1]]
            assert len(np.unique(c)) == len(c) and np.any(np.diff(c.astype(np.int64)) < 0), "long rows: distinct, unsorted columns"
            assert lens[r - 1] in (1, 2, 3), "a filler row sets the alignment"
        # the launch condition of bis_spmm_launch: the tiled kernel iff max_row_nnz + 3 <= cap(K)
        assert (int(lens.max()) + 3 <= cap) == (extra == 0)
        if extra and K > 2:
            assert int(lens.max()) + 3 <= mc.spmm_cap(K - 1), "one entry longer still fits the tile at K - 1"
    # at alignment 3 the longest tiled row fills the tile to its last slot
    assert (cap - 3) + 3 == cap


@pytest.mark.parametrize("n,half,k", [(2000, 4, 8), (50, 7, 3), (5, 4, 2), (2, 1, 2)])
def test_spmm_band_ref_against_longdouble(n, half, k):
    diags, T, D_inv = mc.band_lower_full(n, half, seed=4)
    rp = np.asarray(T.row_ptr)
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert np.array_equal(np.diff(rp), np.minimum(np.arange(n), half))
    if len(T.col):
        assert np.all(T.col < rows) and np.all(rows - T.col <= half)
        assert np.array_equal(T.val, np.concatenate([[diags[r - c][c] for c in range(max(0, r - half), r)] for r in range(n)
                                                     if r > 0]))
    X = np.random.default_rng(5).uniform(-1, 1, (n, k)) * 10.0 ** np.arange(-3, k - 3)
    Y = mc.spmm_band_ref(diags, X)
    ld = {-d: v for d, v in diags.items()}
    exact = mc.band_matvec(n, ld, X, dtype=np.longdouble)
    mag = mc.band_matvec(n, {d: np.abs(v) for d, v in ld.items()}, np.abs(X), dtype=np.longdouble)
    bound = (half + 2) * 2.0 ** -53 * mag
    assert np.all(np.abs(Y.astype(np.longdouble) - exact) <= bound)
    assert np.all(Y[0] == 0.0)
    # ... and it is the sequential sum of the rounded products in CRS order, row by row
    for r in list(range(min(n, 2 * half + 2))) + [n - 1]:
        for j in (0, k - 1):
            p = T.val[rp[r]:rp[r + 1]] * X[T.col[rp[r]:rp[r + 1]], j]
            assert Y[r, j] == (np.cumsum(p)[-1] if len(p) else 0.0), (r, j)
    assert np.all(np.isfinite(mc.mitrsv_ref(diags, D_inv, X, 3)))
    assert np.array_equal(mc.mitrsv_ref(diags, D_inv, X, 0), (X * 1.0) * D_inv[:, None])


def test_lockstep_conditions_at_the_tested_size():
    """What test_gpu_mrhs_scale.py needs of spd_band(180001, 3, 1) with the columns of test_gpu_mcg.py: float64 CG at tol 1e-8
    converges well inside the 300 iterations the GPU tests allow, with Jacobi and without, and for every k used there at least
    two of the first k columns stop in different iterations, so that a column freezes while others run."""
    n = mc.N_LOCKSTEP
    diags = mc.spd_band_diagonals(n, 3, 1)
    mv = lambda v: mc.band_matvec(n, diags, v, dtype=np.float64)
    B, X0 = mc.rhs_columns(mv, n, 8, seed=108)
    for d in (None, diags[0]):
        counts = []
        for j in range(8):
            it, conv = mc.numpy_cg(mv, B[:, j], X0[:, j], 1e-8, 300, d=d)
            assert conv, (j, it)
            counts.append(it)
        print(f"numpy CG on spd_band({n}, 3, 1), {'Jacobi' if d is not None else 'no preconditioner'}: iterations {counts}")
        assert max(counts) <= 100, counts
        for k in (3, 7, 8):
            assert len(set(counts[:k])) >= 2, (k, counts)


def test_every_size_crosses_its_cap():
    """The caps from the constants in the sources: 2048 (kMaxReduceBlocks), 16,384 (kMpMaxBlocks), 8,192 (copy_grid),
    n_cus 32 (launch_level), n_cus 4 (launch_wave), with n_cus = 256."""
    assert [mc.lockstep_act(k) for k in (3, 5, 6, 7, 8)] == [255, 255, 252, 252, 256]
    for k in range(3, 9):
        assert mc.lockstep_strides(mc.N_LOCKSTEP, k), k
    assert not mc.lockstep_strides(174080, 3) and mc.lockstep_strides(174081, 3)  # k = 3 needs n > 174,080
    assert not mc.lockstep_strides(2744, 8)  # the largest case of the existing tests
    # the persistent sweep: launch_wave's grid is the residency cap
    n, w = sum(mc.WAVE_WIDTHS), max(mc.WAVE_WIDTHS)
    assert n == 77000 and len(mc.WAVE_WIDTHS) == 70 > mc.FEW_LEVELS
    grid, cap = mc.wave_grid(n, w, N_CUS)
    assert cap == 1024 and w + 1 > cap and n > 4 * cap and grid == cap
    assert mc.wave_grid(4096, 512, N_CUS)[0] == 513 < cap  # the widest level of the existing tests: not capped
    for widths in (mc.WAVE_WIDTHS, mc.WAVE_WIDTHS_SMALL):
        n, w = sum(widths), max(widths)
        assert len(widths) > mc.FEW_LEVELS
        grid, cap = mc.wave_grid(n, w, N_CUS, share=mc.WAVE_SHARE)
        assert cap == 128 and grid == cap and w + 1 > cap
        positions = -(-n // (4 * grid))
        assert positions == {21000: 42, 77000: 151}[n]  # a wave walks about 40 and 150 positions
    # the per-level sweep: level 0 strides at k = 8 and not at k = 3
    w0 = mc.level_w0(N_CUS)
    assert w0 == 267144
    grid, cap = mc.level_grid(w0, 8, N_CUS)
    assert grid == cap == 8192 and w0 * 8 > cap * 256
    grid, cap = mc.level_grid(w0, 3, N_CUS)
    assert grid < cap and w0 * 3 <= cap * 256
    # the elementwise kernels
    assert mc.N_DIAG * 8 > mc.MVEC_DIAG_MAX_BLOCKS * 256 >= mc.N_DIAG * 3
    assert (mc.N_DIAG * 8) % 256 != 0 and (mc.N_DIAG * 3) % 256 != 0
    assert mc.N_COPY > mc.MVEC_COPY_MAX_BLOCKS * 256 and mc.N_COPY % 256 != 0
