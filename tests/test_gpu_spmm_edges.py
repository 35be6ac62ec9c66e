"""GPU: bis_spmm at the edges of its LDS tile and of its kernel choice -- rows of exactly the longest length the tiled kernel
takes (max_row_nnz + 3 == cap(K)) at every start alignment, rows one entry longer (the serial fallback), a row-block table
built with a chunk above 4096 (the other fallback condition), and row blocks without a single entry.  Generators:
tests/mrhs_cases.py (proved on the CPU by tests/test_mrhs_cases_cpu.py)."""
import numpy as np
import pytest

import mrhs_cases as mc
from helpers import OptionScope, check_rows
from oracle.pyoracle import CRS
from test_gpu_spmm import same_bits, spmm_checked

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


def upload(ctx, A, rp64):
    with OptionScope(ctx, force_rp64=1 if rp64 else -1):
        dA = ctx.matrix(A)
    assert dA.rp_width == (8 if rp64 else 4)
    return dA


def spmv_columns(ctx, dA, X):
    dy = ctx.alloc(max(dA.n_rows, 1))
    out = []
    for j in range(X.shape[1]):
        dx = ctx.upload(X[:, j])
        ctx.spmv(dA, dx, dy)
        out.append(dy.to_host()[:dA.n_rows])
        dx.free()
    dy.free()
    return out


def sequential_rows(A, x):
    """per row the sequential left-to-right sum of the rounded products (test_long_rows_take_the_serial_fallback_in_order)"""
    rp = A.row_ptr
    out = np.zeros(A.n_rows)
    for r in range(A.n_rows):
        p = A.val[rp[r]:rp[r + 1]] * x[A.col[rp[r]:rp[r + 1]]]
        out[r] = np.cumsum(p)[-1] if len(p) else 0.0
    return out


def check_block(ctx, dA, X, k, want_name, ref_spmv, seq, tag, x_offset=0):
    Y = spmm_checked(ctx, dA, np.ascontiguousarray(X[:, :k]), k, x_offset=x_offset)  # (checks the guard behind Y)
    name = dA.spmm_kernel()
    assert name == want_name, (tag, name)
    for j in range(k):
        assert same_bits(Y[:, j], ref_spmv[j]), (tag, j, "bis_spmv", np.nonzero(Y[:, j] != ref_spmv[j])[0][:8])
        assert same_bits(Y[:, j], seq[j]), (tag, j, "sequential sum")
    return Y


@pytest.mark.parametrize("rp64", [False, True])
@pytest.mark.parametrize("K", range(2, 9))
def test_rows_at_the_tile_cap(ctx, K, rp64):
    """Crosses max_row_nnz + 3 <= cap(K) = ((3840 / K) & ~3) - 4 (bis_spmm_launch) from both sides: rows of cap(K) - 3 entries
    starting at offsets 0, 1, 2, 3 (mod 4) of the non-zero stream take spmm_rowblock_kernel -- the one at offset 3 fills the
    tile to its last slot -- and rows one entry longer take spmm_lane_serial_kernel at K and the tiled kernel at K - 1."""
    rp = 64 if rp64 else 32
    rng = np.random.default_rng(100 + K)
    for extra in (0, 1):
        A, long_rows = mc.rows_at_cap(K, seed=10 * K + extra, extra=extra)
        assert int(np.diff(A.row_ptr).max()) + 3 == mc.spmm_cap(K) + extra
        assert [int(A.row_ptr[r]) % 4 for r in long_rows] == [0, 1, 2, 3]
        dA = upload(ctx, A, rp64)
        X = rng.uniform(-1, 1, (A.n_cols, K))
        ref = spmv_columns(ctx, dA, X)
        seq = [sequential_rows(A, X[:, j]) for j in range(K)]
        assert dA.spmv_kernel() != "spmv_wave_per_row_kernel"
        tag = f"K={K} RP={rp} extra={extra}"
        if extra == 0:
            v = 2 if K % 2 == 0 else 1  # (uploads are 16-byte aligned)
            Y = check_block(ctx, dA, X, K, f"spmm_rowblock_kernel K={K} V={v} RP={rp}", ref, seq, tag)
            if K % 2 == 0:  # X only 8-byte aligned: the 8-byte gathers, the same bits
                Y1 = check_block(ctx, dA, X, K, f"spmm_rowblock_kernel K={K} V=1 RP={rp}", ref, seq, tag + " V=1", x_offset=1)
                assert same_bits(Y1, Y)
        else:
            Y = check_block(ctx, dA, X, K, f"spmm_lane_serial_kernel K={K} RP={rp}", ref, seq, tag)
            if K > 2:
                k1 = K - 1
                v = 2 if k1 % 2 == 0 else 1
                check_block(ctx, dA, X, k1, f"spmm_rowblock_kernel K={k1} V={v} RP={rp}", ref, seq, tag + f" at K={k1}")
        for j in (0, K - 1):
            check_rows(Y[:, j], A, np.ascontiguousarray(X[:, j]), tag=tag)
        print(f"{tag}: longest row {int(np.diff(A.row_ptr).max())}, cap {mc.spmm_cap(K)}, kernel {dA.spmm_kernel()}")
        dA.free()


@pytest.mark.parametrize("rp64", [False, True])
def test_a_chunk_above_4096_takes_the_serial_fallback(ctx, rp64):
    """Crosses chunk_nnz <= kSpmmMaxChunk = 4096 (bis_spmm_launch): a matrix of short rows whose row-block table was built
    under spmv_chunk = 8192 runs spmm_lane_serial_kernel, with the bits of the same matrix created under default options
    (the tiled kernel)."""
    rp = 64 if rp64 else 32
    rng = np.random.default_rng(12)
    n = 9000
    lens = rng.integers(0, 9, n)
    rows = np.repeat(np.arange(n), lens)
    col = np.clip(rows + rng.integers(-40, 41, len(rows)), 0, n - 1).astype(np.int32)  # unsorted, repeats allowed
    A = CRS(n, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), col, rng.uniform(-1, 1, len(rows)))
    X = rng.uniform(-1, 1, (n, 8))
    seq = [sequential_rows(A, X[:, j]) for j in range(8)]
    d0 = upload(ctx, A, rp64)
    with OptionScope(ctx, spmv_chunk=8192):
        d1 = upload(ctx, A, rp64)
    for k in (2, 3, 8):
        Xk = np.ascontiguousarray(X[:, :k])
        Y0 = spmm_checked(ctx, d0, Xk, k)
        assert d0.spmm_kernel() == f"spmm_rowblock_kernel K={k} V={2 if k % 2 == 0 else 1} RP={rp}"
        Y1 = spmm_checked(ctx, d1, Xk, k)
        assert d1.spmm_kernel() == f"spmm_lane_serial_kernel K={k} RP={rp}", d1.spmm_kernel()
        assert same_bits(Y1, Y0), (k, rp)
        for j in range(k):
            assert same_bits(Y1[:, j], seq[j]), (k, j)
    d0.free(); d1.free()


@pytest.mark.parametrize("rp64", [False, True])
def test_row_blocks_without_entries(ctx, rp64):
    """Crosses the row-block table's chunk with rows alone (block k starts at the first row r with row_ptr[r] + r >= k chunk):
    6,000 consecutive empty rows between populated ones make whole blocks with n_r > 0 and no entry (z == a: phase 1 is
    skipped); an all-empty matrix of 5,000 rows is made of such blocks only.  Y is exactly +0.0 there."""
    rng = np.random.default_rng(13)
    lens = np.concatenate([rng.integers(1, 7, 700), np.zeros(6000, dtype=np.int64), rng.integers(1, 7, 900)])
    n = len(lens)
    rows = np.repeat(np.arange(n), lens)
    col = rng.integers(0, n, len(rows)).astype(np.int32)
    A = CRS(n, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), col, rng.uniform(-1, 1, len(rows)))
    E = CRS(5000, np.zeros(5001, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0), n_cols=300)
    zero = np.zeros(1).view(np.uint64)[0]
    for M, empty in ((A, slice(700, 6700)), (E, slice(0, 5000))):
        dM = upload(ctx, M, rp64)
        X = rng.uniform(-1, 1, (M.n_cols, 8))
        ref = spmv_columns(ctx, dM, X) if M.nnz else None
        seq = [sequential_rows(M, X[:, j]) for j in range(8)]
        for k in (2, 5, 8):
            Y = spmm_checked(ctx, dM, np.ascontiguousarray(X[:, :k]), k)  # Y starts as NaN, the guard behind it is checked
            assert dM.spmm_kernel().startswith(f"spmm_rowblock_kernel K={k}"), dM.spmm_kernel()
            assert np.all(Y[empty].view(np.uint64) == zero), "an empty row is not +0.0"
            for j in range(k):
                assert same_bits(Y[:, j], seq[j]), (k, j)
                if ref is not None:
                    assert same_bits(Y[:, j], ref[j]), (k, j)
        dM.free()
