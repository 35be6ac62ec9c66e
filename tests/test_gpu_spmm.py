"""GPU: bis_spmm (Y = A X for k interleaved vectors) -- column j equals bis_spmv on column j bit for bit, rows too long for
the LDS tile take the serial fallback in the same summation order, argument checks, the byte model, the column copies."""
import numpy as np
import pytest

from helpers import OptionScope, check_rows, random_spmv_case, spmv_catalogue_case, spmv_catalogue_x
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 7.25


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


def device_crs(dA):
    rp, col, val = dA.download()
    return CRS(dA.n_rows, rp, col, val, n_cols=dA.n_cols)


def identity_cases(ctx):
    """(tag, device matrix, host CRS, X with 8 columns) -- matrices are created under the options in effect when called."""
    rng = np.random.default_rng(2024)
    for tag, gen in (("hpcg 16x12x10", lambda: ctx.gen_hpcg(16, 12, 10)), ("anderson 14", lambda: ctx.gen_anderson(14, shift=9.0)),
                     ("fem 6x5x4", lambda: ctx.gen_fem(6, 5, 4))):
        dA = gen()
        yield tag, dA, device_crs(dA), rng.uniform(-1, 1, (dA.n_cols, 8))
    for seed in (3, 7, 11):  # rectangular, empty rows, repeated columns; 64-bit row pointers where the case asks for them
        A, _, rp64, info = random_spmv_case(seed)
        with OptionScope(ctx, force_rp64=rp64 if rp64 else -1):
            dA = ctx.matrix(A)
        assert dA.rp_width == (8 if rp64 else 4)
        yield f"random{seed} {info}", dA, A, rng.uniform(-1, 1, (A.n_cols, 8))
    for name in ("blocks7", "blocks9", "blocks17"):  # rows that straddle row-block boundaries
        A, rp64 = spmv_catalogue_case(name, None)
        with OptionScope(ctx, force_rp64=rp64 if rp64 else -1):
            dA = ctx.matrix(A)
        yield name, dA, A, np.stack([spmv_catalogue_x(A, seed=j) for j in range(8)], axis=1)
    n = 3000  # a triangle with empty rows: the first five, every third, a run in the middle
    lens = rng.integers(1, 9, n)
    lens[:5] = 0
    lens[::3] = 0
    lens[1500:1600] = 0
    lens = np.minimum(lens, np.arange(n))
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(r, int(lens[r]), replace=False)) for r in range(n)]).astype(np.int32)
    A = CRS(n, rp, col, rng.uniform(-1, 1, rp[-1]))
    X = np.stack([spmv_catalogue_x(A, seed=10 + j) for j in range(8)], axis=1)  # (the last columns are unreferenced: Inf / NaN there)
    yield "empty rows L", ctx.matrix(A), A, X
    A = CRS(1, np.array([0, 0], dtype=np.int64), np.zeros(0, np.int32), np.zeros(0))
    yield "n = 1, empty row", ctx.matrix(A), A, rng.uniform(-1, 1, (1, 8))


def spmm_checked(ctx, dA, Xk, k, x_offset=0):
    """bis_spmm into a NaN-filled Y with a guard behind it; checks the guard and that X came back unchanged."""
    n_rows = dA.n_rows
    buf = ctx.upload(np.concatenate([np.full(n_rows * k, np.nan), np.full(GUARD, FILL)]))
    xbuf = ctx.upload(np.concatenate([np.zeros(x_offset), Xk.ravel()]))
    dX = xbuf.offset(x_offset, Xk.size)
    ctx.spmm(dA, dX, buf.offset(0, n_rows * k), k)
    out = buf.to_host()
    assert np.array_equal(out[n_rows * k:], np.full(GUARD, FILL)), "guard behind Y overwritten"
    assert np.array_equal(dX.to_host().view(np.uint64), Xk.ravel().view(np.uint64)), "X changed"
    buf.free()
    xbuf.free()
    return out[:n_rows * k].reshape(n_rows, k)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("scope", ["default", "rowblock partner"])
def test_column_identity_with_spmv(ctx, scope):
    opts = {} if scope == "default" else dict(spmv_win8=0, spmv_valdict=0)
    with OptionScope(ctx, **opts):
        for tag, dA, A, X in identity_cases(ctx):
            dy = ctx.alloc(max(A.n_rows, 1))
            ref = []
            for j in range(8):
                dx = ctx.upload(X[:, j])
                ctx.spmv(dA, dx, dy)
                ref.append(dy.to_host()[:A.n_rows])
                dx.free()
            assert dA.spmv_kernel() != "spmv_wave_per_row_kernel", tag
            assert dA.spmm_kernel() == ""
            for k in range(1, 9):
                Xk = np.ascontiguousarray(X[:, :k])
                Y = spmm_checked(ctx, dA, Xk, k)
                name = dA.spmm_kernel()
                assert name and f"K={k}" in name, (tag, k, name)
                if k > 1:
                    assert name.startswith("spmm_rowblock_kernel"), (tag, k, name)
                    assert f"RP={8 * dA.rp_width}" in name and (" V=2" if k % 2 == 0 else " V=1") in name, (tag, k, name)
                for j in range(k):
                    assert np.array_equal(Y[:, j], ref[j]) and same_bits(Y[:, j], ref[j]), (tag, k, j)
                if k in (2, 8) and tag.startswith("fem"):  # X only 8-byte aligned: the 8-byte gathers, same bits
                    Y1 = spmm_checked(ctx, dA, Xk, k, x_offset=1)
                    assert " V=1" in dA.spmm_kernel()
                    assert same_bits(Y1, Y), (tag, k)
            dy.free()
            dA.free()


@pytest.mark.parametrize("shuffled", [False, True])
def test_long_rows_take_the_serial_fallback_in_order(ctx, shuffled):
    rng = np.random.default_rng(5 + shuffled)
    n_cols = 40000
    rows = []
    for length in (20000, 9000, 1, 0):
        c = rng.choice(n_cols, length, replace=False)
        rows.append(c if shuffled else np.sort(c))
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int64)
    A = CRS(4, rp, np.concatenate(rows).astype(np.int32), rng.uniform(-1, 1, rp[-1]), n_cols=n_cols)
    dA = ctx.matrix(A)
    for k in (3, 8):
        X = rng.uniform(-1, 1, (n_cols, k))
        Y = spmm_checked(ctx, dA, X, k)
        assert dA.spmm_kernel() == f"spmm_lane_serial_kernel K={k} RP=32"
        for j in range(k):
            for r in range(4):
                p = A.val[rp[r]:rp[r + 1]] * X[A.col[rp[r]:rp[r + 1]], j]
                want = np.cumsum(p)[-1] if len(p) else 0.0  # the sequential left-to-right sum of the rounded products
                assert Y[r, j] == want, (k, j, r)
            check_rows(Y[:, j], A, np.ascontiguousarray(X[:, j]), tag=f"long rows k={k} j={j}")
    dA.free()


def test_argument_checks_and_byte_model(ctx):
    from basic_iterative_solvers_amd import BisError
    A, _, _, _ = random_spmv_case(7)
    for rp64 in (0, 1):
        with OptionScope(ctx, force_rp64=rp64 if rp64 else -1):
            dA = ctx.matrix(A)
        w = 8 if rp64 else 4
        assert dA.rp_width == w
        for k in range(1, 9):
            assert dA.spmm_streamed_bytes(k) == 12 * A.nnz + w * (A.n_rows + 1) + 8 * k * (A.n_cols + A.n_rows)
        for k in (0, 9):
            with pytest.raises(BisError):
                dA.spmm_streamed_bytes(k)
        dX, dY = ctx.alloc(A.n_cols * 8), ctx.alloc(A.n_rows * 8)
        for k in (0, 9):
            with pytest.raises(BisError, match="status 2"):  # BIS_ERR_INVALID
                ctx.spmm(dA, dX, dY, k)
        with pytest.raises(BisError, match="status 2"):
            ctx.spmm(dA, dX, dX, 4)
        dX.free(); dY.free(); dA.free()


@pytest.mark.parametrize("n", [1921, 1])
@pytest.mark.parametrize("k", [3, 8])
def test_mvec_columns_round_trip(ctx, n, k):
    rng = np.random.default_rng(n + k)
    base = rng.uniform(-1, 1, (n, k))
    dX = ctx.upload(base.ravel())
    dv, dw = ctx.alloc(n), ctx.alloc(n)
    want = base.copy()
    for j in range(k):
        v = rng.uniform(-1, 1, n)
        v[0] = -0.0
        dv.set(v)
        ctx.mvec_set_col(dX, n, k, j, dv)
        want[:, j] = v
        assert same_bits(dX.to_host().reshape(n, k), want), j  # column j set, every other column's bits alone
        ctx.mvec_get_col(dw, dX, n, k, j)
        assert same_bits(dw.to_host(), v), j
    dX.free(); dv.free(); dw.free()
