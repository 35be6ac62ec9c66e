"""GPU: single-precision preconditioner storage -- bis_mat_round_f32 and the SpMV form "win4" (bis_spmv_win8.hip, public
form 8): win8's window + sliced-ELL plan with 4-byte values, only for a matrix the call has flagged fp32-exact.

The rounding is held to numpy's float32 conversion bit for bit (ties, subnormals, signed zeros, the largest float, an
overflow that must leave the matrix untouched).  The form is held to the project's gate for every SpMV form: on the rounded
matrix y is BIT-IDENTICAL to win8 (spmv_win4 = 0) and to the row-block kernel on the CRS arrays (spmv_win8 = 0), and within
1e-13 of the oracle on the scale |A| |x|.  Nothing changes for a matrix nobody rounded; scaling and retuning clear the flag.
The consumers that follow: the fused CG, bis_itrsv, the FSAI apply (single and multi-vector) and CG with rounded FSAI
factors against a numpy PCG on the downloaded rounded factor.

A row-range view cannot be built through the public interface, so bis_mat_round_f32's refusal of one has no test here
(the null matrix, the other BIS_ERR_INVALID case, has).  The implied-slot layout is built where at least half of the chunks
lie in slices of 64 rows of one length with common window offsets: hpcg 12x10x9 (1080 rows, 20 slices, most with boundary
rows) does not reach that with either value width, so the "implied by default, explicit with spmv_win8_implicit 0" check
runs on hpcg 40x24x20 (the smallest case of tests/test_gpu_win8_implicit.py), and every case checks that win4's layout
record equals win8's on the same matrix."""
import numpy as np
import pytest
import scipy.sparse as sp

from helpers import hist_dev
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu
KTOL = 1e-13
F32_MAX = 3.4028234663852886e38  # (2 - 2^-23) 2^127
OPTS = ("force_rp64", "spmv_valdict", "spmv_win8_rows", "spmv_win8_depth", "spmv_win8", "spmv_win4", "spmv_win8_implicit", "spmv_win8_tune")


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    yield c
    c.close()


def _reset(ctx):
    for k in OPTS:
        ctx.set_option(k, -1)


def f32(val):
    """numpy's round-to-nearest-even conversion to binary32 and back (an overflow becomes an infinity)"""
    with np.errstate(over="ignore"):
        return np.asarray(val, dtype=np.float64).astype(np.float32).astype(np.float64)


def rounded(A):
    return CRS(A.n_rows, A.row_ptr, A.col, f32(A.val), n_cols=A.n_cols)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_y(a, b):
    """bit for bit, or the same values with the same signs where NaNs sit in the same places (the win8 test's rule)"""
    return same_bits(a, b) or (np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b)))


def banded(rng, n, offsets, max_len, ragged=4, empty_every=53, n_cols=None, special=True):
    n_cols = n_cols or n
    lens = rng.integers(max(max_len - ragged, 0), max_len + 1, n)
    if empty_every:
        lens[::empty_every] = 0
    rp = np.concatenate([[0], np.cumsum(lens)])
    rows = np.repeat(np.arange(n), lens)
    col = np.clip(rows + rng.choice(offsets, rp[-1]), 0, n_cols - 1).astype(np.int32)
    val = rng.uniform(-3, 3, rp[-1])
    if special and rp[-1] > 8:  # (finite in binary32: the catalogue is rounded before it is uploaded)
        val[:8] = [-0.0, 0.0, 5e-324, -1.0, 26.0, F32_MAX, -F32_MAX, 1.0 + 2.0 ** -52]
    return CRS(n, rp, col, val, n_cols=n_cols)


def _two_populations(rng, n=30000):
    lens = rng.integers(0, 9, n)
    lens[::64] = 200
    rp = np.concatenate([[0], np.cumsum(lens)])
    rows = np.repeat(np.arange(n), lens)
    col = np.clip(rows + rng.integers(-300, 301, rp[-1]), 0, n - 1).astype(np.int32)
    return n, rp, col, rng.uniform(-1, 1, rp[-1])


def randomised(A, rng):
    return CRS(A.n_rows, A.row_ptr, A.col, rng.uniform(-2, 2, A.nnz), n_cols=A.n_cols)


def catalogue(oracle, rng):
    """(name, matrix, form expected where the window plan is known to apply -- None: whatever win8 gets)"""
    offs_band = np.arange(-40, 41)
    offs_runs = np.concatenate([np.arange(-3, 4), np.arange(-3, 4) + 700, np.arange(-3, 4) - 700, np.arange(-3, 4) + 5000, np.arange(-3, 4) - 5000])
    neg0 = CRS(300, np.arange(0, 301 * 3, 3), np.repeat(np.arange(300), 3).astype(np.int32), np.tile([-1.0, 0.0, -0.0], 300))
    return [("hpcg 12x10x9, random values", randomised(oracle.gen_hpcg(12, 10, 9), rng), True),
            ("hpcg 40x24x20, random values (implied slots)", randomised(oracle.gen_hpcg(40, 24, 20), rng), True),
            ("fem 6x5x4", oracle.gen_fem(6, 5, 4), None),
            ("fem 10x9x8", oracle.gen_fem(10, 9, 8), None),
            ("band", banded(rng, 9001, offs_band, 27), True),
            ("five runs", banded(rng, 20011, offs_runs, 18, special=False), True),
            ("rectangular", banded(rng, 3000, np.arange(0, 300), 9, n_cols=3300, special=False), True),
            ("long rows", banded(rng, 2000, np.arange(-100, 101), 70, special=False), True),
            ("ragged rows", banded(rng, 40000, offs_band, 30, ragged=30), None),
            ("rows of 0..8 entries among rows of 200", CRS(*_two_populations(rng)), None),
            ("-0.0 sums", neg0, True), ("one row", CRS(1, [0, 2], [0, 0], [2.0, 3.0]), True)]


def scattered(rng):
    return CRS(9000, np.arange(0, 9001 * 12, 12), rng.integers(0, 9000, 9000 * 12).astype(np.int32), rng.uniform(-1, 1, 9000 * 12))


def layout_bytes(dA, A):
    """bis_mat_spmv_streamed_bytes of form 8 by the layout's formula: chunks of 1536 bytes, or 1024 bytes of values plus the
    descriptors and slot records with implied slots; block headers, length order, slice offsets; x and y once"""
    ch, ex, sl, bl, implied = dA.win8_layout()
    R = sl // (4 * bl)
    meta = bl * (8 * 64 + 2 * 256 * R) + 8 * (sl + 1)
    own = (1024 * ch + 8 * (ch - ex) + 512 * ex + meta + 8 * (sl + 1)) if implied else (1536 * ch + meta)
    return 8 * A.n_cols + 8 * A.n_rows + own


# ---- 1. the rounding -------------------------------------------------------------------------------------------------

def _special_matrix(rng, extra=()):
    special = [-0.0, 0.0, 5e-324, 1e-40, -1e-40, 1.0 + 2.0 ** -52, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, -(1.0 + 2.0 ** -24),
               3.4028234e38, F32_MAX, -F32_MAX, 2.0 ** -149, 2.0 ** -150, 1.5 * 2.0 ** -149, np.inf, -np.inf, np.nan] + list(extra)
    n = 3000
    lens = rng.integers(0, 12, n)
    rp = np.concatenate([[0], np.cumsum(lens)])
    val = rng.uniform(-3, 3, rp[-1]) * 10.0 ** rng.integers(-30, 30, rp[-1])
    pos = rng.choice(rp[-1], len(special), replace=False)
    val[pos] = special
    col = rng.integers(0, n, rp[-1]).astype(np.int32)
    return CRS(n, rp, col, val)


@pytest.mark.parametrize("rp64", [0, 1])
def test_rounding_is_numpys(ctx, rp64):
    rng = np.random.default_rng(41 + rp64)
    A = _special_matrix(rng)
    want = f32(A.val)
    assert want[np.where(A.val == 5e-324)[0][0]] == 0.0 and 1.0 in want and (1.0 + 2.0 ** -22) in want  # the ties went to even
    finite = np.isfinite(A.val) & (A.val != 0.0)
    change = np.max(np.abs(want[finite] - A.val[finite]) / np.abs(A.val[finite]))
    assert change == 1.0  # (5e-324 -> 0)
    ctx.set_option("force_rp64", rp64)
    try:
        dA = ctx.matrix(A)
        assert dA.rp_width == (8 if rp64 else 4)
        got_change = dA.round_f32()
        rp, col, val = dA.download()
        assert same_bits(val, want)
        assert np.array_equal(rp, A.row_ptr) and np.array_equal(col, A.col)
        assert got_change == change
        assert dA.round_f32() == 0.0  # idempotent
        assert same_bits(dA.download()[2], want)
        # without the value that loses everything: the change of an ordinary entry, at most half an ulp of binary32
        B = CRS(A.n_rows, A.row_ptr, A.col, np.where(np.abs(A.val) < 1e-37, 0.5, A.val))
        wb = f32(B.val)
        fin = np.isfinite(B.val)
        cb = np.max(np.abs(wb[fin] - B.val[fin]) / np.abs(B.val[fin]))
        dB = ctx.matrix(B)
        assert dB.round_f32() == cb and 0.0 < cb <= 2.0 ** -24
        assert same_bits(dB.download()[2], wb)
        dA.free(); dB.free()
    finally:
        _reset(ctx)


def test_overflow_is_refused_and_leaves_the_matrix_alone(ctx):
    from basic_iterative_solvers_amd import BisError
    A = _special_matrix(np.random.default_rng(43), extra=[1.7976931348623157e308, -3.5e38])
    dA = ctx.matrix(A)
    x = ctx.upload(np.ones(A.n_cols))
    y = ctx.alloc(A.n_rows)
    ctx.spmv(dA, x, y)  # (forms built before the call stay valid after a refusal)
    with pytest.raises(BisError, match="status 6"):
        dA.round_f32()
    assert same_bits(dA.download()[2], A.val)
    ctx.set_option("spmv_valdict", 0)
    try:
        assert dA.spmv_stream_info()[1] == 8  # not flagged
    finally:
        _reset(ctx)
    dA.free(); x.free(); y.free()


def test_bad_arguments_and_the_empty_matrix(ctx):
    import ctypes as C
    m = C.c_double(-7.0)
    assert ctx.lib.bis_mat_round_f32(ctx.h, None, C.byref(m)) == 2  # BIS_ERR_INVALID
    assert ctx.lib.bis_mat_round_f32(None, None, None) == 1  # BIS_ERR_NO_DEVICE
    E = ctx.matrix(CRS(5, np.zeros(6, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0)))
    assert E.round_f32() == 0.0
    A = ctx.matrix(CRS(1, [0, 2], [0, 0], [2.0, 3.0]))
    assert ctx.lib.bis_mat_round_f32(ctx.h, A.h, None) == 0  # the result pointer may be null
    E.free(); A.free()


# ---- 2. bit identity -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rp64,rows,depth", [(0, 1, 4), (0, 2, 4), (1, 2, 2), (0, 4, 3), (1, 1, 6), (0, 2, 6)])
def test_win4_is_bit_identical_to_win8_and_the_rowblock_kernel(ctx, oracle, rp64, rows, depth):
    rng = np.random.default_rng(700 + rows + 10 * rp64)
    ctx.set_option("force_rp64", rp64)
    ctx.set_option("spmv_valdict", 0)
    ctx.set_option("spmv_win8_rows", rows)
    ctx.set_option("spmv_win8_depth", depth)
    try:
        for name, A0, want in catalogue(oracle, rng):
            A = rounded(A0)
            x = rng.uniform(-1, 1, A.n_cols)
            if name == "-0.0 sums":
                x[:] = 0.0
                x[::2] = -0.0
            dx, dy = ctx.upload(x), ctx.alloc(A.n_rows)
            dx1 = ctx.upload(np.concatenate([[7.0], x]))
            ys = {}
            for implicit in (-1, 0):
                ctx.set_option("spmv_win8_implicit", implicit)
                dA = ctx.matrix(A)
                assert dA.round_f32() == 0.0, name  # (rounded on the host already: the call only sets the flag)
                for form, opts in ((8, {}), (6, {"spmv_win4": 0}), (0, {"spmv_win8": 0})):
                    for k, v in opts.items():
                        ctx.set_option(k, v)
                    info = dA.spmv_stream_info()
                    if want or form == 0:
                        assert info[3] == form, (name, form, info)
                    ctx.init_vector(dy, float("nan"))
                    ctx.spmv(dA, dx, dy)
                    ys[implicit, form] = (dy.to_host(), info, dA.spmv_kernel(), dA.win8_layout())
                    if form == 8 and info[3] == 8:
                        ch, ex, sl, bl, implied = dA.win8_layout()
                        assert info == (2, 4, 0, 8), (name, info)
                        assert dA.spmv_kernel() == f"win4 rows={sl // (4 * bl)}", (name, dA.spmv_kernel())
                        assert dA.spmv_streamed_bytes() == layout_bytes(dA, A), name
                        if "implied slots" in name:
                            assert implied == (implicit != 0), (name, implicit, dA.win8_layout())
                        if implicit == 0:
                            assert not implied and ex == ch
                        ctx.init_vector(dy, 3.0)  # an x that is only 8-byte aligned: the window is filled through registers
                        ctx.spmv(dA, dx1.offset(1), dy)
                        assert same_y(dy.to_host(), ys[implicit, 8][0]), name
                        ctx.spmv(dA, dx, dy)  # a second product on the built form
                        assert same_y(dy.to_host(), ys[implicit, 8][0]), name
                    for k in opts:
                        ctx.set_option(k, -1)
                dA.free()
                # win4 exactly where win8: the plan is the same one
                assert (ys[implicit, 8][1][3] == 8) == (ys[implicit, 6][1][3] == 6), (name, ys[implicit, 8][1], ys[implicit, 6][1])
                if ys[implicit, 6][1][3] == 6:
                    assert ys[implicit, 6][1][1] == 8 and ys[implicit, 6][2].startswith("win8 rows="), name
                    # the same plan and the same (value-free) classification of the slices: chunks, slot records, slices, blocks, layout
                    assert ys[implicit, 8][3] == ys[implicit, 6][3], (name, ys[implicit, 8][3], ys[implicit, 6][3])
                assert same_y(ys[implicit, 8][0], ys[implicit, 6][0]), (name, implicit)
                assert same_y(ys[implicit, 8][0], ys[implicit, 0][0]), (name, implicit)
            assert same_y(ys[-1, 8][0], ys[0, 8][0]), name
            if np.all(np.abs(A.val) < 1e6):
                yo = oracle.spmv(A, x)
                scale = max(np.abs(A.to_scipy()).dot(np.abs(x)).max(), 1e-300)
                assert np.max(np.abs(ys[-1, 8][0] - yo)) <= KTOL * scale, name
            dx.free(); dy.free(); dx1.free()
        S = rounded(scattered(rng))
        dS = ctx.matrix(S)
        dS.round_f32()
        assert dS.spmv_stream_info()[3] == 0 and dS.spmv_stream_info()[1] == 8
        dS.free()
    finally:
        _reset(ctx)


@pytest.mark.parametrize("n1,rows", [(81, 2), (102, 4)])
def test_win4_blocks_of_512_and_1024_rows(ctx, n1, rows):
    """Blocks of 512 / 1024 rows are only built for matrices of at least 1024 such blocks: the generated HPCG operator of the
    smallest such size (its values 26 and -1 are exact in binary32), without its dictionary.  Plain and fused products."""
    ctx.set_option("spmv_valdict", 0)
    ctx.set_option("spmv_win8_rows", rows)
    try:
        dA = ctx.gen_hpcg(n1)
        n = dA.n_rows
        assert dA.spmv_stream_info()[3] == 6  # not flagged: today's form
        assert dA.round_f32() == 0.0
        x = ctx.upload(np.random.default_rng(n1).uniform(-1, 1, n))
        y = ctx.alloc(n)
        out = {}
        for form, opts in ((8, {}), (6, {"spmv_win4": 0}), (0, {"spmv_win8": 0})):
            for k, v in opts.items():
                ctx.set_option(k, v)
            assert dA.spmv_stream_info()[3] == form
            ctx.spmv(dA, x, y)
            b, x0 = ctx.alloc(n), ctx.alloc(n)
            ctx.init_vector(b, 1.0); ctx.init_vector(x0, 0.1)
            cg = ctx.cg(dA, b, x0)  # three iterations of the fused (Ap, p) product
            cg.init(1e-14)
            cg.iterate(3)
            hist = np.array(cg.status()[2])
            out[form] = (y.to_host(), hist, dA.spmv_kernel(), dA.spmv_kernel(fused=True))
            cg.free(); b.free(); x0.free()
            for k in opts:
                ctx.set_option(k, -1)
        assert out[8][2] == out[8][3] == f"win4 rows={rows}" and out[6][2] == out[6][3] == f"win8 rows={rows}", (out[8][2:], out[6][2:])
        assert dA.win8_layout()[4]
        assert same_bits(out[8][0], out[6][0]) and same_bits(out[8][0], out[0][0])
        assert len(out[8][1]) >= 3 and same_bits(out[8][1], out[6][1])  # the same partials, summed in the same order
        dA.free(); x.free(); y.free()
    finally:
        _reset(ctx)


# ---- 3. no silent change ---------------------------------------------------------------------------------------------

def test_nothing_changes_for_a_matrix_nobody_rounded(ctx, oracle):
    rng = np.random.default_rng(77)
    ctx.set_option("spmv_valdict", 0)
    try:
        for name, A0, want in catalogue(oracle, rng):
            if not want:
                continue
            for A in (A0, rounded(A0)):  # unrounded; already exact in binary32 but never flagged
                dA = ctx.matrix(A)
                info = dA.spmv_stream_info()
                assert info == (2, 8, 0, 6), (name, info)
                dA.free()
    finally:
        _reset(ctx)


def _hpcg_random_diagonal(oracle, n, seed):
    """the HPCG operator plus a random non-negative diagonal: SPD, arbitrary values (no dictionary form)"""
    A = oracle.gen_hpcg(*n) if isinstance(n, tuple) else oracle.gen_hpcg(n)
    rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
    val = A.val.copy()
    val[A.col == rows] += np.random.default_rng(seed).uniform(0, 1, A.n_rows)
    return CRS(A.n_rows, A.row_ptr, A.col, val)


def test_scaling_and_retuning_clear_the_flag(ctx, oracle):
    A = rounded(_hpcg_random_diagonal(oracle, 8, 4))
    rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
    xh = np.random.default_rng(5).uniform(-1, 1, A.n_rows)
    ctx.set_option("spmv_valdict", 0)
    try:
        for what in ("scale_sym", "retune"):
            dA = ctx.matrix(A)
            dA.round_f32()
            dx, dy = ctx.upload(xh), ctx.alloc(A.n_rows)
            ctx.spmv(dA, dx, dy)
            assert dA.spmv_stream_info()[3] == 8
            if what == "scale_sym":
                sv = ctx.scale_sym(dA).to_host()
                B = CRS(A.n_rows, A.row_ptr, A.col, A.val * (sv[rows] * sv[A.col]))  # a_rc *= (s_r * s_c), as the device does it
                assert not np.array_equal(f32(B.val), B.val)  # the scaled values are not binary32 numbers: a stale flag would show
            else:
                dA.retune()
                B = A
            ctx.spmv(dA, dx, dy)
            assert dA.spmv_stream_info() == (2, 8, 0, 6), what
            assert dA.spmv_kernel().startswith("win8 rows="), what
            assert same_bits(dA.download()[2], B.val)
            assert np.max(np.abs(dy.to_host() - oracle.spmv(B, xh))) <= KTOL * np.abs(B.to_scipy()).dot(np.abs(xh)).max(), what
            assert dA.round_f32() >= 0.0 and dA.spmv_stream_info()[3] == 8  # the caller rounds again
            dA.free(); dx.free(); dy.free()
    finally:
        _reset(ctx)


# ---- 4. the fused CG -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [1, 2, 4])
def test_win4_in_fused_cg(ctx, oracle, rows):
    A = rounded(_hpcg_random_diagonal(oracle, 20, 3))
    n = A.n_rows
    ctx.set_option("spmv_valdict", 0)
    ctx.set_option("spmv_win8_rows", rows)
    try:
        dA = ctx.matrix(A)
        dA.round_f32()
        assert dA.spmv_stream_info()[3] == 8
        b, x = ctx.alloc(n), ctx.alloc(n)
        ctx.init_vector(b, 1.0); ctx.init_vector(x, 0.1)
        cg = ctx.cg(dA, b, x)
        cg.init(1e-14)
        cg.iterate(80)
        iters, conv, hist = cg.status(hist_cap=128)
        assert dA.spmv_kernel(fused=True).startswith("win4 rows="), dA.spmv_kernel(fused=True)
        ref = oracle.solve(A, "cg", "none")
        m = min(len(ref["hist"]), len(hist))
        dev = np.max(np.abs(ref["hist"][:m] - np.array(hist)[:m])) / ref["hist"][0]
        print(f"rows {rows}: {iters} iterations (oracle {ref['iters']}), history deviation {dev:.3e} r0")
        assert dev <= 1e-10
        assert abs(iters - ref["iters"]) <= 1
        cg.free(); dA.free(); b.free(); x.free()
    finally:
        _reset(ctx)


# ---- 5. bis_itrsv ----------------------------------------------------------------------------------------------------

def _spd_band(rng, n=9001, half=12):
    """a symmetric band with a dominant diagonal: rows of up to 2 half + 1 entries, ascending columns"""
    rows = np.repeat(np.arange(n), 8)
    cols = np.clip(rows + rng.integers(1, half + 1, rows.size), 0, n - 1)
    keep = cols != rows
    M = sp.coo_matrix((rng.uniform(-1, 0, keep.sum()), (rows[keep], cols[keep])), shape=(n, n)).tocsr()
    M = M + M.T
    M = (M + sp.diags(np.asarray(abs(M).sum(axis=1)).ravel() + rng.uniform(0.5, 1.5, n))).tocsr()
    M.sum_duplicates(); M.sort_indices()
    return CRS(n, M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data.copy())


@pytest.mark.parametrize("name", ["fem 6x5x4", "band"])
def test_itrsv_on_flagged_triangles(ctx, oracle, name):
    rng = np.random.default_rng(90)
    ctx.set_option("spmv_valdict", 0)
    try:
        dA = ctx.gen_fem(6, 5, 4) if name.startswith("fem") else ctx.matrix(_spd_band(rng))
        n = dA.n_rows
        Ls, L_D, Us, U_D = ctx.ilu0(dA)
        Uinv = ctx.alloc(n)
        ctx.elemwise_div_vectors(Uinv, L_D, U_D)
        b = rng.uniform(-1, 1, n)
        db, x, work = ctx.upload(b), ctx.alloc(n), ctx.alloc(n)
        for T, Dinv in ((Ls, L_D), (Us, Uinv)):
            change = T.round_f32()
            assert 0.0 < change <= 2.0 ** -24
            assert T.spmv_stream_info() == (2, 4, 0, 8), (name, T.spmv_stream_info())
            for k in range(5):
                ctx.itrsv(T, Dinv, db, x, work, k)
                got = x.to_host()
                if k:
                    assert T.itrsv_kernel() == "itrsv spmv+epilogue form=8", (name, k, T.itrsv_kernel())
                ctx.set_option("spmv_win4", 0)
                ctx.itrsv(T, Dinv, db, x, work, k)
                if k:
                    assert T.itrsv_kernel() == "itrsv spmv+epilogue form=6", (name, k, T.itrsv_kernel())
                ctx.set_option("spmv_win4", -1)
                assert same_bits(got, x.to_host()), (name, k)
                assert np.all(np.isfinite(got)) and np.any(got != 0.0)
        for v in (dA, Ls, Us, L_D, U_D, Uinv, db, x, work):
            v.free()
    finally:
        _reset(ctx)


# ---- 6. FSAI ---------------------------------------------------------------------------------------------------------

CG_TOL = 1e-10


def host_csr(dM):
    rp, col, val = dM.download()
    return sp.csr_matrix((val, col, rp), shape=(dM.n_rows, dM.n_cols))


def numpy_pcg(A, G, b, tol, max_iters):
    """Preconditioned CG with M^-1 = G^T G (scipy CSR matrices), x0 = 0: the residual history."""
    Gt = G.T.tocsr()
    x, r = np.zeros_like(b), b.copy()
    z = Gt @ (G @ r)
    p, rz = z.copy(), r @ z
    hist = [np.linalg.norm(r)]
    while len(hist) - 1 < max_iters and not hist[-1] < tol * hist[0]:
        Ap = A @ p
        alpha = rz / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        z = Gt @ (G @ r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
        hist.append(np.linalg.norm(r))
    return np.array(hist)


@pytest.fixture(scope="module")
def fsai_systems(ctx, oracle):
    """Per size, computed once and left alone: the SPD matrix, its FSAI factors rounded and flagged, the downloads of the
    factor before and after the rounding."""
    out = {}
    for key, n in (("12x10x9", (12, 10, 9)), ("20", 20)):
        A = _hpcg_random_diagonal(oracle, n, 6)
        dA = ctx.matrix(A)
        G, Gt, nf = ctx.fsai(dA)
        assert nf == 0
        G64 = host_csr(G)
        changes = (G.round_f32(), Gt.round_f32())
        out[key] = dict(A=A, dA=dA, G=G, Gt=Gt, G64=G64, G32=host_csr(G), Gt32=host_csr(Gt), changes=changes)
    return out


@pytest.mark.parametrize("key", ["12x10x9", "20"])
def test_rounded_fsai_factors(ctx, fsai_systems, key):
    e = fsai_systems[key]
    A, dA, G, Gt = e["A"], e["dA"], e["G"], e["Gt"]
    n = A.n_rows
    assert same_bits(e["G32"].data, f32(e["G64"].data)) and 0.0 < e["changes"][0] <= 2.0 ** -24 and e["changes"][0] == e["changes"][1]
    # rounding is elementwise: round(Gt) = round(G)^T bit for bit, so M^-1 = Gt G stays symmetric positive semidefinite
    T = e["G32"].T.tocsr()
    T.sort_indices()
    W = e["Gt32"].copy()
    W.sort_indices()
    assert np.array_equal(T.indptr, W.indptr) and np.array_equal(T.indices, W.indices) and same_bits(T.data, W.data)
    ctx.set_option("spmv_valdict", 0)
    try:
        assert G.spmv_stream_info()[3] == 8 and Gt.spmv_stream_info()[3] == 8
        As = A.to_scipy().tocsr()
        b = As @ np.ones(n)
        db, dx = ctx.upload(b), ctx.upload(np.zeros(n))
        cg = ctx.cg(dA, db, dx)
        cg.set_preconditioner("fsai", Ls=G, Us=Gt)
        cg.init(CG_TOL)
        cg.iterate(400)
        iters, conv, hist = cg.status()
        assert G.spmv_kernel().startswith("win4 rows=") and Gt.spmv_kernel().startswith("win4 rows=")
        ref32 = numpy_pcg(As, e["G32"], b, CG_TOL, 400)
        ref64 = numpy_pcg(As, e["G64"], b, CG_TOL, 400)
        dev = hist_dev(hist, ref32)
        res = np.linalg.norm(b - As @ dx.to_host())
        print(f"{key}: device {iters} iterations, numpy on the rounded G {len(ref32) - 1}, on the fp64 G {len(ref64) - 1}, "
              f"history deviation {dev:.3e} r0, true residual {res / ref32[0]:.3e} r0, max relative change {e['changes'][0]:.3e}")
        assert conv and ref32[-1] < CG_TOL * ref32[0]
        assert dev <= 1e-10
        assert abs(iters - (len(ref64) - 1)) <= 1
        cg.free(); db.free(); dx.free()
        # the multi-vector apply (bis_spmm on the fp64 CRS arrays, which hold the rounded values) against the single-vector one
        k = 3
        X = np.random.default_rng(12).uniform(-1, 1, (n, k))
        dX, dOut, dTmp = ctx.upload(X.ravel()), ctx.alloc(n * k), ctx.alloc(n * k)
        ctx.mapply_preconditioner("fsai", n, k, G, Gt, None, None, None, None, dOut, dX, dTmp, None)
        got = dOut.to_host().reshape(n, k)
        col, out, tmp = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
        for j in range(k):
            col.set(X[:, j].copy())
            ctx.apply_preconditioner("fsai", n, G, Gt, None, None, None, None, out, col, tmp, None)
            assert same_bits(got[:, j], out.to_host()), (key, j)
        assert G.spmv_kernel().startswith("win4 rows=")
        for v in (dX, dOut, dTmp, col, out, tmp):
            v.free()
    finally:
        _reset(ctx)


# ---- 7. placement ----------------------------------------------------------------------------------------------------

def test_win4_placement_search_and_its_record(ctx, oracle):
    """HPCG-160, the smallest size the search accepts (the size test stays on the fp64 stream's 2560 bytes per chunk): whichever
    allocation is kept holds the same stream, and bis_mat_win8_tuning reports the search on the 4-byte stream."""
    n1 = 160
    N = n1 ** 3
    x = ctx.upload(np.random.default_rng(8).uniform(-1, 1, N))
    ys = {}
    ctx.set_option("spmv_valdict", 0)
    try:
        for tune in (0, 4, -1):
            ctx.set_option("spmv_win8_tune", tune)
            dA = ctx.gen_hpcg(n1)
            assert dA.round_f32() == 0.0  # 26 and -1: the call sets the flag
            y = ctx.alloc(N)
            ctx.spmv(dA, x, y)
            assert dA.spmv_stream_info() == (2, 4, 0, 8)
            trials, first_ms, kept_ms = dA.win8_tuning()
            print(f"spmv_win8_tune {tune}: {trials} re-allocation(s), {first_ms:.4f} ms on the first allocation, {kept_ms:.4f} ms kept")
            if tune == 0:
                assert (trials, first_ms, kept_ms) == (0, 0.0, 0.0)
            else:
                assert 0 <= trials <= (4 if tune == 4 else 12) and first_ms > 0 and 0 < kept_ms <= first_ms
            ys[tune] = y.to_host()
            dA.free(); y.free()
        assert np.array_equal(ys[0], ys[4]) and np.array_equal(ys[0], ys[-1])
        A = oracle.gen_hpcg(n1, row0=1000000, row1=1050000)
        yo = oracle.spmv(A, x.to_host())
        assert np.max(np.abs(ys[-1][1000000:1050000] - yo)) <= KTOL * np.max(np.abs(yo))
    finally:
        _reset(ctx)
    x.free()
