"""GPU: win8 with implied window slots (option spmv_win8_implicit, bis_spmv_win8.hip).  Where all 64 rows of a slice have one
length and their window slots differ only by 8 (row - block_row0) bytes, the stream holds only the chunk's values (2048 bytes)
and a per-chunk descriptor of 4 slot bases; the other slices keep their 512 bytes of slots per chunk in a side array.  y must
be BIT-IDENTICAL to the row-block kernel on the CRS arrays (spmv_win8 = 0) and to today's layout (spmv_win8_implicit = 0):
HPCG sizes whose blocks end mid-slice and whose last block is partial, 1 / 2 / 4 rows per lane, 64-bit row pointers, an x
that is only 8-byte aligned, an x holding -0.0 / inf / NaN (the padding entries must still read the -0.0 slot), stencils with
a few perturbed rows (implicit and explicit slices in one block), and a matrix where nothing qualifies (today's layout and
bytes).  bis_mat_spmv_stream_info keeps col_bytes 2 for both layouts (0 names the row-mask form); bis_mat_win8_layout tells
them apart.  Also: the fused CG history, the placement search, the streamed-byte formula, the partitioned bench path and who
owns a stream that bis_mat_win8_debug_stream redirected."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = ("force_rp64", "spmv_valdict", "spmv_win8_rows", "spmv_win8", "spmv_win8_implicit", "spmv_win8_tune")


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    yield c
    c.close()


def _reset(ctx):
    for k in OPTS:
        ctx.set_option(k, -1)


def _randomised(A, rng):
    return CRS(A.n_rows, A.row_ptr, A.col, rng.uniform(-2, 2, A.nnz), n_cols=A.n_cols)


def _perturbed(A, rng, every=997):
    """the stencil with the first column of every `every`-th row moved by one: those rows' slices lose their common offsets"""
    col = A.col.copy()
    rows = np.arange(0, A.n_rows, every)
    k = A.row_ptr[rows]
    col[k] = np.clip(col[k] + 1, 0, A.n_cols - 1)
    return CRS(A.n_rows, A.row_ptr, col, rng.uniform(-2, 2, A.nnz), n_cols=A.n_cols)


def _ragged(rng, n=40000):
    """rows of 24..27 entries at random offsets in a band: win8 applies, but no slice has common offsets (nor, mostly, one
    length), so the implied-slot layout is not built"""
    lens = rng.integers(24, 28, n)
    rp = np.concatenate([[0], np.cumsum(lens)])
    rows = np.repeat(np.arange(n), lens)
    col = np.clip(rows + rng.integers(-40, 41, rp[-1]), 0, n - 1).astype(np.int32)
    return CRS(n, rp, col, rng.uniform(-1, 1, rp[-1]))


def _layout_bytes(dA, A):
    """bis_mat_spmv_streamed_bytes of form 6 by the layout's documented formula"""
    ch, ex, sl, bl, implied = dA.win8_layout()
    if bl == 0:
        return None
    R = sl // (4 * bl)
    meta = bl * (8 * 64 + 2 * 256 * R) + 8 * (sl + 1)
    own = (2048 * ch + 8 * (ch - ex) + 512 * ex + meta + 8 * (sl + 1)) if implied else (2560 * ch + meta)
    return 8 * A.n_cols + 8 * A.n_rows + own


def _same(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64)) or (
        np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b)))


def _products(ctx, A, xs, w8, implicit):
    """y = A x for every x of xs (and for xs[0] shifted to an 8-byte-aligned address), with the layout's record"""
    ctx.set_option("spmv_win8", w8)
    ctx.set_option("spmv_win8_implicit", implicit)
    dA = ctx.matrix(A)
    dy = ctx.alloc(A.n_rows)
    ys = []
    for x in xs:
        dx = ctx.upload(x)
        ctx.init_vector(dy, float("nan"))
        ctx.spmv(dA, dx, dy)
        ys.append(dy.to_host())
        dx.free()
    dx1 = ctx.upload(np.concatenate([[7.0], xs[0]]))
    ctx.init_vector(dy, 3.0)
    ctx.spmv(dA, dx1.offset(1), dy)
    ys.append(dy.to_host())
    dx1.free()
    rec = (dA.spmv_stream_info(), dA.win8_layout(), dA.spmv_streamed_bytes(), _layout_bytes(dA, A))
    dA.free(); dy.free()
    return ys, rec


@pytest.mark.parametrize("rp64,rows", [(0, 1), (0, 2), (0, 4), (1, 4), (1, 1)])
def test_implied_slots_are_bit_identical(ctx, oracle, rp64, rows):
    rng = np.random.default_rng(900 + 10 * rp64 + rows)
    cases = [("hpcg 40x24x20 (blocks end mid-slice, partial last block)", _randomised(oracle.gen_hpcg(40, 24, 20), rng), True),
             ("hpcg 64", _randomised(oracle.gen_hpcg(64), rng), True),
             ("hpcg 33x17x29", _randomised(oracle.gen_hpcg(33, 17, 29), rng), None),
             ("hpcg 64, perturbed rows", _perturbed(oracle.gen_hpcg(64), rng), True),
             ("random band (nothing qualifies)", _ragged(rng), False)]
    ctx.set_option("force_rp64", rp64)
    ctx.set_option("spmv_valdict", 0)
    ctx.set_option("spmv_win8_rows", rows)
    try:
        for name, A, want in cases:
            x = rng.uniform(-1, 1, A.n_cols)
            special = x.copy()  # -0.0, inf and NaN in x: a padding entry that read anything but the -0.0 slot would show
            special[::7] = -0.0
            special[5::301] = np.inf
            special[11::499] = -np.inf
            special[17::733] = np.nan
            zeros = np.where(np.arange(A.n_cols) % 2 == 0, -0.0, 0.0)
            xs = [x, special, zeros]
            ref, rec0 = _products(ctx, A, xs, 0, -1)
            old, rec_old = _products(ctx, A, xs, -1, 0)
            new, rec_new = _products(ctx, A, xs, -1, -1)
            assert rec0[0][3] == 0 and rec_old[0][3] == 6 and rec_new[0][3] == 6, (name, rec0, rec_old, rec_new)
            ch, ex, sl, bl, implied = rec_new[1]
            assert rec_old[1] == (ch, ch, sl, bl, False), (name, rec_old, rec_new)
            if want is not None:
                assert implied == want, (name, rec_new)
            if implied:
                assert 2 * (ch - ex) >= ch and rec_new[0][0] == 2, (name, rec_new)
            else:
                assert ex == ch and rec_new[0][0] == 2 and rec_new[2] == rec_old[2], (name, rec_new)
            assert rec_old[2] == rec_old[3] and rec_new[2] == rec_new[3], (name, rec_old, rec_new)
            for i in range(len(ref)):
                # the two layouts of win8: the same bits, NaNs included
                assert np.array_equal(old[i].view(np.uint64), new[i].view(np.uint64)), (name, i)
                if i == 1:  # (the row-block kernel may give a NaN of the other sign)
                    assert np.array_equal(ref[i], new[i], equal_nan=True), (name, i)
                else:
                    assert _same(ref[i], new[i]), (name, i)
            assert not np.any(np.isnan(new[2])) and np.array_equal(new[0], new[-1])
    finally:
        _reset(ctx)


def test_implied_slots_fused_cg_history_is_bit_identical(ctx, oracle):
    """the fused (Ap, p) epilogue inside the device CG loop: the same history, bit for bit, with and without implied slots"""
    A = oracle.gen_hpcg(40, 32, 24)
    rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
    val = A.val.copy()
    val[A.col == rows] += np.random.default_rng(3).uniform(0, 1, A.n_rows)
    A = CRS(A.n_rows, A.row_ptr, A.col, val)
    n = A.n_rows
    out = {}
    ctx.set_option("spmv_valdict", 0)
    ctx.set_option("spmv_win8_rows", 4)
    try:
        for implicit in (0, -1):
            ctx.set_option("spmv_win8_implicit", implicit)
            dA = ctx.matrix(A)
            b, x = ctx.alloc(n), ctx.alloc(n)
            ctx.init_vector(b, 1.0); ctx.init_vector(x, 0.1)
            cg = ctx.cg(dA, b, x)
            cg.init(1e-14)
            cg.iterate(60)
            iters, conv, hist = cg.status(hist_cap=128)
            out[implicit] = (iters, np.array(hist), x.to_host(), dA.spmv_stream_info(), dA.win8_layout())
            cg.free(); dA.free(); b.free(); x.free()
        assert out[0][3][3] == 6 and out[-1][3][3] == 6 and not out[0][4][4] and out[-1][4][4], (out[0][3:], out[-1][3:])
        assert out[0][0] == out[-1][0] and out[0][0] > 10
        assert np.array_equal(out[0][1], out[-1][1]) and np.array_equal(out[0][2], out[-1][2])
    finally:
        _reset(ctx)


def test_implied_slots_placement_search_keeps_y(ctx, oracle):
    """the build-time search and bis_mat_tune_placement move the value stream of the implied-slot layout: y stays the same"""
    A = _randomised(oracle.gen_hpcg(64), np.random.default_rng(4))
    x = ctx.upload(np.random.default_rng(5).uniform(-1, 1, A.n_cols))
    ys = {}
    ctx.set_option("spmv_valdict", 0)
    try:
        for tune in (0, 3):
            ctx.set_option("spmv_win8_tune", tune)
            dA = ctx.matrix(A)
            y = ctx.alloc(A.n_rows)
            ctx.spmv(dA, x, y)
            assert dA.spmv_stream_info()[3] == 6 and dA.win8_layout()[4]
            trials, first_ms, kept_ms = dA.win8_tuning()
            if tune:
                assert 0 <= trials <= 3 and first_ms > 0 and 0 < kept_ms <= first_ms
            ys[tune] = y.to_host()
            if tune:
                first, best = ctx.tune_placement(dA, max_trials=3)
                assert first > 0 and 0 < best <= first
                ctx.spmv(dA, x, y)
                ys["after"] = y.to_host()
            dA.free(); y.free()
        assert np.array_equal(ys[0], ys[3]) and np.array_equal(ys[0], ys["after"])
    finally:
        _reset(ctx)
        x.free()


def _row_block_product(ctx, dA, x):
    """y = A x of dA's CRS arrays as they are now, by the row-block kernel (spmv_win8 = 0) on a second matrix"""
    rp, col, val = dA.download()
    ctx.set_option("spmv_win8", 0)
    ref = ctx.matrix(CRS(dA.n_rows, rp, col, val, n_cols=dA.n_cols))
    y = ctx.alloc(dA.n_rows)
    ctx.spmv(ref, x, y)
    assert ref.spmv_stream_info()[3] not in (6, 8)
    out = y.to_host()
    ref.free(); y.free()
    ctx.set_option("spmv_win8", -1)
    return out


@pytest.mark.parametrize("gen,implied,rounded", [("hpcg", True, False), ("hpcg", True, True), ("fem", False, False), ("fem", False, True)])
def test_redirected_stream_is_the_callers(ctx, gen, implied, rounded):
    """bis_mat_win8_debug_stream: a stream redirected to the caller's memory is read from there (the same y, bit for bit), the
    library's own buffer comes back on restore, and a matrix dropped while redirected (scale_sym changes the values) frees its own
    buffer, never the caller's.  The 8-byte stream and, after round_f32, the 4-byte one; implied slots (hpcg 16: 4096 rows in
    256-row blocks) and the explicit layout (fem 6)."""
    import ctypes as C
    from basic_iterative_solvers_amd import Vec

    def stream(dA, to=None):
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        ctx.check(ctx.lib.bis_mat_win8_debug_stream(dA.h, C.byref(ptr), C.byref(nbytes), C.c_void_p(to) if to else None))
        return ptr.value, nbytes.value

    ctx.set_option("spmv_valdict", 0)
    try:
        dA = ctx.gen_hpcg(16) if gen == "hpcg" else ctx.gen_fem(6)
        if rounded:
            dA.round_f32()
        form = 8 if rounded else 6
        x = ctx.upload(np.random.default_rng(61).uniform(-1, 1, dA.n_cols))
        y = ctx.alloc(dA.n_rows)
        ref = _row_block_product(ctx, dA, x)
        ctx.spmv(dA, x, y)  # 1: the stream exists
        assert dA.spmv_stream_info()[3] == form and dA.win8_layout()[4] == implied, (dA.spmv_stream_info(), dA.win8_layout())
        assert np.array_equal(y.to_host().view(np.uint64), ref.view(np.uint64))
        own, nbytes = stream(dA)
        assert own and nbytes > 0 and nbytes % 8 == 0
        mine = ctx.alloc(nbytes // 8)  # 2: the caller's copy
        ctx.copy_vector(mine, Vec(ctx, own, nbytes // 8, False))
        held = mine.to_host()
        stream(dA, to=mine.ptr)  # 3: read from the copy
        ctx.init_vector(y, float("nan"))
        ctx.spmv(dA, x, y)
        assert np.array_equal(y.to_host().view(np.uint64), ref.view(np.uint64))
        assert stream(dA) == (own, nbytes)  # 4: set = NULL restores; redirected or not, the report is the library's own buffer
        assert stream(dA) == (own, nbytes)
        stream(dA, to=mine.ptr)  # 5: dropped while redirected
        s = ctx.scale_sym(dA)
        assert np.array_equal(mine.to_host().view(np.uint64), held.view(np.uint64))  # 6
        ref2 = _row_block_product(ctx, dA, x)
        ctx.init_vector(y, float("nan"))
        ctx.spmv(dA, x, y)  # 7: rebuilt (8-byte values: scale_sym clears the fp32 flag)
        assert dA.spmv_stream_info()[3] == 6 and stream(dA)[0] != mine.ptr
        assert np.array_equal(y.to_host().view(np.uint64), ref2.view(np.uint64))
        assert not np.array_equal(ref, ref2)
        mine.free()  # 8
        dA.free(); x.free(); y.free(); s.free()
    finally:
        _reset(ctx)


def test_implied_slots_partitioned_bench_path():
    """`--gpus 1` under BIS_FORCE_DIST=1 (row views of the matrix, each built by the same win8 builder): bit-identical outputs
    with and without implied slots, and the same solve as the plain path"""
    def run(tmp, extra_env):
        env = dict(os.environ, OMP_NUM_THREADS="1", **extra_env)
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "BIS_PHASE_DIR", "BIS_BENCH_REHEARSE"):
            env.pop(k, None)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", "64", "--steps", "30",
                              "--warmup", "2", "--no-cpu-baseline", "--no-target-512", "--no-sweeps", "--no-configs",
                              "--dump-outputs", tmp], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        return (json.loads(lines[0]), np.load(os.path.join(tmp, "residual_history.npy")), np.load(os.path.join(tmp, "x.npy")))

    import tempfile
    with tempfile.TemporaryDirectory() as d:
        plain = run(os.path.join(d, "plain"), {})
        dist_on = run(os.path.join(d, "on"), {"BIS_FORCE_DIST": "1"})
        dist_off = run(os.path.join(d, "off"), {"BIS_FORCE_DIST": "1", "BIS_SPMV_WIN8_IMPLICIT": "0"})
    assert dist_on[0]["n_gpus"] == 1 and dist_on[0]["per_rank"][0]["spmv_stream"]["val_bytes"] == 8
    assert np.array_equal(dist_on[1], dist_off[1]) and np.array_equal(dist_on[2], dist_off[2])
    m = min(len(plain[1]), len(dist_on[1]))
    assert m > 10 and np.max(np.abs(plain[1][:m] - dist_on[1][:m])) <= 1e-10 * plain[1][0]
    assert np.max(np.abs(plain[2] - dist_on[2])) <= 1e-8 * max(np.max(np.abs(plain[2])), 1e-300)
