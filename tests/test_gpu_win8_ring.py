"""GPU: the chunk ring of the window + sliced-ELL SpMV (win8 / win4, bis_spmv_win8.hip) with one and with two register sets.

A wave walks its n = C1 - C0 chunks in rounds of D (spmv_win8_depth); with two register sets (spmv_win8_sets = 2, depths 1-4) a
loop trip is two whole rounds, then at most one whole round, then fewer than D steps that request nothing.  What can go wrong
is how n relates to D (n = 0, n < D, n = D, D < n < 2D, n = 2D, n = 2D + 1, odd / even numbers of whole rounds) and where the
ends of a wave's slices fall inside a round.  The staircase matrix below gives every wave a different n: 64-row groups of
uniform row length 0 .. 59 (0 .. 15 chunks per slice; a wave owns 1, 2 or 4 slices), three times over at three phases of the
256-, 512- and 1024-row blocks, the groups between them ragged (explicit slices inside the implied-slot layout).  Its ragged
twin keeps every slot explicit.  y is BIT-IDENTICAL to the row-block kernel on the CRS arrays for every depth and both ring
forms, and within 1e-13 (|A||x|)max of the oracle; win4 equals win8 on the rounded matrix; the CG history with the fused
(Ap, p) epilogue is bit-identical between depths and ring forms."""
import numpy as np
import pytest

from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu
KTOL = 1e-13
DEPTHS = (1, 2, 3, 4, 6)
SETS = (1, 2)  # (depth 6 has the one-set form only: sets = 2 runs it as well)
OPTS = ("force_rp64", "spmv_valdict", "spmv_win8_rows", "spmv_win8_depth", "spmv_win8_sets", "spmv_win8", "spmv_win4",
        "spmv_win8_implicit")
SPECIAL = [-0.0, 0.0, 5e-324, -1.0, 26.0, 1.7976931348623157e308, -1.7976931348623157e308, 1.0 + 2.0 ** -52]
SPECIAL_F32 = [-0.0, 0.0, 2.0 ** -149, -1.0, 26.0, 3.4028234663852886e38, -3.4028234663852886e38, 1.0 + 2.0 ** -23]


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    yield c
    c.close()


def _reset(ctx):
    for k in OPTS:
        ctx.set_option(k, -1)


def same_y(a, b):
    """bit for bit, or the same values with the same signs where NaNs sit in the same places (tests/test_gpu_win8.py's rule)"""
    return np.array_equal(a.view(np.uint64), b.view(np.uint64)) or (
        np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b)))


def group_lengths():
    """row length of each 64-row group; -1: a ragged group.  The staircases start at groups 0, 61 and 123: 0 / 1 / 3 mod 4,
    0 / 5 / 3 mod 8, 0 / 13 / 11 mod 16 (the groups of a 256-, 512-, 1024-row block)."""
    stair = list(range(60))
    return stair + [-1] + stair + [-1, -1] + stair


def staircase(rng, ragged, special=SPECIAL, reps=1):
    """reps = 1: 11,712 rows.  The library gives a matrix blocks of 512 (1024) rows only from 2^19 (2^20) rows on, whatever
    spmv_win8_rows asks for, so the instances with 2 and 4 rows per lane are reached with reps = 45 and 90: the smallest such
    sizes (183 groups per repetition, 7 mod 16: every repetition meets the blocks at another phase)."""
    groups = group_lengths() * reps
    n = 64 * len(groups)
    lens = np.zeros(n, dtype=np.int64)
    for g, l in enumerate(groups):
        lens[64 * g:64 * g + 64] = rng.integers(3, 12, 64) if l < 0 else l
    if ragged:
        lens = np.maximum(lens - rng.integers(0, 4, n), 0)
    rp = np.concatenate([[0], np.cumsum(lens)])
    rows = np.repeat(np.arange(n), lens)
    j = np.arange(rp[-1]) - rp[rows]  # position inside the row
    if ragged:  # random offsets inside a band
        col = np.clip(rows + rng.integers(-120, 121, rp[-1]), 0, n - 1)
    else:  # row + offset_j for ONE sorted offset list: a slice of 64 equally long rows has one slot pattern
        offsets = np.sort(rng.choice(np.arange(-120, 121), 60, replace=False))
        col = np.clip(rows + offsets[j], 0, n - 1)
        ragged_rows = np.repeat(np.repeat(np.array(groups) < 0, 64), lens)
        col[ragged_rows] = np.clip(rows[ragged_rows] + rng.integers(-120, 121, int(ragged_rows.sum())), 0, n - 1)
    val = rng.uniform(-2, 2, rp[-1])
    val[:8] = special
    return CRS(n, rp, col.astype(np.int32), val)


REPS = {1: 1, 2: 45, 4: 90}  # spmv_win8_rows -> repetitions of the staircase


@pytest.fixture(scope="module")
def cases(oracle):
    """rows per lane -> [(name, matrix, x, oracle's y, 1e-13 (|A||x|)max, rows held to that bound)], each made once.  The rows
    that hold +-DBL_MAX are held to bit-identity with the row-block kernel only: (|A||x|)max over them would make the bound on
    every row vacuous."""
    made = {}

    def get(rows_per_lane):
        if rows_per_lane not in made:
            out = []
            for name, ragged, seed in (("staircase", False, 11), ("ragged twin", True, 12)):
                rng = np.random.default_rng(seed)
                A = staircase(rng, ragged, reps=REPS[rows_per_lane])
                x = rng.uniform(-1, 1, A.n_cols)
                rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
                ordinary = np.ones(A.n_rows, dtype=bool)
                ordinary[rows[np.abs(A.val) > 1e6]] = False
                B = CRS(A.n_rows, A.row_ptr, A.col, np.where(np.abs(A.val) > 1e6, 0.0, A.val))
                scale = np.bincount(rows, weights=np.abs(B.val) * np.abs(x[B.col]), minlength=A.n_rows).max()  # (|A||x|)max
                out.append((name, A, x, oracle.spmv(B, x), KTOL * scale, ordinary))
            made[rows_per_lane] = out
        return made[rows_per_lane]
    return get


def test_the_staircase_gives_every_chunk_count():
    """the inputs themselves: slices of 0 .. 15 chunks, so with 1 row per lane a wave's n takes every value 0 .. 15 (n = 0,
    n < D, n = D, D < n < 2D, n = 2D and n = 2D + 1 for every depth 1 .. 6), and few padded entries (the plan's 12 % limit)"""
    A = staircase(np.random.default_rng(11), False)
    lens = np.diff(A.row_ptr)
    per_group = lens.reshape(-1, 64)
    uniform = per_group[(per_group == per_group[:, :1]).all(axis=1), 0]
    assert set((uniform + 3) // 4) == set(range(16))
    for d in DEPTHS:
        assert {0, d - 1, d, 2 * d - 1, 2 * d, 2 * d + 1} <= set(range(16))
    assert 4 * ((lens + 3) // 4).sum() <= 1.12 * A.nnz


@pytest.mark.parametrize("rp64", [0, 1])
@pytest.mark.parametrize("implicit", [0, 1])
@pytest.mark.parametrize("rows", [1, 2, 4])
def test_ring_depths_and_sets_are_bit_identical_to_the_rowblock_kernel(ctx, cases, rows, implicit, rp64):
    ctx.set_option("force_rp64", rp64)
    ctx.set_option("spmv_valdict", 0)
    ctx.set_option("spmv_win8_rows", rows)
    ctx.set_option("spmv_win8_implicit", implicit)
    try:
        for name, A, x, yo, tol, ordinary in cases(rows):
            dA = ctx.matrix(A)
            dx, dy = ctx.upload(x), ctx.alloc(A.n_rows)
            dx1 = ctx.upload(np.concatenate([[7.0], x]))
            ctx.set_option("spmv_win8", 0)
            assert dA.spmv_stream_info()[3] == 0, name
            ctx.init_vector(dy, float("nan"))
            ctx.spmv(dA, dx, dy)
            y0 = dy.to_host()
            ctx.set_option("spmv_win8", -1)
            info = dA.spmv_stream_info()
            assert info[1] == 8 and info[3] == 6, (name, info)
            ch, ex, sl, bl, implied = dA.win8_layout()
            assert sl == 4 * rows * bl and ch > 0, (name, dA.win8_layout())
            if name == "staircase" and implicit:  # implied chunks, and explicit ones (the ragged groups) among them
                assert implied and 0 < ex < ch // 4, (name, dA.win8_layout())
            else:  # every chunk keeps its slots
                assert not implied and ex == ch, (name, dA.win8_layout())
            for depth in DEPTHS:
                for sets in SETS:
                    ctx.set_option("spmv_win8_depth", depth)
                    ctx.set_option("spmv_win8_sets", sets)
                    ctx.init_vector(dy, float("nan"))
                    ctx.spmv(dA, dx, dy)
                    y = dy.to_host()
                    assert same_y(y0, y), (name, depth, sets)
                    worst = int(np.argmax(np.where(ordinary, np.abs(y - yo), 0.0)))
                    err = abs(y[worst] - yo[worst])
                    assert err <= tol, (name, depth, sets, worst, y[worst], yo[worst], tol)
                    ctx.init_vector(dy, 3.0)  # an x that is only 8-byte aligned: the window is filled through registers
                    ctx.spmv(dA, dx1.offset(1), dy)
                    assert same_y(y, dy.to_host()), (name, depth, sets, "8-byte-aligned x")
                    ctx.spmv(dA, dx, dy)  # a second product on the built form
                    assert same_y(y, dy.to_host()), (name, depth, sets, "second product")
            ctx.set_option("spmv_win8_depth", -1)
            ctx.set_option("spmv_win8_sets", -1)
            dA.free(); dx.free(); dy.free(); dx1.free()
    finally:
        _reset(ctx)


@pytest.mark.parametrize("implicit", [0, 1])
@pytest.mark.parametrize("rows", [1, 2, 4])
def test_win4_ring_is_bit_identical_to_win8_on_the_rounded_staircase(ctx, rows, implicit):
    rng = np.random.default_rng(13)
    A = staircase(rng, False, special=SPECIAL_F32, reps=REPS[rows])
    A = CRS(A.n_rows, A.row_ptr, A.col, A.val.astype(np.float32).astype(np.float64))
    x = rng.uniform(-1, 1, A.n_cols)
    ctx.set_option("spmv_valdict", 0)
    ctx.set_option("spmv_win8_rows", rows)
    ctx.set_option("spmv_win8_implicit", implicit)
    try:
        dA = ctx.matrix(A)
        assert dA.round_f32() == 0.0  # (rounded on the host already: the call only sets the flag)
        dx, dy = ctx.upload(x), ctx.alloc(A.n_rows)
        ctx.set_option("spmv_win4", 0)
        assert dA.spmv_stream_info()[3] == 6
        ctx.init_vector(dy, float("nan"))
        ctx.spmv(dA, dx, dy)
        y8 = dy.to_host()
        ctx.set_option("spmv_win4", -1)
        info = dA.spmv_stream_info()
        assert info[1] == 4 and info[3] == 8, info
        ch, ex, sl, bl, implied = dA.win8_layout()
        assert sl == 4 * rows * bl, dA.win8_layout()
        assert implied == bool(implicit) and (0 < ex < ch // 4 if implicit else ex == ch), dA.win8_layout()
        for depth in DEPTHS:
            for sets in SETS:
                ctx.set_option("spmv_win8_depth", depth)
                ctx.set_option("spmv_win8_sets", sets)
                ctx.init_vector(dy, float("nan"))
                ctx.spmv(dA, dx, dy)
                assert same_y(y8, dy.to_host()), (depth, sets)
        dA.free(); dx.free(); dy.free()
    finally:
        _reset(ctx)


def _hpcg_with_random_diagonal(oracle, n1, seed):
    """the 27-point HPCG operator with a random amount added to its diagonal: SPD, no two rows with the same values"""
    A = oracle.gen_hpcg(n1)
    diag = A.col == np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
    val = A.val.copy()
    val[diag] += np.random.default_rng(seed).uniform(0, 1, int(diag.sum()))
    return CRS(A.n_rows, A.row_ptr, A.col, val)


def test_fused_cg_history_is_bit_identical_between_depths_and_sets(ctx, oracle):
    """the fused (Ap, p) epilogue: one partial per wave at the same index, whatever the ring -- 80 iterations of CG on the 20^3
    operator give the same history bit for bit at every rows value, depth and ring form, the oracle's within 1e-10 r0.  (A matrix
    of this size gets 256-row blocks whatever spmv_win8_rows says: the next test runs the larger blocks.)"""
    A = _hpcg_with_random_diagonal(oracle, 20, 7)
    n = A.n_rows
    ref = oracle.solve(A, "cg", "none")
    ctx.set_option("spmv_valdict", 0)
    try:
        for rows in (1, 2, 4):
            ctx.set_option("spmv_win8_rows", rows)
            dA = ctx.matrix(A)
            b, x = ctx.alloc(n), ctx.alloc(n)
            first = None
            for depth in DEPTHS:
                for sets in SETS:
                    ctx.set_option("spmv_win8_depth", depth)
                    ctx.set_option("spmv_win8_sets", sets)
                    ctx.init_vector(b, 1.0); ctx.init_vector(x, 0.1)
                    cg = ctx.cg(dA, b, x)
                    cg.init(1e-14)
                    cg.iterate(80)
                    iters, conv, hist = cg.status(hist_cap=128)
                    hist = np.array(hist, dtype=np.float64)
                    cg.free()
                    assert dA.spmv_stream_info()[3] == 6
                    if first is None:
                        first = (iters, hist)
                        m = min(len(ref["hist"]), len(hist))
                        assert np.max(np.abs(ref["hist"][:m] - hist[:m])) <= 1e-10 * ref["hist"][0], rows
                        assert abs(iters - ref["iters"]) <= 1, (rows, iters, ref["iters"])
                    assert iters == first[0] and np.array_equal(hist.view(np.uint64), first[1].view(np.uint64)), (rows, depth, sets)
            dA.free(); b.free(); x.free()
    finally:
        _reset(ctx)


@pytest.mark.parametrize("rows", [2, 4])
def test_fused_cg_history_on_blocks_of_512_and_1024_rows(ctx, rows):
    """the same on the device-generated 102^3 HPCG operator (1,061,208 rows: the smallest cube that gets 1024-row blocks), whose
    waves own 2 and 4 slices: 30 iterations, bit-identical between depths and ring forms, and within 1e-10 r0 of the history
    with the row-block kernel on the CRS arrays"""
    ctx.set_option("spmv_valdict", 0)
    ctx.set_option("spmv_win8_rows", rows)
    try:
        dA = ctx.gen_hpcg(102)
        n = dA.n_rows
        b, x = ctx.alloc(n), ctx.alloc(n)

        def run():
            ctx.init_vector(b, 1.0); ctx.init_vector(x, 0.1)
            cg = ctx.cg(dA, b, x)
            cg.init(1e-14)
            cg.iterate(30)
            iters, conv, hist = cg.status(hist_cap=64)
            cg.free()
            return iters, np.array(hist, dtype=np.float64)
        ctx.set_option("spmv_win8", 0)
        ref = run()
        assert dA.spmv_stream_info()[3] == 0
        ctx.set_option("spmv_win8", -1)
        first = None
        for depth in DEPTHS:
            for sets in SETS:
                ctx.set_option("spmv_win8_depth", depth)
                ctx.set_option("spmv_win8_sets", sets)
                got = run()
                ch, ex, sl, bl, implied = dA.win8_layout()
                assert dA.spmv_stream_info()[3] == 6 and sl == 4 * rows * bl and implied, dA.win8_layout()
                if first is None:
                    first = got
                    assert got[0] == ref[0] and np.max(np.abs(got[1] - ref[1])) <= 1e-10 * ref[1][0]
                assert got[0] == first[0] and np.array_equal(got[1].view(np.uint64), first[1].view(np.uint64)), (depth, sets)
        dA.free(); b.free(); x.free()
    finally:
        _reset(ctx)
