"""GPU: bis_sptrsm / bis_bsptrsm (triangular sweeps on 1..8 interleaved right-hand sides) column by column against the
single-vector sweeps and the oracle, bit for bit; both forms (a launch per level, the persistent wave-per-row kernel)
through option trsm_form; aliasing, independence of the columns, determinism, the int64 row-pointer instances, errors.

The contract (include/bis_hip.h): column j of bis_sptrsm IS bis_sptrsv on column j -- the same fma chain in CRS order, the
same subtraction and division -- so every comparison here is an equality of bit patterns, never a tolerance."""
import numpy as np
import pytest

from helpers import crs_of, load_golden
from oracle.pyoracle import CRS, Oracle

pytestmark = pytest.mark.gpu

FEW_LEVELS = 64  # at most this many levels: a launch per level; more: the persistent kernel (bis_sptrsm.hip)


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.set_option("trsm_form", -1)
    c.close()


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def crs_from_rows(n, rows, vals):
    lens = [len(r) for r in rows]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if sum(lens) else np.zeros(0, np.int32)
    val = np.concatenate([np.asarray(v, dtype=np.float64) for v in vals]) if sum(lens) else np.zeros(0)
    return CRS(n, rp, col, val)


def mirror(T):
    """The strictly upper triangle with entry (n-1-r, n-1-c) for every entry (r, c) of the strictly lower T, columns ascending."""
    n = T.n_rows
    rows, vals = [], []
    for r in range(n - 1, -1, -1):
        a, b = T.row_ptr[r], T.row_ptr[r + 1]
        rows.append((n - 1 - T.col[a:b])[::-1])
        vals.append(T.val[a:b][::-1])
    return crs_from_rows(n, rows, vals)


def band_lower(n, half, seed):
    """Every entry of the band: rows of up to `half` entries, as many dependency levels as rows."""
    rng = np.random.default_rng(seed)
    rows = [np.arange(max(0, r - half), r) for r in range(n)]
    vals = [rng.uniform(-1, 1, len(c)) / half for c in rows]
    return crs_from_rows(n, rows, vals), rng.uniform(1, 2, n)


def ragged_lower(n, seed, chained=True):
    """Rows of 1..6 entries, three rows of 150-199 entries, a few empty rows; row r's entries and its diagonal carry the
    row's scale 10^(-6..6) (the entries divided by their count + 1, so that the solution stays finite).

    chained: every row with entries holds column r - 1, so the triangle has 184 levels and no two neighbouring
    rows are independent.  Why: a triangle that splits into at most 64 contiguous blocks of mutually independent rows sends
    bis_sptrsv to its row-block form (spmv_rowblock_kernel with the triangular epilogue), which rounds every product and
    then adds -- the serial loop's bits only where the products are exact, as with HPCG's -1 entries -- so there the two
    references of this file differ in the last bit and no result can equal both.  chained = False builds exactly such a
    triangle (36 blocks, 24 levels; rows of 0..6 entries): it is checked against the serial loop alone."""
    rng = np.random.default_rng(seed)
    long_rows = {160: 150, 180: 170, 199: 199}
    empty = {0, 5, 50, 100}
    rows, vals, D = [], [], np.empty(n)
    for r in range(n):
        lo = 1 if chained else 0
        cnt = 0 if r in empty else long_rows.get(r, int(rng.integers(lo, min(r, 6) + 1)))
        if cnt and chained:
            c = np.sort(np.append(rng.choice(r - 1, size=cnt - 1, replace=False), r - 1)) if cnt > 1 else np.array([r - 1])
        else:
            c = np.sort(rng.choice(r, size=cnt, replace=False)) if cnt else np.zeros(0, np.int64)
        scale = 10.0 ** rng.uniform(-6, 6)
        rows.append(c)
        vals.append(scale * rng.uniform(-1, 1, cnt) / (cnt + 1))
        D[r] = scale * rng.uniform(1, 2)
    return crs_from_rows(n, rows, vals), D


def n_levels(T, backward):
    n = T.n_rows
    lvl = np.zeros(n, dtype=np.int64)
    order = range(n - 1, -1, -1) if backward else range(n)
    for r in order:
        c = T.col[T.row_ptr[r]:T.row_ptr[r + 1]]
        lvl[r] = lvl[c].max() + 1 if len(c) else 0
    return int(lvl.max()) + 1 if n else 0


CASES = ["hpcg8", "hpcg_4x6x5", "band300", "ragged200", "multicolour16", "nnz0", "n1", "n0", "raggedblocks200"]
SERIAL_LOOP_ONLY = {"raggedblocks200"}  # bis_sptrsv runs its row-block form there: see ragged_lower


@pytest.fixture(scope="module")
def tri(ctx):
    """name -> dict(L, U host CRS, D host, dL, dU, dD device, levels (forward, backward)): built once, never changed."""
    out = {}
    for name in CASES:
        if name in ("hpcg8", "hpcg_4x6x5"):
            g = load_golden(name)
            L, U, D = crs_of(g, "Ls"), crs_of(g, "Us"), g["A_D"]
        elif name == "band300":
            L, D = band_lower(300, 70, 3)
            U = mirror(L)
        elif name in ("ragged200", "raggedblocks200"):
            L, D = ragged_lower(200, 4, chained=name == "ragged200")
            U = mirror(L)
            D = D.copy()
        elif name == "multicolour16":
            dA = ctx.gen_hpcg(16)
            dB, _, n_col = ctx.multicolour(dA)
            assert n_col <= FEW_LEVELS
            dL, dU, dD, dDinv = ctx.split_strict(dB)
            L, U = CRS(dL.n_rows, *dL.download()), CRS(dU.n_rows, *dU.download())
            out[name] = dict(L=L, U=U, D=dD.to_host(), dL=dL, dU=dU, dD=dD)
            dA.free(); dDinv.free()
        else:
            n = {"nnz0": 37, "n1": 1, "n0": 0}[name]
            L = U = CRS(n, np.zeros(n + 1, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0))
            D = np.random.default_rng(5).uniform(1, 2, n)
        if name not in out:
            out[name] = dict(L=L, U=U, D=np.ascontiguousarray(D, dtype=np.float64), dL=ctx.matrix(L), dU=ctx.matrix(U),
                             dD=ctx.upload(D) if len(D) else ctx.alloc(1))
        e = out[name]
        e["levels"] = (n_levels(e["L"], False), n_levels(e["U"], True))
    return out


def rhs_block(n, k, seed):
    """n x k: column 0 ones, column 1 uniform, the rest uniform at the scales 1e-6, 1, 1e6."""
    rng = np.random.default_rng(seed)
    B = rng.uniform(-1, 1, (n, k))
    if n:
        B[:, 0] = 1.0
    for j in range(2, k):
        B[:, j] *= (1e-6, 1.0, 1e6)[(j - 2) % 3]
    return B


def sweepm(ctx, dT, dD, B, backward, alias=False):
    n, k = B.shape
    dB = ctx.upload(B.ravel()) if n else ctx.alloc(1)
    dX = dB if alias else ctx.alloc(max(n * k, 1))
    (ctx.bsptrsm if backward else ctx.sptrsm)(dT, dX, dD, dB, k)
    ctx.sync()
    X = dX.to_host()[:n * k].reshape(n, k)
    dB.free()
    if not alias:
        dX.free()
    return X


def single(ctx, dT, dD, b, backward):
    db, dx = ctx.upload(b), ctx.alloc(len(b))
    (ctx.bsptrsv if backward else ctx.sptrsv)(dT, dx, dD, db)
    x = dx.to_host()
    db.free(); dx.free()
    return x


def expected_name(form, levels, k, backward, rp=32):
    if k == 1:
        return "bis_bsptrsv K=1" if backward else "bis_sptrsv K=1"
    wave = form == 2 or (form != 1 and levels > FEW_LEVELS)
    return f"{'trsm_wave_kernel' if wave else 'trsm_level_kernel'} K={k} RP={rp}"


@pytest.mark.parametrize("name", CASES)
def test_columns_equal_the_single_vector_sweep_and_the_oracle(ctx, orc, tri, name):
    e = tri[name]
    n = e["L"].n_rows
    ks = range(1, 9) if name == "hpcg8" else (2, 3, 5, 8)
    for backward in (False, True):
        T, dT = (e["U"], e["dU"]) if backward else (e["L"], e["dL"])
        for k in ks:
            B = rhs_block(n, k, seed=10 * k + backward)
            both = name not in SERIAL_LOOP_ONLY  # (there the device reference is not computed at all)
            ref_dev = [single(ctx, dT, e["dD"], B[:, j].copy(), backward) for j in range(k)] if n and both else []
            ref_orc = [orc.sptrsv(T, e["D"], B[:, j].copy(), backward=backward) for j in range(k)] if n else []
            for j in range(len(ref_dev)):  # the two references agree: the single-vector sweep reproduces the serial loop's bits
                assert same_bits(ref_dev[j], ref_orc[j]), (name, backward, k, j, dT.sweep_kernel(backward))
            for form in (0, 1, 2):
                ctx.set_option("trsm_form", form)
                try:
                    X = sweepm(ctx, dT, e["dD"], B, backward)
                    kernel = dT.sweepm_kernel(backward)
                    Xa = sweepm(ctx, dT, e["dD"], B, backward, alias=True)
                finally:
                    ctx.set_option("trsm_form", -1)
                tag = (name, "backward" if backward else "forward", k, form, kernel)
                for j in range(k if n else 0):
                    if both:
                        assert same_bits(X[:, j], ref_dev[j]), tag + (j, int(np.sum(X[:, j] != ref_dev[j])))
                    assert same_bits(X[:, j], ref_orc[j]), tag + (j,)
                assert same_bits(Xa, X), tag + ("X aliasing B",)
                if n:
                    assert kernel == expected_name(form, e["levels"][backward], k, backward), tag
    if n == 0:
        assert e["dL"].sweepm_kernel() == ""  # nothing was launched


def test_level_counts_reach_both_forms(tri):
    """The cases are what the issue says they are: natural orderings with more levels than a launch per level serves, a
    multi-colour ordering with few, rows longer than one trip of the wave kernel at every k (64 / k entries) and than 64."""
    assert min(tri["hpcg8"]["levels"]) >= 8 and min(tri["band300"]["levels"]) == 300 and min(tri["ragged200"]["levels"]) > FEW_LEVELS
    assert 3 < max(tri["raggedblocks200"]["levels"]) <= FEW_LEVELS
    assert max(tri["multicolour16"]["levels"]) <= FEW_LEVELS
    assert int(np.diff(tri["band300"]["L"].row_ptr).max()) == 70
    for name in ("ragged200", "raggedblocks200"):
        assert sorted(np.diff(tri[name]["L"].row_ptr))[-3:] == [150, 170, 199]
        assert int(np.sum(np.diff(tri[name]["L"].row_ptr) == 0)) >= 4
    assert tri["nnz0"]["L"].nnz == 0 and tri["n1"]["L"].n_rows == 1 and tri["n0"]["L"].n_rows == 0


@pytest.mark.parametrize("name,form", [("band300", 2), ("multicolour16", 0), ("hpcg_4x6x5", 1)])
def test_columns_are_independent_and_runs_repeat(ctx, tri, name, form):
    e = tri[name]
    n, k = e["L"].n_rows, 5
    ctx.set_option("trsm_form", form)
    try:
        for backward in (False, True):
            dT = e["dU"] if backward else e["dL"]
            B = rhs_block(n, k, seed=77)
            X = sweepm(ctx, dT, e["dD"], B, backward)
            assert same_bits(sweepm(ctx, dT, e["dD"], B, backward), X)  # two runs, the same bits
            B2 = B.copy()
            B2[:, 2] = np.random.default_rng(78).uniform(-5, 5, n)
            X2 = sweepm(ctx, dT, e["dD"], B2, backward)
            assert not same_bits(X2[:, 2], X[:, 2])
            for j in (0, 1, 3, 4):  # changing column 2 of B changes no bit of any other column of X
                assert same_bits(X2[:, j], X[:, j]), (name, backward, j)
    finally:
        ctx.set_option("trsm_form", -1)


def test_int64_row_pointer_instances(ctx, orc, tri):
    e = tri["band300"]
    ctx.set_option("force_rp64", 1)
    try:
        dL, dU = ctx.matrix(e["L"]), ctx.matrix(e["U"])
    finally:
        ctx.set_option("force_rp64", -1)
    assert dL.rp_width == 8 and dU.rp_width == 8
    n = e["L"].n_rows
    try:
        for backward, T, dT in ((False, e["L"], dL), (True, e["U"], dU)):
            for k in (3, 8):
                B = rhs_block(n, k, seed=5 + k)
                for form in (1, 2):
                    ctx.set_option("trsm_form", form)
                    X = sweepm(ctx, dT, e["dD"], B, backward)
                    assert dT.sweepm_kernel(backward) == expected_name(form, 300, k, backward, rp=64)
                    for j in range(k):
                        assert same_bits(X[:, j], orc.sptrsv(T, e["D"], B[:, j].copy(), backward=backward)), (backward, k, form, j)
                        assert same_bits(X[:, j], single(ctx, dT, e["dD"], B[:, j].copy(), backward)), (backward, k, form, j)
    finally:
        ctx.set_option("trsm_form", -1)
        dL.free(); dU.free()


def test_errors(ctx, tri):
    from basic_iterative_solvers_amd import BisError
    e = tri["hpcg8"]
    n = e["L"].n_rows
    X, B = ctx.alloc(n * 9), ctx.alloc(n * 9)
    ctx.init_vector(B, 1.0)
    for k in (0, 9):
        with pytest.raises(BisError, match="status 2"):
            ctx.sptrsm(e["dL"], X, e["dD"], B, k)
        with pytest.raises(BisError, match="status 2"):
            ctx.bsptrsm(e["dU"], X, e["dD"], B, k)
    dA = ctx.matrix(crs_of(load_golden("hpcg8"), "A"))  # a diagonal entry in every row
    with pytest.raises(BisError, match="status 2.*bis_sptrsm: matrix is not strictly lower triangular"):
        ctx.sptrsm(dA, X, e["dD"], B, 4)
    with pytest.raises(BisError, match="status 2.*bis_bsptrsm: matrix is not strictly upper triangular"):
        ctx.bsptrsm(dA, X, e["dD"], B, 4)
    with pytest.raises(BisError, match="status 2.*strictly upper"):
        ctx.bsptrsm(e["dL"], X, e["dD"], B, 4)  # a lower triangle on the backward side
    assert dA.sweepm_kernel() == ""
    dA.free(); X.free(); B.free()
