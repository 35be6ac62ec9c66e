"""GPU: block Jacobi (bis_bj_*, preconditioner type 11) against the numpy restatement of include/bis_hip.h's definitions
(tests/bjacobi_ref.py; tests/test_bjacobi_abi.py ties that restatement to numpy.linalg.inv on the CPU).

Setup and apply are compared bit for bit: the downloaded inverse blocks with the restated Gauss-Jordan inverses, bis_bj_apply
and bis_bj_mapply with the restated product, on every input below, with out aliasing in, with both vectors one element off
a 16-byte boundary, twice.  Inputs: fem 6x6x6 and 5x4x3 at 3 rows a block; hpcg 8x7x6 (336 rows) at 1, 2, 5, 13 and 32 (last
blocks of 1, 11 and 16 rows); a nonsymmetric 601-row band of half-width 20 with four zero diagonal entries (each next to a
strong off-diagonal pair, so the elimination has to swap) at 8 rows a block (last block: 1 row), under a random block_ptr
that mixes 1..32 and starts 32, 1, 32, 1, 1, and with entries split into repeated, unsorted ones; hpcg 40x24x20 at 7
(19200 = 7 * 2742 + 6, several workgroups); the first and the last also with 64-bit row pointers.

Solves: each device solver with the handle against a numpy restatement of the same iteration with the restated apply: the
stopping iteration equal, the history within the project's gate for the method (helpers.HIST_TOL; MINRES at CG's, FGMRES and
MGMRES at GMRES'), the residual of the returned x -- in the norm the method records -- within that gate of the last entry.

Not covered: the row-range-view row of the error table (no public entry point makes a view), and "nothing is left
allocated" after a failing create (another process on the device moves the free-memory figure).

Each test prints what it measured before it asserts."""
import ctypes as C

import numpy as np
import pytest

import bjacobi_ref as ref
from helpers import HIST_TOL, OptionScope, hist_dev
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

INVALID, ZERO_DIAG, UNSUPPORTED = 2, 4, 6
ZERO_ROWS = (50, 203, 333, 468)  # zero diagonal entries of the band; none is the last row of a block of 8


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def host_crs(dA):
    return CRS(dA.n_rows, *dA.download())


# ---- the band ---------------------------------------------------------------------------------------------------------

def band601(dups=False, plant=None):
    """Nonsymmetric band, n = 601, half-width 20, rows dominated by their diagonal -- except the rows z of ZERO_ROWS, whose
    diagonal entry is a stored 0.0 and which are coupled to row z + 1 by a pair of entries as large as a diagonal.  dups:
    every fifth entry is split into two entries of the same column, the second one moved to the end of its row.  plant =
    r: rows and columns r, r + 1 hold [[1, 2], [2, 4]]."""
    n, half = 601, 20
    rng = np.random.default_rng(601)
    M = np.zeros((n, n))
    for d in range(1, half + 1):
        M[np.arange(d, n), np.arange(0, n - d)] = rng.uniform(-1, 1, n - d)
        M[np.arange(0, n - d), np.arange(d, n)] = rng.uniform(-1, 1, n - d)
    absum = np.abs(M).sum(axis=1)
    M[np.arange(n), np.arange(n)] = absum * rng.uniform(1.1, 1.5, n) + 1e-3
    for z in ZERO_ROWS:
        M[z, z] = 0.0
        M[z, z + 1] = 1.3 * absum[z]
        M[z + 1, z] = -1.2 * absum[z + 1]
    if plant is not None:
        M[plant:plant + 2, plant:plant + 2] = [[1.0, 2.0], [2.0, 4.0]]
    rows, vals = [], []
    for r in range(n):
        c = list(range(max(0, r - half), min(n, r + half + 1)))
        v = [M[r, q] for q in c]
        if dups:
            tail_c, tail_v = [], []
            for q in range(r % 5, len(c), 5):
                part = v[q] * 0.375
                tail_c.append(c[q]); tail_v.append(v[q] - part)
                v[q] = part
            c, v = c + tail_c[::-1], v + tail_v[::-1]
        rows.append(c); vals.append(v)
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int64)
    return CRS(n, rp, np.array([q for c in rows for q in c], dtype=np.int32), np.array([q for v in vals for q in v]))


def mixed_block_ptr(n):
    """Random sizes 1..32 after the fixed start 32, 1, 32, 1, 1; the first seed whose blocks keep every zero-diagonal row
    of the band together with its partner row."""
    for seed in range(100):
        rng = np.random.default_rng(seed)
        sizes = [32, 1, 32, 1, 1]
        while sum(sizes) < n:
            sizes.append(int(min(rng.integers(1, 33), n - sum(sizes))))
        bp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        blk = np.repeat(np.arange(len(sizes)), sizes)
        if all(blk[z] == blk[z + 1] for z in ZERO_ROWS):
            return bp
    raise AssertionError("no seed keeps the pairs together")


# ---- cases ------------------------------------------------------------------------------------------------------------
# name: (matrix maker, block size or None, wants a block_ptr, 64-bit row pointers)
CASES = {
    "fem666": (lambda c: c.gen_fem(6, 6, 6), 3, False, False),
    "fem543": (lambda c: c.gen_fem(5, 4, 3), 3, False, False),
    "hpcg876_bs1": (lambda c: c.gen_hpcg(8, 7, 6), 1, False, False),
    "hpcg876_bs2": (lambda c: c.gen_hpcg(8, 7, 6), 2, False, False),
    "hpcg876_bs5": (lambda c: c.gen_hpcg(8, 7, 6), 5, False, False),
    "hpcg876_bs13": (lambda c: c.gen_hpcg(8, 7, 6), 13, False, False),
    "hpcg876_bs32": (lambda c: c.gen_hpcg(8, 7, 6), 32, False, False),
    "band": (lambda c: c.matrix(band601()), 8, False, False),
    "band_mixed": (lambda c: c.matrix(band601()), None, True, False),
    "band_dups": (lambda c: c.matrix(band601(dups=True)), 8, False, False),
    "hpcg402420_bs7": (lambda c: c.gen_hpcg(40, 24, 20), 7, False, False),
    "fem666_rp64": (lambda c: c.gen_fem(6, 6, 6), 3, False, True),
    "hpcg402420_bs7_rp64": (lambda c: c.gen_hpcg(40, 24, 20), 7, False, True),
}
NAMES = list(CASES)


@pytest.fixture(scope="module")
def built(ctx):
    """Per case, once: the device matrix, its host copy, the restated handles and the device handles (plain, symmetrised)."""
    cache = {}

    def get(name):
        if name not in cache:
            make, bs, mixed, rp64 = CASES[name]
            if rp64:
                with OptionScope(ctx, force_rp64=1):
                    dA = make(ctx)
            else:
                dA = make(ctx)
            assert dA.rp_width == (8 if rp64 else 4)
            A = host_crs(dA)
            bp = mixed_block_ptr(A.n_rows) if mixed else None
            kw = dict(block_ptr=bp) if mixed else dict(block_size=bs)
            cache[name] = dict(dA=dA, A=A, n=A.n_rows, kw=kw,
                               ref=ref.BlockJacobi(A, **kw), ref_sym=ref.BlockJacobi(A, symmetrize=True, **kw),
                               bj=ctx.bjacobi(dA, **kw), bj_sym=ctx.bjacobi(dA, symmetrize=True, **kw))
        return cache[name]

    yield get
    for e in cache.values():
        e["bj"].free(); e["bj_sym"].free(); e["dA"].free()


def dev_apply(ctx, bj, v, alias=False, offset=False, dispatcher=False):
    """bis_bj_apply (or type 11 through bis_apply_preconditioner) on the host vector v; offset: both vectors start one
    element into their allocations (8-byte, not 16-byte aligned)."""
    n = len(v)
    pad = 1 if offset else 0
    din_all = ctx.upload(np.concatenate([np.full(pad, 9.0), v]))
    din = din_all.offset(pad, n)
    dout_all = din_all if alias else ctx.upload(np.full(n + pad, np.nan))
    dout = dout_all.offset(pad, n)
    if dispatcher:
        ctx.apply_preconditioner("bj", n, bj.operand, None, None, None, None, None, dout, din, None, None)
    else:
        bj.apply(dout, din)
    whole = dout_all.to_host()
    if pad:
        assert whole[0] == 9.0 or (not alias and np.isnan(whole[0])), "the element in front of the vector was written"
    din_all.free()
    if not alias:
        dout_all.free()
    return whole[pad:]


def inputs(e):
    rng = np.random.default_rng(29)
    n = e["n"]
    return dict(A1=ref.host_spmv(e["A"], np.ones(n)), uniform=rng.uniform(-1, 1, n), big=1e3 * rng.uniform(-1, 1, n))


# ---- setup ------------------------------------------------------------------------------------------------------------

def test_the_band_makes_the_elimination_swap():
    A = band601()
    blocks = ref.extract(A, ref.block_ptr_of(601, block_size=8))
    for z in ZERO_ROWS:
        B = blocks[z // 8]
        k = z % 8
        assert B[k, k] == 0.0 and k < 7 and abs(B[k + 1, k]) > 0
    assert ref.BlockJacobi(A, block_size=8).singular == []
    assert ref.BlockJacobi(A, block_size=1).singular == sorted(ZERO_ROWS)
    bp = mixed_block_ptr(601)
    sizes = np.diff(bp)
    assert list(sizes[:5]) == [32, 1, 32, 1, 1] and sizes.min() == 1 and sizes.max() == 32 and len(set(sizes)) >= 10


@pytest.mark.parametrize("name", NAMES)
def test_blocks_equal_the_restatement_bit_for_bit(ctx, built, name):
    e = built(name)
    for tag, bj, rj in (("plain", e["bj"], e["ref"]), ("symmetrised", e["bj_sym"], e["ref_sym"])):
        want_vals, want_offs = rj.flat()
        sizes = np.diff(rj.bptr)
        assert bj.info() == (len(sizes), int(sizes.max()), int((sizes * sizes).sum()))
        vals, offs = bj.blocks()
        assert np.array_equal(offs, want_offs)
        differ = np.count_nonzero(vals.view(np.uint64) != want_vals.view(np.uint64))
        print(f"{name} {tag}: {len(sizes)} blocks, largest {sizes.max()}, last {sizes[-1]}, {len(vals)} values, {differ} differ in bits")
        assert rj.singular == [] and differ == 0
        if tag == "symmetrised":
            for b in range(len(sizes)):
                R = vals[offs[b]:offs[b + 1]].reshape(sizes[b], sizes[b])
                assert same_bits(R, R.T.copy()), f"block {b} is not its transpose"
    if name.startswith("band"):
        assert not same_bits(e["bj"].blocks()[0], e["bj_sym"].blocks()[0]), "the band's blocks are not symmetric: symmetrize must change them"


@pytest.mark.parametrize("name", NAMES)
def test_two_creates_give_the_same_bits(ctx, built, name):
    e = built(name)
    again = ctx.bjacobi(e["dA"], **e["kw"])
    assert same_bits(again.blocks()[0], e["bj"].blocks()[0])
    again.free()


# ---- apply ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_apply_equals_the_restated_product_bit_for_bit(ctx, built, name):
    e = built(name)
    for tag, bj, rj in (("plain", e["bj"], e["ref"]), ("symmetrised", e["bj_sym"], e["ref_sym"])):
        for vname, v in inputs(e).items():
            want = rj.apply(v)
            out = dev_apply(ctx, bj, v)
            differ = np.count_nonzero(out.view(np.uint64) != want.view(np.uint64))
            print(f"{name} {tag} {vname}: {differ} of {len(v)} entries differ in bits")
            assert differ == 0
            assert same_bits(dev_apply(ctx, bj, v), want), "a second apply differs"
            assert same_bits(dev_apply(ctx, bj, v, alias=True), want), "out aliasing in differs"
            assert same_bits(dev_apply(ctx, bj, v, offset=True), want), "vectors off a 16-byte boundary differ"
            assert same_bits(dev_apply(ctx, bj, v, alias=True, offset=True), want)
            assert same_bits(dev_apply(ctx, bj, v, dispatcher=True), want), "type 11 through bis_apply_preconditioner differs"
            assert same_bits(dev_apply(ctx, bj, v, alias=True, dispatcher=True), want)


@pytest.mark.parametrize("name", NAMES)
def test_multi_vector_columns_have_the_bits_of_the_single_apply(ctx, built, name):
    e = built(name)
    n, bj = e["n"], e["bj"]
    rng = np.random.default_rng(31)
    for k in (1, 2, 3, 5, 8):
        X = rng.uniform(-1, 1, (n, k)) * (10.0 ** rng.integers(-3, 4, k))[None, :]
        singles = np.stack([dev_apply(ctx, bj, np.ascontiguousarray(X[:, j])) for j in range(k)], axis=1)
        assert same_bits(singles, e["ref"].apply(X)), "the restated multi-vector product differs from the single applies"
        dX, dY = ctx.upload(X.ravel()), ctx.upload(np.full(n * k, np.nan))
        bj.mapply(dY, dX, k)
        assert same_bits(dY.to_host().reshape(n, k), singles), f"k = {k}"
        ctx.init_vector(dY, np.nan)
        ctx.mapply_preconditioner("bj", n, k, bj.operand, None, None, None, None, None, dY, dX, None, None)
        assert same_bits(dY.to_host().reshape(n, k), singles), f"k = {k} through bis_mapply_preconditioner"
        bj.mapply(dX, dX, k)
        assert same_bits(dX.to_host().reshape(n, k), singles), f"k = {k} aliased"
        dX.set(X.ravel())
        ctx.mapply_preconditioner("bj", n, k, bj.operand, None, None, None, None, None, dX, dX, None, None)
        assert same_bits(dX.to_host().reshape(n, k), singles), f"k = {k} aliased through bis_mapply_preconditioner"
        dX.free(); dY.free()


def test_dispatch_refusals(ctx, built):
    from basic_iterative_solvers_amd import BisError
    e = built("fem666")
    n, bj, dA = e["n"], e["bj"], e["dA"]
    x, b = ctx.upload(np.zeros(n)), ctx.upload(np.ones(n))
    X, B = ctx.upload(np.zeros(2 * n)), ctx.upload(np.ones(2 * n))
    with pytest.raises(BisError, match="status 6"):
        ctx.apply_preconditioner("bj", n, bj.operand, None, None, None, None, None, x, b, None, None, outer=2)
    with pytest.raises(BisError, match="status 6"):
        ctx.mapply_preconditioner("bj", n, 2, bj.operand, None, None, None, None, None, X, B, None, None, outer=2)
    for op in (bj.operand, dA, None):  # an operand of another size, a matrix that is no operand, none
        size = n - 3 if op is bj.operand else n
        with pytest.raises(BisError, match="status 2"):
            ctx.apply_preconditioner("bj", size, op, None, None, None, None, None, x, b, None, None)
        with pytest.raises(BisError, match="status 2"):
            ctx.mapply_preconditioner("bj", size, 2, op, None, None, None, None, None, X, B, None, None)
    for k in (0, 9):
        with pytest.raises(BisError, match="status 2"):
            bj.mapply(X, B, k)
        with pytest.raises(BisError, match="status 2"):
            ctx.mapply_preconditioner("bj", n, k, bj.operand, None, None, None, None, None, X, B, None, None)
    solvers = [ctx.cg(dA, b, x), ctx.minres(dA, b, x), ctx.fgmres(dA, b, x), ctx.mcg(dA, B, X, 2), ctx.mbicgstab(dA, B, X, 2),
               ctx.mgmres(dA, B, X, 2)]
    small = ctx.bjacobi(built("fem543")["dA"], block_size=3)
    for s in solvers:
        with pytest.raises(BisError, match="status 2"):
            s.set_preconditioner("bj", Ls=small.operand)
        with pytest.raises(BisError, match="status 2"):
            s.set_preconditioner("bj", Ls=dA)
        with pytest.raises(BisError, match="status 6"):
            s.set_preconditioner("bj", Ls=bj.operand, outer=2)
        s.set_preconditioner(bj)  # the object stands for its type and operand
        s.free()
    small.free()
    # every other entry point sees the zero matrix, and destroying the operand does nothing
    y = ctx.upload(np.full(n, 7.0))
    ctx.spmv(bj.operand, b, y)
    assert not y.to_host().any()
    assert ctx.lib.bis_mat_destroy(ctx.h, bj.operand.h) == 0
    assert same_bits(dev_apply(ctx, bj, np.ones(n)), e["ref"].apply(np.ones(n)))
    for v in (x, b, X, B, y):
        v.free()


# ---- errors -----------------------------------------------------------------------------------------------------------

def raw_create(ctx, A_h, block_size=0, block_ptr=None, symmetrize=0, with_params=True, with_out=True):
    from basic_iterative_solvers_amd import BJParams
    if block_ptr is not None:
        bp = np.ascontiguousarray(block_ptr, dtype=np.int32)
        params = BJParams(block_size, bp.ctypes.data_as(C.POINTER(C.c_int32)), len(bp) - 1, symmetrize)
    else:
        params = BJParams(block_size, None, 0, symmetrize)
    out = C.c_void_p()
    st = ctx.lib.bis_bj_create(ctx.h, A_h, C.byref(params) if with_params else None, C.byref(out) if with_out else None)
    return st, out


def test_errors(ctx):
    dA = ctx.matrix(band601())
    n = 601
    uniform8 = list(range(0, n, 8)) + [n]
    # null arguments
    for st, out in (raw_create(ctx, None, 8), raw_create(ctx, dA.h, 8, with_params=False)):
        assert st == INVALID and not out
    assert raw_create(ctx, dA.h, 8, with_out=False)[0] == INVALID
    # A not square
    wide = band601()
    dW = ctx.matrix(CRS(n, wide.row_ptr, wide.col, wide.val, n_cols=n + 2))
    st, out = raw_create(ctx, dW.h, 8)
    assert st == INVALID and not out
    dW.free()
    # block_size outside 1..32
    for bs in (0, 33, -1):
        st, out = raw_create(ctx, dA.h, bs)
        assert st == INVALID and not out, bs
    # block_ptr: does not start at 0, does not ascend strictly, does not end at n, a block of more than 32 rows
    bad = {"starts at 1": [1] + uniform8[1:], "repeats a row": uniform8[:5] + [uniform8[4]] + uniform8[5:],
           "descends": uniform8[:5] + [uniform8[3]] + uniform8[5:], "ends before n": uniform8[:-1],
           "ends after n": uniform8[:-1] + [n + 1], "33 rows": [0, 33] + list(range(40, n, 8)) + [n]}
    for why, bp in bad.items():
        st, out = raw_create(ctx, dA.h, 8, block_ptr=bp)
        assert st == INVALID and not out, why
    st, out = raw_create(ctx, dA.h, 99, block_ptr=uniform8)  # (block_size is ignored beside a block_ptr)
    assert st == 0 and out
    ctx.lib.bis_bj_destroy(ctx.h, out)
    # a zero pivot: a block of one row on a zero diagonal entry; block [[1, 2], [2, 4]] planted in the band
    st, out = raw_create(ctx, dA.h, 1)
    assert st == ZERO_DIAG and not out
    dA.free()
    planted = band601(plant=96)
    bp = list(range(0, 96, 8)) + [96, 98] + list(range(106, n, 8)) + [n]
    assert ref.BlockJacobi(planted, block_ptr=bp).singular == [12]
    dP = ctx.matrix(planted)
    for sym in (0, 1):
        st, out = raw_create(ctx, dP.h, block_ptr=bp, symmetrize=sym)
        assert st == ZERO_DIAG and not out
    ok = ctx.bjacobi(dP, block_size=8)  # inside a block of 8 rows the planted entries make no singular block
    assert ok.info()[0] == 76
    ok.free()
    # a pivot that is not finite
    inf = band601()
    inf.val[inf.row_ptr[300] + 20] = np.inf  # the diagonal entry of row 300
    assert inf.col[inf.row_ptr[300] + 20] == 300
    dI = ctx.matrix(inf)
    st, out = raw_create(ctx, dI.h, 8)
    assert st == ZERO_DIAG and not out
    dI.free(); dP.free()


def test_no_rows_and_one_row(ctx):
    empty = ctx.matrix(CRS(0, np.zeros(1, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0)))
    for kw in (dict(block_size=4), dict(block_ptr=[0])):
        bj = ctx.bjacobi(empty, **kw)
        assert bj.info() == (0, 0, 0) and bj.operand.n_rows == 0
        ctx.check(ctx.lib.bis_bj_apply(ctx.h, bj.h, None, None))
        ctx.check(ctx.lib.bis_bj_mapply(ctx.h, bj.h, None, None, 3))
        ctx.apply_preconditioner("bj", 0, bj.operand, None, None, None, None, None, None, None, None, None)
        vals, offs = bj.blocks()
        assert len(vals) == 0 and list(offs) == [0]
        bj.free()
    empty.free()
    one = ctx.matrix(CRS(1, np.array([0, 1], dtype=np.int64), np.zeros(1, np.int32), np.array([-2.5])))
    bj = ctx.bjacobi(one, block_size=32)
    assert bj.info() == (1, 1, 1) and bj.blocks()[0][0] == 1.0 / -2.5
    assert dev_apply(ctx, bj, np.array([3.0]))[0] == (1.0 / -2.5) * 3.0
    bj.free(); one.free()


# ---- solves -----------------------------------------------------------------------------------------------------------
ITERS = 400


def report(tag, run, want, true, r0, gate):
    dev = hist_dev(run["hist"], want["hist"])
    print(f"{tag}: device {run['iters']} iterations conv {run['conv']}, numpy {want['iters']} conv {want['conv']}, history entries "
          f"{len(run['hist'])} / {len(want['hist'])}, hist dev {dev:.3e} (gate {gate:.0e}), residual of x {true:.6e}, last entry "
          f"{run['hist'][-1]:.6e}, r0 {r0:.6e}")
    assert run["conv"] and want["conv"]
    assert run["iters"] == want["iters"] and len(run["hist"]) == len(want["hist"])
    assert dev <= gate
    assert abs(true - run["hist"][-1]) <= gate * r0


@pytest.fixture(scope="module")
def fem888(ctx):
    dA = ctx.gen_fem(8, 8, 8)
    A = host_crs(dA)
    e = dict(dA=dA, A=A, n=A.n_rows, b=np.random.default_rng(41).uniform(-1, 1, A.n_rows), bj=ctx.bjacobi(dA, block_size=3, symmetrize=True),
             ref=ref.BlockJacobi(A, block_size=3, symmetrize=True))
    yield e
    e["bj"].free(); dA.free()


def test_cg_on_fem888(ctx, fem888):
    e, tol = fem888, 1e-10
    A, b, n = e["A"], e["b"], e["n"]
    counts = {}
    for pc in ("bj", "j"):
        db, dx = ctx.upload(b), ctx.upload(np.zeros(n))
        if pc == "bj":
            cg = ctx.cg(e["dA"], db, dx)
            cg.set_preconditioner(e["bj"])
        else:
            D, Dinv = ctx.mat_diag(e["dA"])
            cg = ctx.cg(e["dA"], db, dx, A_D=D)
        cg.init(tol)
        cg.iterate(ITERS)
        iters, conv, hist = cg.status()
        counts[pc] = (iters, conv)
        if pc == "bj":
            run = dict(iters=iters, conv=conv, hist=hist, x=dx.to_host())
        else:
            D.free(); Dinv.free()
        cg.free(); db.free(); dx.free()
    want = ref.np_pcg(A, e["ref"].apply, b, tol, ITERS)
    print(f"fem 8x8x8, CG, tol {tol:g}: block Jacobi (3, symmetrised) {counts['bj'][0]} iterations, point Jacobi {counts['j'][0]} "
          f"(converged {counts['bj'][1]} / {counts['j'][1]})")
    report("CG + bj", run, want, np.linalg.norm(b - ref.host_spmv(A, run["x"])), want["hist"][0], HIST_TOL["cg"])


def test_minres_on_fem888(ctx, fem888):
    e, tol = fem888, 1e-10
    A, b, n = e["A"], e["b"], e["n"]
    db, dx = ctx.upload(b), ctx.upload(np.zeros(n))
    s = ctx.minres(e["dA"], db, dx)
    s.set_preconditioner(e["bj"])
    s.init(tol)
    s.iterate(ITERS)
    iters, conv, hist = s.status()
    run = dict(iters=iters, conv=conv, hist=hist, x=dx.to_host())
    s.free(); db.free(); dx.free()
    want = ref.np_minres(A, e["ref"].apply, b, tol, ITERS)
    r = b - ref.host_spmv(A, run["x"])
    report("MINRES + bj", run, want, float(np.sqrt(r @ e["ref"].apply(r))), want["hist"][0], HIST_TOL["cg"])  # phibar: the M^-1 norm


def band_system(built):
    e = built("band")
    rng = np.random.default_rng(43)
    return e, rng.uniform(-1, 1, (e["n"], 3))


def test_fgmres_on_the_band(ctx, built):
    e, B = band_system(built)
    A, n, tol, m = e["A"], e["n"], 1e-9, 10
    b = np.ascontiguousarray(B[:, 0])
    db, dx = ctx.upload(b), ctx.upload(np.zeros(n))
    s = ctx.fgmres(e["dA"], db, dx, restart=m)
    s.set_preconditioner(e["bj"])
    s.init(tol)
    s.iterate(ITERS)
    iters, conv, hist = s.status()
    run = dict(iters=iters, conv=conv, hist=hist, x=dx.to_host())
    s.free(); db.free(); dx.free()
    want = ref.np_gmres(A, e["ref"].apply, b, np.zeros(n), m, tol, ITERS, right=True)
    report("FGMRES(10) + bj", run, want, np.linalg.norm(b - ref.host_spmv(A, run["x"])), want["hist"][0], HIST_TOL["gm"])


def test_lockstep_bicgstab_on_the_band(ctx, built):
    e, B = band_system(built)
    A, n, tol, k = e["A"], e["n"], 1e-8, 3
    dB, dX = ctx.upload(B.ravel()), ctx.upload(np.zeros(n * k))
    s = ctx.mbicgstab(e["dA"], dB, dX, k)
    s.set_preconditioner(e["bj"])
    s.init(tol)
    s.iterate(ITERS)
    X = None
    for j in range(k):
        iters, conv, hist = s.status(j)
        X = dX.to_host().reshape(n, k) if X is None else X
        b = np.ascontiguousarray(B[:, j])
        want = ref.np_bicgstab(A, e["ref"].apply, b, np.zeros(n), tol, ITERS)
        run = dict(iters=iters, conv=conv, hist=hist)
        report(f"MBiCGSTAB + bj, column {j}", run, want, np.linalg.norm(b - ref.host_spmv(A, X[:, j])), want["hist"][0], HIST_TOL["bi"])
    s.free(); dB.free(); dX.free()


def test_lockstep_cg_and_gmres_on_fem666(ctx, built):
    e = built("fem666")
    A, n, tol = e["A"], e["n"], 1e-9
    rng = np.random.default_rng(47)
    B = rng.uniform(-1, 1, (n, 4))
    B[:, 0] = ref.host_spmv(A, np.ones(n))
    # MCG, k = 4, the symmetrised handle
    k = 4
    dB, dX = ctx.upload(B.ravel()), ctx.upload(np.zeros(n * k))
    s = ctx.mcg(e["dA"], dB, dX, k)
    s.set_preconditioner(e["bj_sym"])
    s.init(tol)
    s.iterate(ITERS)
    st = [s.status(j) for j in range(k)]
    X = dX.to_host().reshape(n, k)
    s.free(); dB.free(); dX.free()
    for j in range(k):
        b = np.ascontiguousarray(B[:, j])
        want = ref.np_pcg(A, e["ref_sym"].apply, b, tol, ITERS)
        run = dict(iters=st[j][0], conv=st[j][1], hist=st[j][2])
        report(f"MCG + bj, column {j}", run, want, np.linalg.norm(b - ref.host_spmv(A, X[:, j])), want["hist"][0], HIST_TOL["cg"])
    # MGMRES(10), k = 2: the history is the estimate of || M^-1 r ||
    k, m = 2, 10
    B2 = np.ascontiguousarray(B[:, 1:3])
    dB, dX = ctx.upload(B2.ravel()), ctx.upload(np.zeros(n * k))
    s = ctx.mgmres(e["dA"], dB, dX, k, restart=m)
    s.set_preconditioner(e["bj"])
    s.init(tol)
    s.iterate(ITERS)
    st = [s.status(j) for j in range(k)]
    X = dX.to_host().reshape(n, k)
    s.free(); dB.free(); dX.free()
    for j in range(k):
        b = np.ascontiguousarray(B2[:, j])
        want = ref.np_gmres(A, e["ref"].apply, b, np.zeros(n), m, tol, ITERS, right=False)
        run = dict(iters=st[j][0], conv=st[j][1], hist=st[j][2])
        true = np.linalg.norm(e["ref"].apply(b - ref.host_spmv(A, X[:, j])))
        report(f"MGMRES(10) + bj, column {j}", run, want, true, want["hist"][0], HIST_TOL["gm"])
