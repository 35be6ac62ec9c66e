"""GPU: the aggregation multigrid preconditioner (bis_mg_*, BIS_PC_MG / "mg") against a numpy restatement of the
definitions in include/bis_hip.h: the aggregates entry for entry (grid and MIS, with the MIS invariants), the smoother
weights and the Galerkin operators bit for bit (both row-pointer widths), the shape of the hierarchy, the error table, the
V-cycle, and the fused CG against a numpy PCG with the restated cycle.

Reference: `hierarchy_reference` and `cycle_reference` below.  Where the gate is "the same bits" (aggregates, weights,
Galerkin values) the restatement runs the stated fp64 operations in the stated order.  Where it is a tolerance (the cycle)
the restatement's SpMV sums its products in np.longdouble and rounds once; the gate is 1e-13 |.|_inf, the project's kernel
gate.

One row of the error table has no test: a row-range view cannot be made through the public interface (bis_mat_row_view is
internal to the library), so BIS_ERR_INVALID for a view is covered by the code only."""
import ctypes as C

import numpy as np
import pytest

from helpers import HIST_TOL, OptionScope, hist_dev
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

LD = np.longdouble
GATE = 1e-13
INVALID, ZERO_DIAG, UNSUPPORTED = 2, 4, 6
DEFAULTS = dict(max_levels=10, coarse_limit=256, coarsening=0, nu=1, coarse_sweeps=4, omega=0.0, coarse_scale=1.0)


# ---- host side: inputs ---------------------------------------------------------------------------------------------

def crs_from_dense(M, keep=None):
    keep = (M != 0.0) if keep is None else keep
    n = M.shape[0]
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    r, c = np.nonzero(keep)
    return CRS(n, rp, c.astype(np.int32), M[r, c], n_cols=M.shape[1])


def band_dense(n, half, density, seed):
    """Symmetric band, each off-diagonal pair present with probability `density`, strictly dominant diagonal: SPD."""
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


def band600_isolated():
    """The band with three rows cut off from every other row (rows without off-diagonal entries) and some equal
    off-diagonal magnitudes (ties between root neighbours)."""
    M = band600()
    for i in (0, 311, 599):
        d = M[i, i]
        M[i, :] = 0.0
        M[:, i] = 0.0
        M[i, i] = d
    off = M != 0.0
    np.fill_diagonal(off, False)
    M[off] = np.sign(M[off]) * np.round(np.abs(M[off]) * 4 + 0.5) / 4  # magnitudes from {0.25, 0.5, ..., 1.25}
    return M


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def rows_of(A):
    return np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))


def host_spmv(A, x):
    """y = A x with the products and the row sums in longdouble, rounded once (every row has an entry)."""
    prod = A.val.astype(LD) * x.astype(LD)[A.col]
    return np.add.reduceat(prod, A.row_ptr[:-1]).astype(np.float64)


# ---- the restatement -----------------------------------------------------------------------------------------------

def run_sums(v, start, end):
    """Per run [start, end) of v the fp64 sum taken left to right, the first value starting it."""
    acc = v[start].copy()
    length = end - start
    for j in range(1, int(length.max()) if len(length) else 0):
        m = length > j
        acc[m] = acc[m] + v[start[m] + j]
    return acc


def weights_reference(A, omega):
    if omega > 0:
        rows = rows_of(A)
        d = np.zeros(A.n_rows)
        for k in np.flatnonzero(A.col == rows)[::-1]:  # (the first diagonal entry of a row wins)
            d[rows[k]] = A.val[k]
        return omega / d
    a = np.abs(A.val)
    s = np.zeros(A.n_rows)
    start, length = A.row_ptr[:-1], np.diff(A.row_ptr)
    for j in range(int(length.max())):
        m = length > j
        s[m] = s[m] + a[start[m] + j]
    return 1.0 / s


def grid_aggregates(n, g):
    nx, ny, nz, dof = g
    cx, cy, cz = (nx + 1) // 2, (ny + 1) // 2, (nz + 1) // 2
    i = np.arange(n)
    d, node = i % dof, i // dof
    x, t = node % nx, node // nx
    y, z = t % ny, t // ny
    return ((((z // 2) * cy + y // 2) * cx + x // 2) * dof + d).astype(np.int32), (cx, cy, cz, dof)


def hash32(i):
    x = np.uint64(i) & np.uint64(0xffffffff)
    m = np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & m
    x ^= x >> np.uint64(16)
    return int(x)


def mis_aggregates(A):
    """Sequential greedy MIS in descending (hash32(i), i) order over the off-diagonal pattern, then the members."""
    n = A.n_rows
    order = sorted(range(n), key=lambda i: (hash32(i), i), reverse=True)
    root = np.zeros(n, dtype=bool)
    nbrs = []
    for i in range(n):
        s, e = A.row_ptr[i], A.row_ptr[i + 1]
        keep = A.col[s:e] != i
        nbrs.append((A.col[s:e][keep], np.abs(A.val[s:e][keep])))
    for i in order:
        if not root[nbrs[i][0]].any():
            root[i] = True
    number = np.cumsum(root) - 1
    agg = np.zeros(n, dtype=np.int32)
    for i in range(n):
        if root[i]:
            agg[i] = number[i]
            continue
        c, a = nbrs[i]
        m = root[c]
        assert m.any(), "not maximal"
        c, a = c[m], a[m]
        best = c[a == a.max()].min()
        agg[i] = number[best]
    return agg, root


def galerkin_reference(A, agg, nc):
    rows = rows_of(A)
    key = (agg[rows].astype(np.int64) << 32) | agg[A.col].astype(np.int64)
    order = np.argsort(key, kind="stable")
    ks, vs = key[order], A.val[order]
    start = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    end = np.concatenate([start[1:], [len(ks)]])
    val = run_sums(vs, start, end)
    r_c, c_c = ks[start] >> 32, (ks[start] & 0xffffffff).astype(np.int32)
    rp = np.searchsorted(r_c, np.arange(nc + 1)).astype(np.int64)
    return CRS(nc, rp, c_c, val)


def hierarchy_reference(A, grid, **kw):
    """The levels of bis_mg_create: dicts of A, grid, w, agg (None on the coarsest level), kind; where the MIS ran, root (the
    flags of its roots) as well."""
    p = dict(DEFAULTS, **kw)
    levels = []
    while True:
        n = A.n_rows
        L = dict(A=A, grid=grid, w=weights_reference(A, p["omega"]), agg=None, kind=0)
        levels.append(L)
        if n <= p["coarse_limit"] or len(levels) >= p["max_levels"]:
            break
        use_grid = p["coarsening"] != 2 and grid is not None and int(np.prod(grid)) == n
        if use_grid:
            agg, cgrid = grid_aggregates(n, grid)
            nc = int(np.prod(cgrid))
        else:
            agg, L["root"] = mis_aggregates(A)
            cgrid, nc = None, int(agg.max()) + 1
        if 5 * nc > 4 * n:
            break
        L["agg"], L["kind"] = agg, 1 if use_grid else 2
        A, grid = galerkin_reference(A, agg, nc), cgrid
    return levels


def cycle_reference(levels, b, nu=1, coarse_sweeps=4, coarse_scale=1.0, l=0):
    L = levels[l]
    A, w = L["A"], L["w"]

    def sweep(x):
        return x + w * (b - host_spmv(A, x))

    x = w * b
    if l + 1 == len(levels):
        for _ in range(coarse_sweeps - 1):
            x = sweep(x)
        return x
    for _ in range(nu - 1):
        x = sweep(x)
    d = b - host_spmv(A, x)
    agg = L["agg"]
    order = np.argsort(agg, kind="stable")  # members in ascending row order
    ptr = np.searchsorted(agg[order], np.arange(int(agg.max()) + 2))
    rc = run_sums(d[order], ptr[:-1], ptr[1:])
    ec = cycle_reference(levels, rc, nu, coarse_sweeps, coarse_scale, l + 1)
    x = x + coarse_scale * ec[agg]
    for _ in range(nu):
        x = sweep(x)
    return x


def numpy_pcg(A, apply, b, tol, max_iters):
    """Preconditioned CG from x0 = 0 with z = apply(r); the residual history and x."""
    x = np.zeros_like(b)
    r = b.copy()
    z = apply(r)
    p = z.copy()
    rz = r @ z
    hist = [np.linalg.norm(r)]
    while len(hist) - 1 < max_iters and not hist[-1] < tol * hist[0]:
        Ap = host_spmv(A, p)
        alpha = rz / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        z = apply(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
        hist.append(np.linalg.norm(r))
    return np.array(hist), x


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


def grid_of(dA):
    g = dA.grid_hint()
    return tuple(int(v) for v in g) if g[0] > 0 else None


def downloaded(mg):
    """The device hierarchy in the restatement's form."""
    out = []
    for l in range(mg.levels):
        M = mg.level_matrix(l)
        out.append(dict(A=host_crs(M), grid=grid_of(M), w=mg.weights(l), kind=mg.kinds[l],
                        agg=mg.aggregates(l) if mg.kinds[l] else None, rp_width=M.rp_width))
    return out


MATRICES = {
    "hpcg876": lambda c: c.gen_hpcg(8, 7, 6),
    "fem666": lambda c: c.gen_fem(6, 6, 6),
    "unstr666": lambda c: c.gen_unstr(6, 6, 6),
    "band600": lambda c: c.matrix(crs_from_dense(band600())),
    "band600_isolated": lambda c: c.matrix(crs_from_dense(band600_isolated())),
    "hpcg402420": lambda c: c.gen_hpcg(40, 24, 20),
}
KIND = {"hpcg876": 1, "fem666": 1, "unstr666": 2, "band600": 2, "band600_isolated": 2, "hpcg402420": 1}
SETUP = dict(coarse_limit=30)


@pytest.fixture(scope="module")
def built(ctx):
    """Per matrix, computed once and left alone: the matrix, its host copy, the hierarchy at SETUP and its download."""
    cache = {}

    def get(name):
        if name not in cache:
            dA = MATRICES[name](ctx)
            mg = ctx.mg(dA, **SETUP)
            cache[name] = dict(dA=dA, A=host_crs(dA), grid=grid_of(dA), mg=mg, dev=downloaded(mg))
        return cache[name]
    return get


def compare_hierarchies(dev, ref, tag):
    assert len(dev) == len(ref), f"{tag}: {len(dev)} levels instead of {len(ref)}"
    for l, (d, r) in enumerate(zip(dev, ref)):
        assert d["A"].n_rows == r["A"].n_rows and d["kind"] == r["kind"], (tag, l)
        assert d["grid"] == r["grid"], (tag, l, d["grid"], r["grid"])
        assert same_bits(d["w"], r["w"]), f"{tag}: weights of level {l}"
        if r["agg"] is not None:
            assert np.array_equal(d["agg"], r["agg"]), f"{tag}: aggregates of level {l}"
        if l > 0:
            a, b = d["A"], r["A"]
            assert np.array_equal(a.row_ptr, b.row_ptr) and np.array_equal(a.col, b.col), f"{tag}: pattern of level {l}"
            assert same_bits(a.val, b.val), f"{tag}: values of level {l}"
            lens = np.diff(a.row_ptr)
            inner = np.ones(len(a.col), dtype=bool)
            inner[a.row_ptr[:-1][lens > 0]] = False
            assert np.all(np.diff(a.col.astype(np.int64))[inner[1:]] > 0), f"{tag}: columns of level {l} do not ascend"


@pytest.mark.parametrize("name", ["hpcg876", "fem666", "unstr666", "band600", "band600_isolated"])
def test_aggregates_weights_and_galerkin_operators(built, name):
    e = built(name)
    ref = hierarchy_reference(e["A"], e["grid"], **SETUP)
    print(f"{name}: rows {[L['A'].n_rows for L in e['dev']]}, kinds {[L['kind'] for L in e['dev']]}")
    assert e["dev"][0]["kind"] == KIND[name] and len(e["dev"]) >= 2
    compare_hierarchies(e["dev"], ref, name)


def check_mis_invariants(A, agg, root_ref=None):
    """The MIS invariants of the aggregates `agg` of A: the roots (root_ref: those of the restatement, computed here if not
    given) are numbered by ascending row, independent and maximal, every member is adjacent to the root of its aggregate, and
    a row without off-diagonal entries is a root.  Returns those rows."""
    n, nc = A.n_rows, int(agg.max()) + 1
    rows = rows_of(A)
    off = A.col != rows
    # the roots: aggregate I's root is the row that the ascending numbering points at
    if root_ref is None:
        _, root_ref = mis_aggregates(A)
    first = np.full(nc, -1)
    root_rows = np.flatnonzero(root_ref)
    assert len(root_rows) == nc
    first[agg[root_rows]] = root_rows
    assert np.array_equal(agg[root_rows], np.arange(nc)), "aggregates are not numbered by ascending root row"
    is_root = np.zeros(n, dtype=bool)
    is_root[root_rows] = True
    # independent: no entry joins two roots
    assert not np.any(is_root[rows[off]] & is_root[A.col[off]])
    # maximal, and every member is adjacent to its root
    adjacent = set(zip(rows[off].tolist(), A.col[off].tolist()))
    for i in np.flatnonzero(~is_root):
        assert (int(i), int(first[agg[i]])) in adjacent, f"row {i} is not adjacent to the root of its aggregate"
    # a row without off-diagonal entries is a root
    lonely = np.flatnonzero(np.bincount(rows[off], minlength=n) == 0)
    assert np.all(is_root[lonely])
    return lonely


@pytest.mark.parametrize("name", ["unstr666", "band600", "band600_isolated"])
def test_mis_invariants(built, name):
    e = built(name)
    lonely = check_mis_invariants(e["A"], e["dev"][0]["agg"])
    if name == "band600_isolated":
        assert len(lonely) == 3


def test_two_setups_give_the_same_bits(ctx, built):
    for name in ("unstr666", "hpcg876"):
        e = built(name)
        mg2 = ctx.mg(e["dA"], **SETUP)
        again = downloaded(mg2)
        assert len(again) == len(e["dev"])
        for a, b in zip(again, e["dev"]):
            assert np.array_equal(a["A"].row_ptr, b["A"].row_ptr) and np.array_equal(a["A"].col, b["A"].col)
            assert same_bits(a["A"].val, b["A"].val) and same_bits(a["w"], b["w"])
            assert (a["agg"] is None) == (b["agg"] is None) and (a["agg"] is None or np.array_equal(a["agg"], b["agg"]))
        mg2.free()


@pytest.mark.parametrize("name", ["hpcg876", "unstr666"])
def test_64_bit_row_pointers(ctx, built, name):
    e = built(name)
    with OptionScope(ctx, force_rp64=1):
        dA = MATRICES[name](ctx)
        assert dA.rp_width == 8
        mg = ctx.mg(dA, **SETUP)
        dev = downloaded(mg)
    assert all(L["rp_width"] == 8 for L in dev) and all(L["rp_width"] == 4 for L in e["dev"])
    for L in dev + e["dev"]:
        L.pop("rp_width")
    compare_hierarchies(dev, e["dev"], name + " rp64")  # the row-pointer width changes nothing else
    mg.free()
    dA.free()


def test_hierarchy_shapes(ctx, built):
    mg = ctx.mg(built("hpcg876")["dA"], coarse_limit=8)
    assert mg.rows == [336, 48, 8] and mg.kinds == [1, 1, 0] and mg.levels == 3
    assert [grid_of(mg.level_matrix(l)) for l in range(3)] == [(8, 7, 6, 1), (4, 4, 3, 1), (2, 2, 2, 1)]
    assert mg.nnz[0] == built("hpcg876")["A"].row_ptr[-1] and mg.operand.n_rows == 336 and mg.operand.nnz == 0
    mg.free()
    mg = ctx.mg(built("fem666")["dA"], coarse_limit=30)
    assert mg.rows == [648, 81, 24] and mg.kinds == [1, 1, 0]
    assert [grid_of(mg.level_matrix(l)) for l in range(3)] == [(6, 6, 6, 3), (3, 3, 3, 3), (2, 2, 2, 3)]
    mg.free()
    # max_levels cuts the hierarchy; coarsening = mis ignores the hint
    mg = ctx.mg(built("hpcg876")["dA"], coarse_limit=8, max_levels=2)
    assert mg.rows == [336, 48] and mg.kinds == [1, 0]
    mg.free()
    mg = ctx.mg(built("hpcg876")["dA"], coarse_limit=30, coarsening="mis")
    assert mg.kinds[0] == 2 and grid_of(mg.level_matrix(1)) is None
    mg.free()
    # a diagonal matrix: every row is a root, the step is dropped
    dD = ctx.matrix(crs_from_dense(np.diag(np.arange(1.0, 301.0))))
    mg = ctx.mg(dD, coarse_limit=30)
    assert mg.rows == [300] and mg.kinds == [0]
    mg.free()
    dD.free()


def apply_host(ctx, mg, v, alias=False, through_dispatcher=False):
    n = len(v)
    din = ctx.upload(v)
    dout = din if alias else ctx.upload(np.full(n, np.nan))
    if through_dispatcher:
        ctx.apply_preconditioner("mg", n, mg.operand, None, None, None, None, None, dout, din, None, None)
    else:
        mg.apply(dout, din)
    out = dout.to_host()
    din.free()
    if not alias:
        dout.free()
    return out


def test_smoother_only_one_row_and_no_rows(ctx, built):
    e = built("hpcg876")
    v = np.random.default_rng(5).uniform(-1, 1, 336)
    mg = ctx.mg(e["dA"], max_levels=1, coarse_sweeps=3)
    assert mg.levels == 1 and mg.rows == [336]
    ref = cycle_reference(downloaded(mg), v, coarse_sweeps=3)
    out = apply_host(ctx, mg, v)
    assert np.max(np.abs(out - ref)) <= GATE * np.max(np.abs(ref))
    mg.free()
    one = ctx.matrix(CRS(1, np.array([0, 1], dtype=np.int64), np.zeros(1, np.int32), np.array([-2.5])))
    mg = ctx.mg(one)
    assert mg.levels == 1 and mg.rows == [1]
    # x = w b = 0.4 b, then three sweeps x += 0.4 (b - (-2.5) x)
    x = 0.4 * 3.0
    for _ in range(3):
        x = x + 0.4 * (3.0 - (-2.5 * x))
    assert apply_host(ctx, mg, np.array([3.0]))[0] == x
    mg.free()
    one.free()
    empty = ctx.matrix(CRS(0, np.zeros(1, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0)))
    mg = ctx.mg(empty)
    assert mg.levels == 1 and mg.rows == [0] and mg.operand.n_rows == 0
    ctx.check(ctx.lib.bis_mg_apply(ctx.h, mg.h, None, None))
    mg.free()
    empty.free()


def raw_create(ctx, A_h, with_out=True, **kw):
    from basic_iterative_solvers_amd import MGParams
    p = dict(DEFAULTS, **kw)
    params = MGParams(p["max_levels"], p["coarse_limit"], p["coarsening"], p["nu"], p["coarse_sweeps"], p["omega"], p["coarse_scale"])
    out = C.c_void_p()
    st = ctx.lib.bis_mg_create(ctx.h, A_h, C.byref(params), C.byref(out) if with_out else None)
    return st, out


def test_errors(ctx):
    base = band_dense(40, 3, 1.1, 1)
    keep = base != 0.0

    def status_of(M, mask=None, crs=None, **kw):
        dA = ctx.matrix(crs if crs is not None else crs_from_dense(M, mask))
        st, out = raw_create(ctx, dA.h, **kw)
        assert not out, "*out written on an error"
        dA.free()
        return st

    # BIS_ERR_INVALID: null arguments, not square, bad parameters, grid-only coarsening without a hint
    dA = ctx.matrix(crs_from_dense(base))
    assert raw_create(ctx, None)[0] == INVALID
    assert raw_create(ctx, dA.h, with_out=False)[0] == INVALID
    for bad in (dict(max_levels=0), dict(max_levels=17), dict(coarse_limit=0), dict(coarsening=3), dict(coarsening=-1), dict(nu=0),
                dict(coarse_sweeps=0), dict(omega=-0.5), dict(omega=float("nan"))):
        st, out = raw_create(ctx, dA.h, **bad)
        assert st == INVALID and not out, bad
    st, out = raw_create(ctx, dA.h, coarsening=1, coarse_limit=8)
    assert st == INVALID and not out
    st, out = raw_create(ctx, dA.h, coarse_limit=8)  # (the matrix itself is fine; NULL parameters are the defaults)
    assert st == 0 and out
    ctx.lib.bis_mg_destroy(ctx.h, out)
    out = C.c_void_p()
    assert ctx.lib.bis_mg_create(ctx.h, dA.h, None, C.byref(out)) == 0 and out
    ctx.lib.bis_mg_destroy(ctx.h, out)
    dA.free()
    assert status_of(None, crs=crs_from_dense(np.hstack([base, np.zeros((40, 2))]))) == INVALID
    # BIS_ERR_ZERO_DIAG: a row without a diagonal entry, a stored zero on the diagonal -- on level 0 ...
    no_diag = keep.copy()
    no_diag[17, 17] = False
    assert status_of(base, no_diag, coarse_limit=8) == ZERO_DIAG
    zero = base.copy()
    zero[23, 23] = 0.0
    assert status_of(zero, keep, coarse_limit=8) == ZERO_DIAG
    # ... and on a coarse level: the aggregate {0, 1} of a 1 x 4 x 1 grid sums [[1, -1], [-1, 1]] to a stored zero
    T = np.array([[1.0, -1, 0, 0], [-1, 1, -0.5, 0], [0, -0.5, 2, -1], [0, 0, -1, 2]])
    dT = ctx.matrix(crs_from_dense(T))
    dT.set_grid_hint(4, 1, 1)
    st, out = raw_create(ctx, dT.h, coarse_limit=1)
    assert st == ZERO_DIAG and not out
    dT.free()
    # BIS_ERR_UNSUPPORTED: MIS aggregates of a pattern that is not structurally symmetric
    for drop in ([(10, 12)], [(12, 10)], [(10, 12), (31, 30)]):
        m = keep.copy()
        for rc in drop:
            assert m[rc]
            m[rc] = False
        assert status_of(base, m, coarse_limit=8) == UNSUPPORTED, drop


APPLY_CASES = ["hpcg876", "fem666", "unstr666", "band600", "hpcg402420"]


@pytest.mark.parametrize("name", APPLY_CASES)
def test_cycle_against_the_restatement(ctx, built, name):
    e = built(name)
    n = e["A"].n_rows
    v = np.random.default_rng(11).uniform(-1, 1, n)
    if name == "hpcg402420":
        M = e["dA"]
        layout = M.win8_layout()
        print(f"{name}: SpMV kernel form {M.spmv_stream_info()[3]}, win8 layout {layout}")
    worst = 0.0
    for omega in (0.0, 0.6):
        mg = e["mg"] if omega == 0.0 else ctx.mg(e["dA"], omega=omega, **SETUP)
        levels = e["dev"] if omega == 0.0 else downloaded(mg)
        assert len(levels) >= 2
        for nu in (1, 2):
            for scale in (1.0, 1.5):
                mg2 = ctx.mg(e["dA"], omega=omega, nu=nu, coarse_scale=scale, **SETUP)
                ref = cycle_reference(levels, v, nu=nu, coarse_scale=scale)
                out = apply_host(ctx, mg2, v)
                disp = apply_host(ctx, mg2, v, through_dispatcher=True)
                dev = np.max(np.abs(out - ref)) / np.max(np.abs(ref))
                worst = max(worst, dev)
                print(f"{name}: omega {omega} nu {nu} scale {scale}: |dev - ref|_inf / |ref|_inf = {dev:.3e}")
                assert dev <= GATE
                assert same_bits(disp, out), "type 10 through bis_apply_preconditioner differs from bis_mg_apply"
                mg2.free()
        if omega != 0.0:
            mg.free()
    print(f"{name}: worst deviation {worst:.3e}")


@pytest.mark.parametrize("name", APPLY_CASES)
def test_aliasing_repeatability_symmetry_and_definiteness(ctx, built, name):
    e = built(name)
    n = e["A"].n_rows
    rng = np.random.default_rng(13)
    u, v = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    Mv = apply_host(ctx, e["mg"], v)
    assert same_bits(apply_host(ctx, e["mg"], v), Mv), "two applies differ"
    assert same_bits(apply_host(ctx, e["mg"], v, alias=True), Mv), "out aliasing in differs"
    assert same_bits(apply_host(ctx, e["mg"], v, alias=True, through_dispatcher=True), Mv)
    Mu = apply_host(ctx, e["mg"], u)
    a, b = u @ Mv, v @ Mu
    scale = np.linalg.norm(u) * np.linalg.norm(Mv)
    print(f"{name}: (u, M^-1 v) = {a:.15e}, (v, M^-1 u) = {b:.15e}, difference / (|u| |M^-1 v|) = {abs(a - b) / scale:.3e}")
    assert abs(a - b) <= 1e-12 * scale
    assert v @ Mv > 0 and u @ Mu > 0


CG_TOL = 1e-10


def device_cg(ctx, dA, b, pc=None, budget=400, **kw):
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


@pytest.mark.parametrize("name,make,kw", [("hpcg32", lambda c: c.gen_hpcg(32, 32, 32), dict(coarse_limit=64)),
                                          ("unstr888", lambda c: c.gen_unstr(8, 8, 8), dict(coarse_limit=64)),
                                          ("hpcg32_nu2_scale1.5", lambda c: c.gen_hpcg(32, 32, 32),
                                           dict(coarse_limit=64, nu=2, coarse_scale=1.5))],
                         ids=["hpcg32", "unstr888", "hpcg32_nu2_scale1.5"])
def test_cg_against_numpy_pcg_with_the_restated_cycle(ctx, name, make, kw):
    dA = make(ctx)
    A = host_crs(dA)
    mg = ctx.mg(dA, **kw)
    levels = downloaded(mg)
    assert levels[0]["kind"] == (2 if name.startswith("unstr") else 1) and len(levels) >= 2
    b = host_spmv(A, np.ones(A.n_rows))
    run = device_cg(ctx, dA, b, "mg", Ls=mg.operand)
    cyc = dict(nu=kw.get("nu", 1), coarse_scale=kw.get("coarse_scale", 1.0))
    ref_hist, _ = numpy_pcg(A, lambda r: cycle_reference(levels, r, **cyc), b, CG_TOL, 400)
    plain = device_cg(ctx, dA, b)
    r0 = ref_hist[0]
    dev = hist_dev(run["hist"], ref_hist)
    res = np.linalg.norm(b - host_spmv(A, run["x"]))
    print(f"{name}: rows {mg.rows}, device {run['iters']} iterations conv {run['conv']}, numpy {len(ref_hist) - 1}, "
          f"unpreconditioned {plain['iters']}, hist dev {dev:.3e}, true residual {res:.6e}, last entry {run['hist'][-1]:.6e}, r0 {r0:.6e}")
    assert run["conv"] and ref_hist[-1] < CG_TOL * r0
    assert run["iters"] == len(ref_hist) - 1
    assert dev <= HIST_TOL["cg"]
    assert res <= run["hist"][-1] + 1e-10 * r0
    if name.startswith("hpcg"):  # (b = A 1 is an eigenvector of the FEM-like operators: plain CG needs one iteration there)
        assert plain["conv"] and run["iters"] < plain["iters"]
    mg.free()
    dA.free()


def test_what_is_not_built_is_refused(ctx, built):
    from basic_iterative_solvers_amd import BisError
    e = built("fem666")
    dA, mg, n = e["dA"], e["mg"], e["A"].n_rows
    k = 2
    X, B, T = ctx.upload(np.zeros(n * k)), ctx.upload(np.ones(n * k)), ctx.upload(np.zeros(n * k))
    with pytest.raises(BisError, match="status 6"):
        ctx.mapply_preconditioner("mg", n, k, mg.operand, None, None, None, None, None, X, B, T, None)
    for solver in (ctx.mcg(dA, B, X, k), ctx.mbicgstab(dA, B, X, k), ctx.mgmres(dA, B, X, k)):
        with pytest.raises(BisError, match="status 6"):
            solver.set_preconditioner("mg", Ls=mg.operand)
        solver.free()
    x, b = ctx.upload(np.zeros(n)), ctx.upload(np.ones(n))
    cg = ctx.cg(dA, b, x)
    with pytest.raises(BisError, match="status 6"):
        cg.set_preconditioner("mg", Ls=mg.operand, outer=2)
    with pytest.raises(BisError, match="status 2"):
        cg.set_preconditioner("mg", Ls=dA)  # not the operand of a hierarchy
    cg.free()
    with pytest.raises(BisError, match="status 6"):
        ctx.apply_preconditioner("mg", n, mg.operand, None, None, None, None, None, x, b, None, None, outer=2)
    with pytest.raises(BisError, match="status 2"):
        ctx.apply_preconditioner("mg", n - 1, mg.operand, None, None, None, None, None, x, b, None, None)
    # every other entry point sees the zero matrix
    y = ctx.upload(np.full(n, 7.0))
    ctx.spmv(mg.operand, b, y)
    assert not y.to_host().any()
    for v in (X, B, T, x, b, y):
        v.free()
