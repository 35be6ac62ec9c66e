"""GPU: which form a triangular sweep takes (bis_sptrsv.hip, the table in its header) -- input x options -> the kernel
sweep_kernel() names, both directions, every result against the oracle's natural-order sweep (kernels.hpp:54-117).  The
routes the other files leave open: options flipped on a live triangle between two sweeps, what a value change drops, and
the chained-first order falling back to the tiled sweep."""
import numpy as np
import pytest

from helpers import OptionScope, permute_crs
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

TILED = "trsv_tiled_kernel"
CHAINED = "trsv_chain_kernel"
WAVE = "sptrsv_wave_kernel"
LANE = "sptrsv_syncfree_kernel"
VIEWS = "spmv_rowblock_kernel (triangular epilogue, a launch per independent row block)"
PER_LEVEL = "trsv_level_kernel (a launch per level)"
LEVEL_SCHEDULED = (WAVE, LANE)
NO_TILES_NO_CHAINS = dict(trsv_tiled=0, trsv_chain=0)


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    yield c
    c.close()


def _mirror(L):
    """Row n-1-r, columns n-1-c: strictly upper, the backward sweep walks it in the dependency order of the forward one."""
    n, rp = L.n_rows, L.row_ptr
    rpu = np.concatenate([[0], np.cumsum(np.diff(rp)[::-1])]).astype(np.int64)
    idx = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in range(n - 1, -1, -1)])
    return CRS(n, rpu, (n - 1 - L.col[idx]).astype(np.int32), L.val[idx])


def _band():
    """The 20000-row band of width 6 of test_gpu_records.py, and its mirror image; no grid."""
    nb, w = 20000, 6
    lens = np.minimum(np.arange(nb), w)
    rp = np.concatenate([[0], np.cumsum(lens)])
    col = np.concatenate([np.arange(r - lens[r], r) for r in range(nb)]).astype(np.int32)
    val = np.random.default_rng(4).uniform(-1, 1, rp[-1]) / w
    L = CRS(nb, rp, col, val)
    return L, _mirror(L), np.full(nb, 2.0)


def _two_dof_grid(nx, ny, nz):
    """The neighbour stencil of test_tiled_sweep_grid_and_backoff_options_bit_exact at dof = 2 (every lower neighbour
    within distance 1, both unknowns of it), without the entries whose column is row - 1 in another node: the only rows
    that follow their predecessor are the second unknowns of a node, so every chain is 2 rows long."""
    dof = 2
    cand = [(ddx, ddy, ddz, dd) for ddz in (-1, 0, 1) for ddy in (-1, 0, 1) for ddx in (-1, 0, 1) for dd in range(-(dof - 1), dof)
            if (ddz, ddy, ddx, dd) < (0, 0, 0, 0)]
    n = nx * ny * nz * dof
    rows = [[] for _ in range(n)]
    for z in range(nz):
        for y in range(ny):
            for xx in range(nx):
                for d in range(dof):
                    r = ((z * ny + y) * nx + xx) * dof + d
                    for ddx, ddy, ddz, dd in cand:
                        X, Y, Z, Dd = xx + ddx, y + ddy, z + ddz, d + dd
                        if 0 <= X < nx and 0 <= Y < ny and 0 <= Z < nz and 0 <= Dd < dof:
                            c = ((Z * ny + Y) * nx + X) * dof + Dd
                            if c != r - 1 or (X, Y, Z) == (xx, y, z):
                                rows[r].append(c)
                    rows[r].sort()
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])])
    col = np.array([c for cs in rows for c in cs], dtype=np.int32)
    L = CRS(n, rp, col, np.random.default_rng(nx + ny + nz).uniform(-0.3, 0.3, len(col)))
    Ut = L.to_scipy().T.tocsr()
    Ut.sort_indices()
    return L, CRS(n, Ut.indptr, Ut.indices.astype(np.int32), Ut.data), np.random.default_rng(7).uniform(1, 2, n)


class _Case:
    """One input: the host triangles, D and b, the oracle's two sweeps (computed once), and make() -> device triangles
    built under the options in effect at the call."""

    def __init__(self, ctx, oracle, kind):
        self.ctx, self.kind = ctx, kind
        self.dA = None
        if kind == "band":
            self.L, self.U, self.D = _band()
        elif kind == "two_dof_grid":
            self.grid = (21, 20, 20)  # 16800 rows
            self.L, self.U, self.D = _two_dof_grid(*self.grid)
        else:
            if kind == "hpcg12":
                A, self.dA = oracle.gen_hpcg(12), ctx.gen_hpcg(12)
            elif kind == "hpcg8_colour":
                dA = ctx.gen_hpcg(8)
                self.dA, perm, _ = ctx.multicolour(dA)
                dA.free()
                A = permute_crs(oracle.gen_hpcg(8), perm)
            else:
                A, self.dA = oracle.gen_unstr(10, 10, 11), ctx.gen_unstr(10, 10, 11)
            Lf, self.L, Uf, self.U = oracle.split_LU(A)
            self.D = oracle.peel_diag(Lf)[0]
        self.n = self.L.n_rows
        self.b = np.random.default_rng(11).uniform(-1, 1, self.n)
        self.want = (oracle.sptrsv(self.L, self.D, self.b), oracle.sptrsv(self.U, self.D, self.b, backward=True))
        self.db, self.x = ctx.upload(self.b), ctx.alloc(self.n)

    def make(self):
        if self.dA is not None:
            dL, dU, dD, dDinv = self.ctx.split_strict(self.dA)
            dDinv.free()
            return dL, dU, dD
        dL, dU = self.ctx.matrix(self.L), self.ctx.matrix(self.U)
        if self.kind == "two_dof_grid":
            dL.set_grid_hint(*self.grid, 2); dU.set_grid_hint(*self.grid, 2)
        return dL, dU, self.ctx.upload(self.D)

    def sweep_and_check(self, dL, dU, dD, names, what):
        """One forward and one backward sweep into a NaN-filled x: the names asked for, and the oracle's bits (the two
        per-level forms sum products, not the reference's fma chain: 1e-12 max|x| as in test_level_and_syncfree_sweep_options)."""
        ctx, x = self.ctx, self.x
        for T, solve, backward, allowed, want in ((dL, ctx.sptrsv, False, names[0], self.want[0]), (dU, ctx.bsptrsv, True, names[1], self.want[1])):
            ctx.init_vector(x, np.nan)
            solve(T, x, dD, self.db)
            got, k = x.to_host(), T.sweep_kernel(backward)
            print(self.kind, what, "backward" if backward else "forward", "->", k)
            assert k in allowed, (self.kind, what, backward, k)
            if k in (VIEWS, PER_LEVEL):
                err = np.max(np.abs(got - want)) / np.max(np.abs(want))
                print("   max |dx| / max |x| =", err)
                assert err <= 1e-12, (self.kind, what, backward, k, err)
            else:
                assert np.array_equal(got, want), (self.kind, what, backward, k)


@pytest.fixture(scope="module")
def case(ctx, oracle):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = _Case(ctx, oracle, kind)
        return made[kind]
    return get


def _both(*names):
    return (names, names)


_TABLE = [  # (input, options, kernel names allowed forward / backward)
    ("hpcg12", {}, _both(TILED)),
    ("hpcg12", NO_TILES_NO_CHAINS, _both(*LEVEL_SCHEDULED)),
    ("hpcg12", dict(NO_TILES_NO_CHAINS, trsv_wave=0), _both(LANE)),
    ("hpcg12", dict(NO_TILES_NO_CHAINS, trsv_wave=1), _both(WAVE)),
    ("hpcg12", dict(NO_TILES_NO_CHAINS, trsv_one_xcd=1), _both(LANE)),
    ("band", {}, _both(CHAINED)),
    ("band", dict(trsv_chain=0), _both(*LEVEL_SCHEDULED)),
    ("hpcg8_colour", {}, _both(VIEWS)),
    # (the host analysis has no block search; every level of this input is still one ascending row range, in both directions)
    ("hpcg8_colour", dict(trsv_host_analysis=1), _both(VIEWS)),
    ("unstr", {}, _both(WAVE)),
]


@pytest.mark.parametrize("kind,opts,names", _TABLE, ids=[f"{k}-{'-'.join(f'{a}={b}' for a, b in o.items()) or 'default'}" for k, o, _ in _TABLE])
def test_sweep_form_table(ctx, case, kind, opts, names):
    """Input x options -> kernel name, forward and backward, swept twice (the first call builds, the second reuses what
    it built): the name and the oracle's result after each."""
    c = case(kind)
    with OptionScope(ctx, **opts):
        dL, dU, dD = c.make()
        try:
            for rep in ("build", "reuse"):
                c.sweep_and_check(dL, dU, dD, names, (opts, rep))
        finally:
            dL.free(); dU.free(); dD.free()


@pytest.mark.parametrize("kind,first,other", [("hpcg12", TILED, NO_TILES_NO_CHAINS), ("band", CHAINED, dict(trsv_chain=0))])
def test_sweep_options_are_read_per_call(ctx, case, kind, first, other):
    """The form is decided at every sweep call from the options in effect then: the same handles take the tiled (chained)
    sweep, a level-scheduled kernel while it is switched off, and the plan they already have once it is back on."""
    c = case(kind)
    dL, dU, dD = c.make()
    try:
        c.sweep_and_check(dL, dU, dD, _both(first), "default")
        with OptionScope(ctx, **other):
            c.sweep_and_check(dL, dU, dD, _both(*LEVEL_SCHEDULED), other)
        c.sweep_and_check(dL, dU, dD, _both(first), "default again")
    finally:
        dL.free(); dU.free(); dD.free()


@pytest.mark.parametrize("kind,name,line,lines_per_direction", [("band", CHAINED, "chained sptrsv plan", 1), ("hpcg12", TILED, "tiled sptrsv plan", 2)])
def test_what_a_value_change_drops(ctx, case, capfd, monkeypatch, kind, name, line, lines_per_direction):
    """bis_mat_retune between two sweeps: the chained plan depends on the pattern only and is kept (its plan line appears
    once per direction), the tiled plan holds a copy of the values and is built again (twice per direction)."""
    monkeypatch.setenv("BIS_TRSV_CHAIN_STATS", "1")
    monkeypatch.setenv("BIS_TRSV_TILE_STATS", "1")
    c = case(kind)
    dL, dU, dD = c.make()
    try:
        capfd.readouterr()
        c.sweep_and_check(dL, dU, dD, _both(name), "before retune")
        dL.retune(); dU.retune()
        c.sweep_and_check(dL, dU, dD, _both(name), "after retune")
        ctx.sync()
        err = capfd.readouterr().err
        print(err)
        assert err.count(line) == 2 * lines_per_direction, err
    finally:
        dL.free(); dU.free(); dD.free()


def test_chained_first_falls_back_to_the_tiled_sweep(ctx, case, capfd, monkeypatch):
    """A grid-hinted pair with several unknowns per node and at least 16384 rows has the chained sweep tried first; where
    its plan does not apply the tiled sweep serves the triangle after all.  Input: 21 x 20 x 20 nodes, dof = 2 (16800
    rows), _two_dof_grid: chains of 2 rows, below the chained plan's average of 3.  Default options: one "too short, not
    used" chained plan line per direction, then one tiled plan line per direction, both sweeps tiled, bit-exact, twice."""
    monkeypatch.setenv("BIS_TRSV_CHAIN_STATS", "1")
    monkeypatch.setenv("BIS_TRSV_TILE_STATS", "1")
    c = case("two_dof_grid")
    dL, dU, dD = c.make()
    try:
        capfd.readouterr()
        for rep in ("build", "reuse"):
            c.sweep_and_check(dL, dU, dD, _both(TILED), rep)
        ctx.sync()
        err = capfd.readouterr().err
        print(err)
        lines = [l for l in err.splitlines() if l.startswith(("chained sptrsv plan", "tiled sptrsv plan"))]
        assert len(lines) == 4, err
        for direction in ("forward", "backward"):
            mine = [l for l in lines if f"plan ({direction})" in l]
            assert len(mine) == 2 and mine[0].startswith("chained sptrsv plan") and mine[0].endswith("too short, not used") and \
                mine[1].startswith("tiled sptrsv plan"), err
    finally:
        dL.free(); dU.free(); dD.free()
