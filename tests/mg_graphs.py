"""Adversarial inputs for the multigrid setup (bis_mg.hip, bis_spgemm.hip inside smoothed aggregation), numpy only: seeded
graphs from tests/reorder_ref.py made diagonally dominant, and the restated hierarchies of each, computed once per process.

test_mg_graphs_cpu.py shows on the restatement alone that every case is what CASES says it is; test_gpu_mg_graphs.py runs
them on the device.  Nothing here touches the GPU library.

Out of scope: the grid-stride wrap of the setup kernels past 16384 workgroups (mg_grid) needs more than 4 M rows, where the
Python MIS restatement is too slow."""
import functools
import time

import numpy as np

import reorder_ref as rr
from oracle.pyoracle import CRS


def rows_of(A):
    return np.repeat(np.arange(A.n_rows, dtype=np.int64), np.diff(A.row_ptr))


def dominant(A):
    """A with its pattern and off-diagonal values kept, a diagonal entry appended to every row that stores none, and the first
    diagonal entry of every row set to 1.2 sum |off-diagonal| + 1e-3: no zero diagonal on any level, well-conditioned cycles."""
    n = A.n_rows
    rows = rows_of(A)
    has = np.zeros(n, dtype=bool)
    has[rows[A.col == rows]] = True
    if not has.all():
        # the new entry goes behind the row's last one: a stable sort by row of (old entries, new diagonals)
        add = np.flatnonzero(~has)
        r_all = np.concatenate([rows, add])
        order = np.argsort(r_all, kind="stable")
        col = np.concatenate([A.col, add.astype(np.int32)])[order]
        val = np.concatenate([A.val, np.ones(len(add))])[order]
        rp = np.concatenate([[0], np.cumsum(np.bincount(r_all, minlength=n))])
        A = CRS(n, rp, col, val)
        rows = rows_of(A)
    val = A.val.copy()
    off = A.col != rows
    s = np.bincount(rows[off], weights=np.abs(val[off]), minlength=n)
    diag = np.flatnonzero(~off)
    first = diag[np.concatenate([[True], rows[diag][1:] != rows[diag][:-1]])]
    val[first] = 1.2 * s[rows[first]] + 1e-3
    return CRS(n, A.row_ptr, A.col, val)


def pairs_and_singles(p, s):
    """p disjoint 2 x 2 blocks on rows (0, 1), (2, 3), ..., then s rows that hold their diagonal only: whatever the order of
    the MIS keys, every block is one aggregate and every single row its own, p + s aggregates of 2 p + s rows."""
    rng = np.random.default_rng([9, p, s])
    k = 2 * np.arange(p, dtype=np.int64)
    col = np.concatenate([np.stack([k, k + 1, k, k + 1], axis=1).ravel(), 2 * p + np.arange(s, dtype=np.int64)])
    rp = np.concatenate([2 * np.arange(2 * p + 1), 4 * p + np.arange(1, s + 1)])
    edge = np.repeat(rng.uniform(-1.0, 1.0, p), 4)  # (a block's four entries; dominant() replaces the two on the diagonal)
    return dominant(CRS(2 * p + s, rp, col.astype(np.int32), np.concatenate([edge, np.ones(s)])))


def zero_edges(n):
    """dominant(banded_sym(n, 2, 40)) with a seeded tenth of its off-diagonal pairs set to a stored 0.0 on both sides."""
    A = dominant(rr.banded_sym(n, 2, 40))
    rows = rows_of(A)
    lower = np.flatnonzero(A.col < rows)
    rng = np.random.default_rng([10, n])
    pick = rng.choice(lower, len(lower) // 10, replace=False)
    key = rows * n + A.col  # (columns ascend and do not repeat: the keys ascend)
    mirror = np.searchsorted(key, A.col[pick].astype(np.int64) * n + rows[pick])
    assert np.array_equal(key[mirror], A.col[pick].astype(np.int64) * n + rows[pick])
    val = A.val.copy()
    val[pick] = 0.0
    val[mirror] = 0.0
    return CRS(n, A.row_ptr, A.col, val)


def shuffled_ties():
    """`shuffled` with its off-diagonal magnitudes rounded up to quarters (0.25 .. 1, signs kept): members find several root
    neighbours of equal |a_ij| in rows whose columns do not ascend, so "the lowest column among equals" is not "the first
    stored among equals"."""
    A = rr.symmetric_part(rr.ragged_lower(5000))
    off = A.col != rows_of(A)
    val = A.val.copy()
    val[off] = np.where(val[off] < 0, -1.0, 1.0) * np.ceil(np.abs(val[off]) * 4.0) / 4.0
    return dominant(CRS(A.n_rows, A.row_ptr, A.col, val))


def shuffled_with_duplicate():
    """`shuffled` with one lower entry of a row stored a second time at the row's end (its mirror once): what symmetric_part
    removes, put back.  Returns (matrix, row)."""
    A = CASES["shuffled"].A
    n = A.n_rows
    rows = rows_of(A)
    k = int(np.flatnonzero((A.col < rows) & (np.diff(A.row_ptr)[rows] > 4))[40])
    r = int(rows[k])
    at = int(A.row_ptr[r + 1])
    col, val = np.insert(A.col, at, A.col[k]), np.insert(A.val, at, 0.125)
    rp = A.row_ptr.copy()
    rp[r + 1:] += 1
    return CRS(n, rp, col, val), r


HUB_N, HUB_FAN = 2000, 1200


class Case:
    """A: the matrix; grid: its hint (nx, ny, nz, dof) or None; params: what bis_mg_create gets beside the defaults;
    smoothed: whether the smoothed hierarchy is built as well."""

    def __init__(self, make, grid=None, smoothed=True, **params):
        self._make, self.grid, self.smoothed, self.params = make, grid, smoothed, params

    @functools.cached_property
    def A(self):
        return self._make()


CASES = {
    "path5000": Case(lambda: dominant(rr.path(5000)), coarse_limit=30),
    "hub": Case(lambda: dominant(rr.hub(HUB_N, HUB_FAN)), coarse_limit=8),
    "hub5000": Case(lambda: dominant(rr.hub(5000, 3000)), smoothed=False, coarse_limit=30),
    "clique300": Case(lambda: dominant(rr.clique_at(2000, 224, 300)), coarse_limit=30),
    "components": Case(lambda: dominant(rr.with_tail(rr.grid2d(60), 3)), coarse_limit=30),
    "shuffled": Case(lambda: dominant(rr.symmetric_part(rr.ragged_lower(5000))), coarse_limit=30),
    "shuffled_ties": Case(shuffled_ties, coarse_limit=30),
    "zero_edges": Case(lambda: zero_edges(5000), coarse_limit=30),
    "wide30000": Case(lambda: dominant(rr.banded_sym(30000, 2, 40)), smoothed=False, coarse_limit=30),
    "boundary_keep": Case(lambda: pairs_and_singles(100, 300), coarse_limit=30),
    "boundary_drop": Case(lambda: pairs_and_singles(100, 301), coarse_limit=30),
    "chain16": Case(lambda: dominant(rr.path(1 << 16)), grid=(1 << 16, 1, 1, 1), smoothed=False, coarse_limit=1, max_levels=16),
    "chain16_exact": Case(lambda: dominant(rr.path(1 << 15)), grid=(1 << 15, 1, 1, 1), smoothed=False, coarse_limit=1, max_levels=16),
}
SMOOTHED = [name for name, c in CASES.items() if c.smoothed]

_REFERENCE = {}
SECONDS = {}


def reference(name, smoothed=False):
    """The restated hierarchy of a case (test_gpu_mg.hierarchy_reference / spgemm_ref.hierarchy), computed once and left
    alone; SECONDS records what it took."""
    key = (name, bool(smoothed))
    if key not in _REFERENCE:
        import spgemm_ref
        import test_gpu_mg as base
        c = CASES[name]
        assert c.smoothed or not smoothed, name
        t0 = time.perf_counter()
        _REFERENCE[key] = spgemm_ref.hierarchy(c.A, c.grid, **c.params) if smoothed else base.hierarchy_reference(c.A, c.grid, **c.params)
        SECONDS[key] = time.perf_counter() - t0
    return _REFERENCE[key]
