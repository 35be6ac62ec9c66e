"""A numpy restatement of bis_spgemm, bis_mat_transpose and of smoothed aggregation (bis_mg_create_smoothed: rho, omega_l,
P, R, A_c, the two transfers and the cycle), written from the definitions in include/bis_hip.h.

Where the header states an order of fp64 operations (the product's sums, P's values, both transfers) the restatement
performs these operations in that order: its results are the bits the device must give.  The SpMVs of the cycle are
test_gpu_mg.py's (products and row sums in np.longdouble, rounded once), so a cycle is compared at a tolerance.
No module state; nothing here touches the device."""
import numpy as np

import test_gpu_mg as base
from oracle.pyoracle import CRS

LD = np.longdouble
V, W, K, KGCR = 0, 1, 2, 3
run_sums, rows_of, host_spmv = base.run_sums, base.rows_of, base.host_spmv


def crs(n_rows, n_cols, row_ptr, col, val):
    return CRS(n_rows, np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int32), np.asarray(val, dtype=np.float64), n_cols=n_cols)


def crs_from_dense(M, keep=None):
    keep = (M != 0.0) if keep is None else keep
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))])
    r, c = np.nonzero(keep)
    return crs(M.shape[0], M.shape[1], rp, c, M[r, c])


def to_dense(A):
    """Entries that share a position are added in CRS order."""
    M = np.zeros((A.n_rows, A.n_cols))
    np.add.at(M, (rows_of(A), A.col), A.val)
    return M


def spgemm(A, B):
    """C = A B: products enumerated by position in A's row, then position in B's row; a stable sort by (row, column);
    every run summed left to right, the first product starting it."""
    assert A.n_cols == B.n_rows
    n, p = A.n_rows, B.n_cols
    len_b = np.diff(B.row_ptr)
    cnt = len_b[A.col] if A.nnz else np.zeros(0, dtype=np.int64)
    total = int(cnt.sum())
    if total == 0:
        return crs(n, p, np.zeros(n + 1), [], [])
    src = np.repeat(np.arange(A.nnz), cnt)                       # the entry of A of every product
    first = np.cumsum(cnt) - cnt
    t = np.arange(total) - np.repeat(first, cnt) + np.repeat(B.row_ptr[:-1][A.col], cnt)  # ... and the entry of B
    rows = rows_of(A)[src]
    prod = A.val[src] * B.val[t]
    key = (rows.astype(np.int64) << 32) | B.col[t].astype(np.int64)
    order = np.argsort(key, kind="stable")
    ks, vs = key[order], prod[order]
    start = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    end = np.concatenate([start[1:], [len(ks)]])
    val = run_sums(vs, start, end)
    r_c = ks[start] >> 32
    return crs(n, p, np.searchsorted(r_c, np.arange(n + 1)), ks[start] & 0xffffffff, val)


def transpose(A):
    """Row c lists column c of A by ascending row, repeats inside a row of A in that row's order."""
    order = np.argsort(A.col, kind="stable")
    return crs(A.n_cols, A.n_rows, np.searchsorted(A.col[order], np.arange(A.n_cols + 1)), rows_of(A)[order], A.val[order])


# ---- smoothed aggregation --------------------------------------------------------------------------------------------

def first_diagonal(A):
    rows = rows_of(A)
    d = np.zeros(A.n_rows)
    for k in np.flatnonzero(A.col == rows)[::-1]:  # (the first diagonal entry of a row wins)
        d[rows[k]] = A.val[k]
    return d


def abs_row_sums(A):
    """s_i = sum_j |a_ij| left to right from 0."""
    a = np.abs(A.val)
    s = np.zeros(A.n_rows)
    start, length = A.row_ptr[:-1], np.diff(A.row_ptr)
    for j in range(int(length.max())):
        m = length > j
        s[m] = s[m] + a[start[m] + j]
    return s


def smoothed_transition(A, agg, nc, prolong_omega, product=None):
    """(omega_l, P, R, A_c) of a level.  `product` replaces spgemm for the two Galerkin products where only iteration counts
    matter (the CPU test passes a scipy product)."""
    product = product or spgemm
    n = A.n_rows
    d = first_diagonal(A)
    rho = np.max(abs_row_sums(A) / np.abs(d))
    omega_l = np.float64(prolong_omega) / rho
    T = crs(n, nc, np.arange(n + 1), agg, np.ones(n))
    Q = spgemm(A, T)
    c = omega_l / d
    rq = rows_of(Q)
    t = (Q.col == agg[rq]).astype(np.float64)
    cq = c[rq] * Q.val
    P = crs(n, nc, Q.row_ptr, Q.col, t - cq)
    R = transpose(P)
    return omega_l, P, R, product(R, product(A, P))


def hierarchy(A, grid, prolong_omega=0.0, product=None, **kw):
    """The levels of bis_mg_create_smoothed: test_gpu_mg.hierarchy_reference's dicts plus P, R, omega_l (None on the coarsest)."""
    p = dict(base.DEFAULTS, **kw)
    po = 4.0 / 3.0 if prolong_omega == 0.0 else prolong_omega
    levels = []
    while True:
        n = A.n_rows
        L = dict(A=A, grid=grid, w=base.weights_reference(A, p["omega"]), agg=None, kind=0, P=None, R=None, omega_l=None)
        levels.append(L)
        if n <= p["coarse_limit"] or len(levels) >= p["max_levels"]:
            break
        use_grid = p["coarsening"] != 2 and grid is not None and int(np.prod(grid)) == n
        if use_grid:
            agg, cgrid = base.grid_aggregates(n, grid)
            nc = int(np.prod(cgrid))
        else:
            agg, L["root"] = base.mis_aggregates(A)
            cgrid, nc = None, int(agg.max()) + 1
        if 5 * nc > 4 * n:
            break
        L["agg"], L["kind"] = agg, 1 if use_grid else 2
        L["omega_l"], L["P"], L["R"], A = smoothed_transition(A, agg, nc, po, product)
        grid = cgrid
    return levels


def restrict(R, d):
    """r_c[I] = sum over row I of R of R_t d[col t]: lane q of 64 sums the positions q, q + 64, ... from 0; then lane q + 32
    is added to lane q, then + 16, ..., + 1."""
    prod = R.val * d[R.col]
    start, length = R.row_ptr[:-1], np.diff(R.row_ptr)
    S = np.zeros((R.n_rows, 64))
    lane = np.arange(64)
    for j in range((int(length.max()) + 63) // 64 if len(length) else 0):
        pos = j * 64 + lane[None, :]
        m = pos < length[:, None]
        idx = np.where(m, start[:, None] + pos, 0)
        S = np.where(m, S + prod[idx], S)
    for off in (32, 16, 8, 4, 2, 1):
        S[:, :off] = S[:, :off] + S[:, off:2 * off]
    return S[:, 0].copy()


def prolong(P, x, ec, scale):
    """x_i + scale (sum over row i of P of P_t e_c[col t], left to right, the first product starting it)."""
    prod = P.val * ec[P.col]
    start, end = P.row_ptr[:-1], P.row_ptr[1:]
    has = end > start
    s = run_sums(prod, start[has], end[has])
    out = x.copy()
    out[has] = x[has] + scale * s
    return out


def ldot(a, b):
    return np.float64(np.dot(a.astype(LD), b.astype(LD)))


def config(cycle=V, cycle_levels=0, nu=1, coarse_scale=1.0, coarse_sweeps=4):
    return dict(cycle=cycle, cycle_levels=cycle_levels, nu=nu, coarse_scale=coarse_scale, coarse_sweeps=coarse_sweeps)


def coarse_solve(levels, rc, l, cfg):
    """e_c of transition l: the header's V, W and K steps (bis_mg_set_cycle), unchanged by smoothing."""
    N = l + 1
    A = levels[N]["A"]
    kind = cfg["cycle"] if (l < len(levels) - 2 and (cfg["cycle_levels"] == 0 or l < cfg["cycle_levels"])) else V
    c = cycle(levels, rc, cfg, N)
    if kind == V:
        return c
    if kind == W:
        return c + cycle(levels, rc - host_spmv(A, c), cfg, N)
    with np.errstate(all="ignore"):
        v = host_spmv(A, c)
        t = c if kind == K else v
        rho1, alpha1 = ldot(t, v), ldot(t, rc)
        if rho1 == 0.0 or not np.isfinite(rho1):
            return np.zeros_like(rc)
        s1 = alpha1 / rho1
        rt = rc - s1 * v
        d = cycle(levels, rt, cfg, N)
        w = host_spmv(A, d)
        t2 = d if kind == K else w
        gamma, beta, alpha2 = ldot(t2, v), ldot(t2, w), ldot(t2, rt)
        rho2 = beta - (gamma * gamma) / rho1
        if not rho2 > 0.0:
            c1, c2 = s1, np.float64(0.0)
        else:
            c2 = alpha2 / rho2
            c1 = s1 - (gamma * c2) / rho1
        return (c1 * c) + (c2 * d)


def cycle(levels, b, cfg=None, l=0):
    """One cycle of a smoothed hierarchy (levels with P and R) for the right-hand side b."""
    cfg = cfg or config()
    L = levels[l]
    A, w = L["A"], L["w"]

    def sweep(x):
        return x + w * (b - host_spmv(A, x))

    x = w * b
    if l + 1 == len(levels):
        for _ in range(cfg["coarse_sweeps"] - 1):
            x = sweep(x)
        return x
    for _ in range(cfg["nu"] - 1):
        x = sweep(x)
    rc = restrict(L["R"], b - host_spmv(A, x))
    ec = coarse_solve(levels, rc, l, cfg)
    x = prolong(L["P"], x, ec, cfg["coarse_scale"])
    for _ in range(cfg["nu"]):
        x = sweep(x)
    return x
