"""ILU(k) with level-of-fill restated in numpy / pure Python, from the definitions in include/bis_hip.h (bis_mat_iluk):

* symbolic_sum_rule: the textbook row-wise symbolic factorisation, lev(i,j) = min over pivots p < min(i,j) of
  lev(i,p) + lev(p,j) + 1, entries above the level dropped as they arise;
* symbolic_two_search: the fill-path form the device runs -- one breadth-first search per row on A (upper part) and one on
  A^T (lower part, transposed), each continuing only through vertices below its start, to depth k + 1;
* padded: A with +0.0 at the fill positions, columns ascending;
* numeric: the IKJ elimination on a given pattern in the device's order (ascending pivots, the |u_kk| < 1e-16 skip, an
  update on EVERY shared position, pivot replacement); with exact=True every update is one correctly rounded fma;
* fma: float(Fraction(a) * Fraction(b) + Fraction(c)), exact for finite arguments (no math.fma before Python 3.13).

Matrices are oracle.pyoracle.CRS objects."""
from fractions import Fraction

import numpy as np

from oracle.pyoracle import CRS


def fma(a, b, c):
    """a * b + c with one rounding (finite arguments; an exact zero comes out as +0.0)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _rows(A):
    rp = np.asarray(A.row_ptr, dtype=np.int64)
    col = np.asarray(A.col, dtype=np.int64)
    return [col[rp[i]:rp[i + 1]] for i in range(A.n_rows)]


def _transposed_rows(A):
    rows = _rows(A)
    out = [[] for _ in range(A.n_rows)]
    for i, r in enumerate(rows):
        for j in r:
            out[int(j)].append(i)
    return [np.asarray(r, dtype=np.int64) for r in out]


def symbolic_sum_rule(A, k):
    """Per row a dict {column: level} of the positions with level <= k, by the sum rule."""
    lev = []
    for i, r in enumerate(_rows(A)):
        row = {int(j): 0 for j in r}
        done = set()
        while True:  # pivots in ascending order, those created on the way included
            cand = [p for p in row if p < i and p not in done]
            if not cand:
                break
            p = min(cand)
            done.add(p)
            for j, l_pj in lev[p].items():
                if j <= p:
                    continue
                new = row[p] + l_pj + 1
                if new <= k and new < row.get(j, k + 1):
                    row[j] = new
        lev.append(row)
    return lev


def _search(adj, i, k):
    """{t: level} for the t > i that a breadth-first search from i reaches within k + 1 edges through vertices < i."""
    seen = {i}
    frontier = [i]
    out = {}
    for depth in range(1, k + 2):
        nxt = []
        for v in frontier:
            for t in adj[v]:
                t = int(t)
                if t in seen:
                    continue
                seen.add(t)
                if t > i:
                    out[t] = depth - 1
                else:
                    nxt.append(t)
        frontier = nxt
    return out


def symbolic_two_search(A, k):
    """The same levels by the two searches.  The diagonal is level 0 where A stores it."""
    n = A.n_rows
    rows, trows = _rows(A), _transposed_rows(A)
    lev = [dict() for _ in range(n)]
    for i in range(n):
        if i in set(int(c) for c in rows[i]):
            lev[i][i] = 0
        for t, l in _search(rows, i, k).items():
            lev[i][t] = l
        for t, l in _search(trows, i, k).items():  # column i of the lower part
            lev[t][i] = l
    return lev


def padded(A, lev):
    """(P, n_fill): the pattern of `lev` with A's values at A's positions and +0.0 elsewhere, columns ascending."""
    n = A.n_rows
    rp = np.asarray(A.row_ptr, dtype=np.int64)
    cols, vals = [], []
    for i in range(n):
        have = {int(c): float(v) for c, v in zip(A.col[rp[i]:rp[i + 1]], A.val[rp[i]:rp[i + 1]])}
        c = np.array(sorted(lev[i]), dtype=np.int32)
        cols.append(c)
        vals.append(np.array([have.get(int(j), 0.0) for j in c], dtype=np.float64))
    prp = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    P = CRS(n, prp, np.concatenate(cols).astype(np.int32) if n else np.zeros(0, np.int32),
            np.concatenate(vals) if n else np.zeros(0))
    return P, int(prp[-1] - rp[-1])


def numeric(P, pivot_tol=1e-8, pivot_repl=1e-4, exact=False):
    """(Ls, L_D, Us, U_D) of the elimination on P's pattern (rows sorted, diagonal stored, no repeated column)."""
    n = P.n_rows
    rp = np.asarray(P.row_ptr, dtype=np.int64)
    col = np.asarray(P.col, dtype=np.int64)
    w = np.array(P.val, dtype=np.float64)
    U_D = np.zeros(n)
    where = np.full(n, -1, dtype=np.int64)  # position of a column in the current row
    ustart = np.zeros(n, dtype=np.int64)
    for i in range(n):
        s, e = rp[i], rp[i + 1]
        c = col[s:e]
        assert np.all(np.diff(c) > 0)
        where[c] = np.arange(s, e)
        ustart[i] = s + np.searchsorted(c, i, side="right")
        for p in range(s, e):
            k = int(col[p])
            if k >= i:
                break
            pivot = U_D[k]
            if abs(pivot) < 1e-16:
                continue
            factor = w[p] / pivot
            w[p] = factor
            q = np.arange(ustart[k], rp[k + 1])
            at = where[col[q]]
            q, at = q[at >= 0], at[at >= 0]
            if exact:
                for a, b in zip(at, q):
                    w[a] = fma(-factor, w[b], w[a])
            else:
                w[at] = w[at] - factor * w[q]
        d = where[i]
        assert d >= 0
        u = w[d]
        if abs(u) < pivot_tol:
            u = (1.0 if u >= 0 else -1.0) * pivot_repl
        w[d] = u
        U_D[i] = u
        where[c] = -1
    rows = np.repeat(np.arange(n), np.diff(rp))
    lo, up = col < rows, col > rows

    def part(m):
        prp = np.concatenate([[0], np.cumsum(np.bincount(rows[m], minlength=n))]).astype(np.int64)
        return CRS(n, prp, col[m].astype(np.int32), w[m])
    return part(lo), np.ones(n), part(up), U_D


def iluk(A, k, pivot_tol=1e-8, pivot_repl=1e-4, exact=False):
    """(Ls, L_D, Us, U_D, P, n_fill) of ILU(k), k >= 1 (k = 0 with fill semantics: every position of A's pattern updates)."""
    P, n_fill = padded(A, symbolic_two_search(A, k))
    return numeric(P, pivot_tol, pivot_repl, exact) + (P, n_fill)


def random_pattern(n, density, symmetric, seed):
    """A seeded n x n matrix with a full diagonal; structurally symmetric or not."""
    rng = np.random.default_rng(seed)
    M = rng.random((n, n)) < density
    if symmetric:
        M = M | M.T
    np.fill_diagonal(M, True)
    rows, cols = np.nonzero(M)
    val = rng.uniform(-1, 1, rows.size)
    val[rows == cols] = 4.0 + n * density
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return CRS(n, rp, cols.astype(np.int32), val)
