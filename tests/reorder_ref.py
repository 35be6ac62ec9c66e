"""Plain sequential references for the reordering layer (bis_reorder.hip, bis_order.hip) and seeded graph builders for its
tests.  The references are the definitions the device code reproduces, written on Python lists so that they stay usable at
5e5 rows; numpy only builds the arrays.  Nothing here touches the GPU library or the oracle.

test_reorder_ref_cpu.py shows by independent means that the references are right and pins the colour and component counts
the GPU cases rely on."""
import numpy as np

from oracle.pyoracle import CRS


# ---- references --------------------------------------------------------------------------------------------------------

def greedy_colours(A):
    """Greedy first-fit in natural row order: row r takes the smallest colour not held by its stored columns c < r
    (entries at or above the diagonal do not constrain r).  int32 array."""
    rp, col = A.row_ptr.tolist(), A.col.tolist()
    colour = [0] * A.n_rows
    for r in range(A.n_rows):
        used = 0
        for k in range(rp[r], rp[r + 1]):
            c = col[k]
            if c < r:
                used |= 1 << colour[c]
        colour[r] = ((used + 1) & ~used).bit_length() - 1  # lowest clear bit
    return np.array(colour, dtype=np.int32)


def colour_perm(colour):
    """perm[new] = old of the stable counting sort of the rows by colour."""
    return np.argsort(colour, kind="stable").astype(np.int32)


def adjacency(A):
    """Sorted neighbour lists of the undirected graph of A (the diagonal and repeated entries dropped)."""
    n = A.n_rows
    rp, col = A.row_ptr.tolist(), A.col.tolist()
    adj = [set() for _ in range(n)]
    for r in range(n):
        for k in range(rp[r], rp[r + 1]):
            c = col[k]
            if c != r:
                adj[r].add(c)
                adj[c].add(r)
    return [sorted(a) for a in adj]


def queue_order(A, rcm):
    """The sequential definition of the two orderings (host/utilities/permute.hpp bfs_like_permutation): components start
    at the lowest unseen vertex (BFS) or the unseen vertex of smallest (degree, index) (RCM); a popped vertex appends its
    unseen neighbours by ascending index (BFS) or ascending (degree, index) (RCM); RCM reverses the result."""
    n = A.n_rows
    adj = adjacency(A)
    deg = [len(a) for a in adj]
    starts = sorted(range(n), key=deg.__getitem__) if rcm else range(n)
    seen, perm = [False] * n, []
    for s0 in starts:
        if seen[s0]:
            continue
        seen[s0] = True
        head = len(perm)
        perm.append(s0)
        while head < len(perm):
            v = perm[head]
            head += 1
            nb = [w for w in adj[v] if not seen[w]]
            for w in nb:
                seen[w] = True
            if rcm:
                nb.sort(key=deg.__getitem__)
            perm += nb
    return np.array(perm[::-1] if rcm else perm, dtype=np.int32)


def n_components(A):
    """Connected components of the undirected graph of A."""
    adj = adjacency(A)
    seen = [False] * A.n_rows
    count = 0
    for s0 in range(A.n_rows):
        if seen[s0]:
            continue
        count += 1
        seen[s0] = True
        stack = [s0]
        while stack:
            v = stack.pop()
            for w in adj[v]:
                if not seen[w]:
                    seen[w] = True
                    stack.append(w)
    return count


def scale_ref(A, init):
    """-scale (extract_scale + scale_mat): s = init, s[r] = 1/sqrt(|a_rr|) from the LAST stored diagonal entry of row r
    (rows without one keep init), then val[k] *= (s[r] * s[col[k]]) -- the product of the two scales first, as the kernel
    associates it.  Returns (s, scaled values, lowest row holding a stored diagonal entry with |a_rr| < 1e-16, or -1)."""
    n = A.n_rows
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.row_ptr))
    s = np.full(n, float(init))
    bad = -1
    for k in np.flatnonzero(A.col == rows).tolist():  # ascending k: a later diagonal entry of a row overwrites an earlier one
        r, v = int(rows[k]), abs(float(A.val[k]))
        if v < 1e-16 and bad < 0:
            bad = r
        with np.errstate(divide="ignore"):
            s[r] = np.float64(1.0) / np.sqrt(np.float64(v))
    with np.errstate(all="ignore"):
        val = A.val * (s[rows] * s[A.col])
    return s, val, bad


# ---- builders ----------------------------------------------------------------------------------------------------------

def _from_pairs(n, r, c, rng):
    """CRS of the distinct (r, c) pairs, columns ascending; off-diagonal values in [-1, 1], diagonal values in [1, 2]."""
    key = np.unique(np.asarray(r, dtype=np.int64) * n + np.asarray(c, dtype=np.int64))
    rr, cc = key // n, key % n
    rp = np.concatenate([[0], np.cumsum(np.bincount(rr, minlength=n))])
    val = rng.uniform(-1.0, 1.0, len(key))
    val[rr == cc] = rng.uniform(1.0, 2.0, int(np.count_nonzero(rr == cc)))
    return CRS(n, rp, cc.astype(np.int32), val)


def _rows_of(A):
    rp, col, val = A.row_ptr.tolist(), A.col.tolist(), A.val.tolist()
    return ([col[rp[r]:rp[r + 1]] for r in range(A.n_rows)], [val[rp[r]:rp[r + 1]] for r in range(A.n_rows)])


def _from_rows(rows, vals):
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int64)
    col = np.array([c for cs in rows for c in cs], dtype=np.int32)
    val = np.array([v for vs in vals for v in vs], dtype=np.float64)
    return CRS(len(rows), rp, col, val)


def path(n, seed=1):
    """Tridiagonal matrix: the path graph 0 - 1 - ... - n-1 with a full diagonal."""
    rng = np.random.default_rng([seed, 1])
    i = np.arange(n, dtype=np.int64)
    return _from_pairs(n, np.concatenate([i, i[1:], i[:-1]]), np.concatenate([i, i[:-1], i[1:]]), rng)


def banded_sym(n, k, band, seed=1):
    """Symmetric pattern, full diagonal, random values: every row draws k partners in [r - band, r + band] (those outside
    the matrix are dropped), and every edge is stored on both sides.  Columns ascending."""
    rng = np.random.default_rng([seed, 2, n])
    r = np.repeat(np.arange(n, dtype=np.int64), k)
    off = rng.integers(1, band + 1, n * k) * rng.choice([-1, 1], n * k)
    c = r + off
    ok = (c >= 0) & (c < n)
    r, c = r[ok], c[ok]
    i = np.arange(n, dtype=np.int64)
    return _from_pairs(n, np.concatenate([i, r, c]), np.concatenate([i, c, r]), rng)


def grid2d(nx, seed=1):
    """5-point stencil on an nx x nx grid, row = y * nx + x, columns ascending."""
    rng = np.random.default_rng([seed, 3])
    n = nx * nx
    i = np.arange(n, dtype=np.int64)
    right = i[(i % nx) < nx - 1]
    down = i[i < n - nx]
    r = np.concatenate([i, right, right + 1, down, down + nx])
    c = np.concatenate([i, right + 1, right, down + nx, down])
    return _from_pairs(n, r, c, rng)


def _append(A, B):
    """blockdiag(A, B)."""
    return CRS(A.n_rows + B.n_rows, np.concatenate([A.row_ptr, A.row_ptr[-1] + B.row_ptr[1:]]),
               np.concatenate([A.col, B.col + A.n_rows]), np.concatenate([A.val, B.val]))


def with_tail(A, m):
    """A with an m-vertex path appended as a component of its own."""
    return _append(A, path(m, seed=7))


def with_isolated(A, m):
    """A with m isolated vertices appended: alternately a diagonal-only row and an empty row."""
    lens = (np.arange(m) % 2 == 0).astype(np.int64)
    iso = CRS(m, np.concatenate([[0], np.cumsum(lens)]), np.flatnonzero(lens).astype(np.int32), np.full(int(lens.sum()), 3.0))
    return _append(A, iso)


def hub(n, fan, seed=1):
    """Vertex 0 joined to `fan` others; every vertex also draws two partners anywhere (stored on both sides), which leaves
    many vertices of equal degree.  Full diagonal, columns ascending."""
    rng = np.random.default_rng([seed, 4, n])
    spokes = rng.choice(np.arange(1, n, dtype=np.int64), fan, replace=False)
    r = np.repeat(np.arange(n, dtype=np.int64), 2)
    c = rng.integers(0, n, 2 * n)
    i = np.arange(n, dtype=np.int64)
    z = np.zeros(fan, dtype=np.int64)
    return _from_pairs(n, np.concatenate([i, r, c, z, spokes]), np.concatenate([i, c, r, spokes, z]), rng)


def clique_at(n, first_row, m, seed=1):
    """An m-clique on rows first_row .. first_row + m - 1 inside a tridiagonal matrix.  Greedy first-fit gives clique row
    first_row + j the colour j (for first_row even), so the matrix needs exactly max(m, 2) colours."""
    rng = np.random.default_rng([seed, 5])
    i = np.arange(n, dtype=np.int64)
    q = np.arange(first_row, first_row + m, dtype=np.int64)
    qr, qc = np.repeat(q, m), np.tile(q, m)
    return _from_pairs(n, np.concatenate([i, i[1:], i[:-1], qr]), np.concatenate([i, i[:-1], i[1:], qc]), rng)


RAGGED_COUNTS = (0, 1, 7, 8, 9, 16, 17, 45)


def ragged_lower(n, empty_every=53, lone_every=211, seed=1):
    """Rows whose counts of lower entries cycle through RAGGED_COUNTS (the 8-entry batches of the colouring: none, one,
    one short of a batch, a full batch, one over, two batches, two and one, six batches), drawn from the 120 rows before
    the row; every lower entry has its mirror.  Columns are shuffled inside each row.  Every 37th row stores no diagonal;
    every `empty_every`-th row is empty and so is its column; every `lone_every`-th row holds its diagonal only; every 11th
    row stores one of its lower entries twice (the mirror once)."""
    rng = np.random.default_rng([seed, 6, n])

    def alone(r):
        return r % empty_every == 0 or r % lone_every == 0

    rows = [[] for _ in range(n)]
    for r in range(n):
        if alone(r):
            if r % empty_every != 0:
                rows[r].append(r)
            continue
        cand = [c for c in range(max(0, r - 120), r) if not alone(c)]
        want = min(RAGGED_COUNTS[r % 8], len(cand))
        lower = rng.choice(cand, want, replace=False).tolist() if want else []
        for c in lower:
            rows[c].append(r)
        rows[r] += lower
        if lower and r % 11 == 0:
            rows[r].append(lower[0])
        if r % 37 != 0:
            rows[r].append(r)
    vals = []
    for r in range(n):
        rng.shuffle(rows[r])
        vals.append([rng.uniform(1.0, 2.0) if c == r else rng.uniform(-1.0, 1.0) for c in rows[r]])
    return _from_rows(rows, vals)


def symmetric_part(A):
    """A restricted to its symmetric part: the first stored copy of every entry whose mirror is stored too (the diagonal
    stays); the order inside a row is kept."""
    rows, vals = _rows_of(A)
    have = [set(c) for c in rows]
    out_r, out_v = [], []
    for r in range(A.n_rows):
        seen, cr, vr = set(), [], []
        for c, v in zip(rows[r], vals[r]):
            if c in seen or (c != r and r not in have[c]):
                continue
            seen.add(c)
            cr.append(c)
            vr.append(v)
        out_r.append(cr)
        out_v.append(vr)
    return _from_rows(out_r, out_v)


def unsym(n, seed=1):
    """banded_sym(n, 2, 40) with a seeded third of its strictly lower entries removed (their mirrors stay)."""
    A = banded_sym(n, 2, 40, seed)
    rng = np.random.default_rng([seed, 8, n])
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.row_ptr))
    lower = np.flatnonzero(A.col < rows)
    keep = np.ones(A.nnz, dtype=bool)
    keep[rng.choice(lower, len(lower) // 3, replace=False)] = False
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))])
    return CRS(n, rp, A.col[keep], A.val[keep])
