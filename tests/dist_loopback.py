"""Single-process harness for the row-partitioned layer (bis_dist.hip): loop-back transports that serve the C-ABI's
communicator callbacks without a peer, plain numpy references of everything the layer computes, and the table of
irregular partitions the tests run on (test_dist_loopback_cpu.py, test_gpu_dist_loopback.py).  Test infrastructure."""
import contextlib
import ctypes as C

import numpy as np

from oracle.pyoracle import CRS

U = 2.0 ** -53


# ---- matrices ---------------------------------------------------------------------------------------------------------

def crs_from_coo(n_rows, rows, cols, vals, n_cols):
    """CRS from entry lists; entries keep their given order inside a row (duplicates and unsorted columns survive)."""
    rows = np.asarray(rows, dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_rows))]).astype(np.int64)
    return CRS(n_rows, rp, np.asarray(cols, dtype=np.int64)[order].astype(np.int32), np.asarray(vals, dtype=np.float64)[order],
               n_cols=n_cols)


def row_index(A):
    return np.repeat(np.arange(A.n_rows, dtype=np.int64), np.diff(A.row_ptr))


def local_rows(A, row0, row1):
    """Rows [row0, row1) of a global matrix, global column indices kept: what a rank hands to bis_dist_create."""
    k0, k1 = int(A.row_ptr[row0]), int(A.row_ptr[row1])
    return CRS(row1 - row0, A.row_ptr[row0:row1 + 1] - k0, A.col[k0:k1], A.val[k0:k1], n_cols=A.n_cols)


# ---- references -------------------------------------------------------------------------------------------------------

def ref_halo_plan(A_loc, row_starts, rank):
    """(halo, recv_counts, (a, b)): sorted distinct remote columns, how many of them each peer owns, and the first
    longest run of rows without a remote column."""
    rs = np.asarray(row_starts, dtype=np.int64)
    row0, row1 = int(rs[rank]), int(rs[rank + 1])
    n = A_loc.n_rows
    col = A_loc.col.astype(np.int64)
    remote = (col < row0) | (col >= row1)
    halo = np.unique(col[remote])
    owners = np.searchsorted(rs, halo, side="right") - 1  # the last p with row_starts[p] <= c: skips ranks without rows
    recv = np.bincount(owners, minlength=len(rs) - 1).astype(np.int64)
    brows = np.nonzero(np.bincount(row_index(A_loc)[remote], minlength=n))[0]
    starts, ends = np.concatenate([[0], brows + 1]), np.concatenate([brows, [n]])
    k = int(np.argmax(ends - starts))  # argmax returns the first maximum
    return halo.astype(np.int32), recv, (int(starts[k]), int(ends[k]))


def interior_runs(A_loc, row_starts, rank):
    """Lengths of all maximal runs of rows without a remote column, in row order."""
    rs = np.asarray(row_starts, dtype=np.int64)
    col = A_loc.col.astype(np.int64)
    remote = (col < rs[rank]) | (col >= rs[rank + 1])
    brows = np.nonzero(np.bincount(row_index(A_loc)[remote], minlength=A_loc.n_rows))[0]
    return np.concatenate([brows, [A_loc.n_rows]]) - np.concatenate([[0], brows + 1])


def ref_renumber(A_loc, halo, row0, row1):
    """The local matrix as bis_dist_create documents it: owned columns -> c - row0, the k-th halo column -> n_local + k."""
    nl = row1 - row0
    col = A_loc.col.astype(np.int64)
    own = (col >= row0) & (col < row1)
    lcol = np.where(own, col - row0, nl + np.searchsorted(halo, col)).astype(np.int32)
    return CRS(nl, A_loc.row_ptr, lcol, A_loc.val, n_cols=nl + len(halo))


def _row_sums(A, terms):
    out = np.zeros(A.n_rows, dtype=np.longdouble)
    nonempty = np.diff(A.row_ptr) > 0
    if terms.size:  # segments between the starts of consecutive non-empty rows are exactly those rows
        out[nonempty] = np.add.reduceat(terms, A.row_ptr[:-1][nonempty])
    return out


def ref_spmv(A, x):
    """(y, mag) in np.longdouble: y_i = sum_j a_ij x_j and mag_i = sum_j |a_ij| |x_j|, row by row."""
    prod = A.val.astype(np.longdouble) * np.asarray(x)[A.col].astype(np.longdouble)
    return _row_sums(A, prod), _row_sums(A, np.abs(prod))


def check_spmv_rows(y, A, x, tag):
    """|y_i - y^_i| <= (nnz_i + 2) 2^-53 sum_j |a_ij| |x_j|: the bound of an fma-accumulated dot of nnz_i terms with slack
    for another summation tree.  A row without entries must give exactly 0."""
    y_ref, mag = ref_spmv(A, x)
    y = np.asarray(y)
    assert y.shape == (A.n_rows,) and np.all(np.isfinite(y)), f"{tag}: non-finite y"
    nnz = np.diff(A.row_ptr)
    bad = np.nonzero(np.abs(y.astype(np.longdouble) - y_ref) > (nnz + 2) * np.longdouble(U) * mag)[0]
    assert bad.size == 0, f"{tag}: rows {bad[:5]} outside their bound: y={y[bad[:5]]} ref={y_ref[bad[:5]]}"
    assert np.all(y[nnz == 0] == 0.0), f"{tag}: an empty row is not exactly 0"


def ref_dot(a, b):
    """(sum a_i b_i, sum |a_i b_i|) in np.longdouble."""
    p = np.asarray(a).astype(np.longdouble) * np.asarray(b).astype(np.longdouble)
    return p.sum(), np.abs(p).sum()


def ref_diag(A_loc, row0):
    """(D, 1/D, status) of a row block with global columns, the last diagonal entry of a row winning.  status is None, or
    ("zero" | "none", global row) as peel_diag_crs reports it walking the rows in order: a diagonal entry below 1e-16 in
    magnitude stops it where it stands in the row, whatever follows; a row without a diagonal entry after its last."""
    n = A_loc.n_rows
    rows = row_index(A_loc)
    hit = np.nonzero(A_loc.col.astype(np.int64) == rows + row0)[0]
    D = np.ones(n)
    D[rows[hit]] = A_loc.val[hit]  # repeated index: the last assignment stays
    have = np.zeros(n, dtype=bool)
    have[rows[hit]] = True
    zero = np.zeros(n, dtype=bool)
    zero[rows[hit[np.abs(A_loc.val[hit]) < 1e-16]]] = True
    bad = np.nonzero(zero | ~have)[0]
    status = None
    if bad.size:
        status = ("zero" if zero[bad[0]] else "none", row0 + int(bad[0]))
    with np.errstate(divide="ignore"):
        return D, 1.0 / D, status


def ref_diag_block(A_loc, row0):
    """The square diagonal block: entries with row0 <= col < row0 + n, columns made local, order inside a row kept."""
    n = A_loc.n_rows
    col = A_loc.col.astype(np.int64)
    keep = (col >= row0) & (col < row0 + n)
    rp = np.concatenate([[0], np.cumsum(np.bincount(row_index(A_loc)[keep], minlength=n))]).astype(np.int64)
    return CRS(n, rp, (col[keep] - row0).astype(np.int32), A_loc.val[keep])


def spmv64(A, x):
    """Plain float64 y = A x (the reference solver's operator)."""
    return np.bincount(row_index(A), weights=A.val * x[A.col], minlength=A.n_rows)


def ref_pcg(A, b, x0, Minv, tol, max_iters):
    """Global preconditioned CG with the statements of the reference loop in tests/dist_worker.py (cg.hpp's schedule):
    (r, z) before the step, x and r updated, z = M^-1 r, beta from the new (r, z), the residual norm sampled last.
    Returns (x, history)."""
    x = x0.copy()
    r = b - spmv64(A, x)
    z = Minv(r)
    p = z.copy()
    hist = [np.sqrt(float(r @ r))]
    for _ in range(max_iters):
        t = spmv64(A, p)
        rz = float(r @ z)
        al = rz / float(t @ p)
        x = x + al * p
        r = r - al * t
        z = Minv(r)
        be = float(r @ z) / rz
        p = z + be * p
        hist.append(np.sqrt(float(r @ r)))
        if hist[-1] < tol * hist[0]:
            break
    return x, np.array(hist)


def make_minv(pc, oracle, blocks, diag, nl):
    """M^-1 of the global reference PCG: identity, the diagonal, or SGS of every rank's diagonal block (block-Jacobi of
    the sweeps, assembled from oracle sweeps as tests/dist_worker.py does)."""
    if pc == "none":
        return lambda v: v.copy()
    if pc == "j":
        return lambda v: v / diag
    facs = []
    for Bq in blocks:
        L_, Ls_, U_, Us_ = oracle.split_LU(Bq)
        D_, Dinv_, st = oracle.peel_diag(L_)
        assert st == 0
        facs.append((Ls_, Us_, D_, Dinv_))

    def minv(v):
        out = np.empty_like(v)
        for q, f in enumerate(facs):
            out[q * nl:(q + 1) * nl] = oracle.apply_preconditioner("sgs", f[0], f[1], f[2], f[3], None, None, v[q * nl:(q + 1) * nl])
        return out
    return minv


# ---- loop-back transports ---------------------------------------------------------------------------------------------

class _Loopback:
    """A CommOps whose callbacks are plain Python and talk to no peer.  They synchronise the stream they are handed and
    wait on nothing else, keep the first exception for the test (reraise()) and return 1 after one.

    launcher.torch_comm_ops wraps the device pointers in torch tensors; that needs torch imported BEFORE the library, as
    the multi-process worker and bench.py do: torch brings a HIP runtime of its own, the library then shares it.  A pytest
    process has loaded the library first and holds two runtimes, and the library's pointers and streams mean nothing to
    torch's.  So these callbacks copy and synchronise with the runtime the library itself is linked to (hipMemcpy and
    hipStreamSynchronize, looked up through the library's handle), which is right in either order."""

    def __init__(self):
        from basic_iterative_solvers_amd import CommOps, load_library
        self.hip = load_library()
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.error = None
        self.log = []  # "x" per exchange, the count per all-reduce, in call order
        self.ops = CommOps()
        self.ops.user = None
        self.ops.allreduce_sum = type(self.ops.allreduce_sum)(self._guard(self.allreduce))
        self.ops.exchange = type(self.ops.exchange)(self._guard(self.exchange))

    def _hip_ok(self, status, what):
        if status != 0:
            raise RuntimeError(f"{what}: HIP error {status}")

    def _guard(self, fn):
        def call(user, stream, *args):
            try:
                self._hip_ok(self.hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
                fn(*args)  # (its copies are blocking: done when it returns)
                return 0
            except Exception as ex:  # nothing may unwind through the C frames above
                if self.error is None:
                    self.error = ex
                return 1
        return call

    def reraise(self):
        if self.error is not None:
            err, self.error = self.error, None
            raise err

    @contextlib.contextmanager
    def checked(self):
        """Around a library call that uses the transport: what a callback raised comes out, in place of the status the
        library made of the callback's return value."""
        try:
            yield
        finally:
            self.reraise()

    def download(self, ptr, n):
        out = np.zeros(n)
        if n:
            self._hip_ok(self.hip.hipMemcpy(out.ctypes.data, ptr, 8 * n, 2), "hipMemcpy device to host")
        return out

    def upload(self, ptr, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        if arr.size:
            self._hip_ok(self.hip.hipMemcpy(ptr, arr.ctypes.data, 8 * arr.size, 1), "hipMemcpy host to device")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class KnownVectorTransport(_Loopback):
    """For SpMV and dot: the test holds the global x.  exchange checks the packed send buffer against x_glob[send_cols]
    bit for bit (and the counts it is handed against the plan's) and fills the halo with x_glob[halo_cols];
    allreduce_sum adds `others`, the host-computed sum of the other ranks' local dot products, to buf[0]."""

    def __init__(self, x_glob, send_counts, send_cols, halo_cols, recv_counts):
        super().__init__()
        self.x_glob = x_glob
        self.send_counts, self.send_cols = [int(c) for c in send_counts], np.asarray(send_cols, dtype=np.int64)
        self.halo_cols, self.recv_counts = np.asarray(halo_cols, dtype=np.int64), [int(c) for c in recv_counts]
        self.others = 0.0
        self.sendbuf_exact = []  # one entry per exchange

    def exchange(self, sendbuf, send_counts, recvbuf, recv_counts, n):
        self.log.append("x")
        got = ([int(send_counts[p]) for p in range(n)], [int(recv_counts[p]) for p in range(n)])
        ok = got == (self.send_counts, self.recv_counts)
        ok = ok and same_bits(self.download(sendbuf, len(self.send_cols)), self.x_glob[self.send_cols])
        self.sendbuf_exact.append(ok)
        self.upload(recvbuf, self.x_glob[self.halo_cols])

    def allreduce(self, buf, count):
        self.log.append(int(count))
        h = self.download(buf, count)
        h[0] += self.others
        self.upload(buf, h)


class ReplicatedWorldTransport(_Loopback):
    """For CG on a block-circulant world A = I (x) B + S (x) C + S^T (x) C^T with b and x0 equal on every rank: every rank
    holds the same vectors at every iteration, so rank 0 alone is created.  The halo entry for global column c of peer q
    is rank 0's own entry c - row_starts[q]; rank 0's local vector starts n_local doubles below the receive buffer; a sum
    over the ranks is P times rank 0's term."""

    def __init__(self, n_ranks, n_local, halo_cols, row_starts, send_cols):
        super().__init__()
        rs = np.asarray(row_starts, dtype=np.int64)
        halo = np.asarray(halo_cols, dtype=np.int64)
        self.P, self.n_local = n_ranks, n_local
        self.halo_local = halo - rs[np.searchsorted(rs, halo, side="right") - 1]
        self.send_local = np.asarray(send_cols, dtype=np.int64) - rs[0]
        self.sendbuf_exact = []

    def exchange(self, sendbuf, send_counts, recvbuf, recv_counts, n):
        self.log.append("x")
        v = self.download(recvbuf - 8 * self.n_local, self.n_local)
        self.sendbuf_exact.append(same_bits(self.download(sendbuf, len(self.send_local)), v[self.send_local]))
        self.upload(recvbuf, v[self.halo_local])

    def allreduce(self, buf, count):
        self.log.append(int(count))
        self.upload(buf, self.download(buf, count) * float(self.P))


def send_lists(plans, rank):
    """What the peers need from `rank`: (send_counts, send_cols) from every rank's (halo, recv) plan, in peer order --
    the routing the launcher does with an all-gather."""
    parts = []
    for halo, recv in plans:
        off = int(np.sum(recv[:rank]))
        parts.append(np.asarray(halo[off:off + int(recv[rank])], dtype=np.int32))
    return np.array([len(p) for p in parts], dtype=np.int64), (np.concatenate(parts) if parts else np.zeros(0, np.int32))


# ---- the case table ---------------------------------------------------------------------------------------------------

def _random_rows(rng, row_lo, row_hi, col_ranges, per_row, diag=True):
    """Entry lists for rows [row_lo, row_hi): 1..per_row random columns drawn from the union of col_ranges, plus one
    diagonal entry at a random place in the row."""
    nr = row_hi - row_lo
    lens = rng.integers(1, per_row + 1, nr)
    rows = np.repeat(np.arange(row_lo, row_hi), lens)
    widths = np.array([b - a for a, b in col_ranges])
    pick = rng.integers(0, widths.sum(), rows.size)
    edges = np.concatenate([[0], np.cumsum(widths)])
    seg = np.searchsorted(edges, pick, side="right") - 1
    cols = np.array([a for a, _ in col_ranges])[seg] + (pick - edges[seg])
    vals = rng.uniform(-1, 1, rows.size)
    if diag:
        rows = np.concatenate([rows, np.arange(row_lo, row_hi)])
        cols = np.concatenate([cols, np.arange(row_lo, row_hi)])
        vals = np.concatenate([vals, rng.uniform(1, 2, nr) * rng.choice([-1.0, 1.0], nr)])
        shuffle = rng.permutation(rows.size)  # the stable sort by row then leaves a random order inside every row
        rows, cols, vals = rows[shuffle], cols[shuffle], vals[shuffle]
    return rows, cols, vals


def _assemble(n, parts):
    rows, cols, vals = (np.concatenate([p[k] for p in parts]) for k in range(3))
    return crs_from_coo(n, rows, cols, vals, n)


CASES = ["all_to_all", "empty_rank", "no_halo", "all_boundary", "one_way", "skipped_owner", "ties", "untidy", "long"]


def make_case(name):
    """(A, row_starts, ranks to run, has_diag) of a named partition.  What each is there for is asserted on the numpy
    plan by check_case_property."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name in ("all_to_all", "empty_rank"):
        n = 3001
        A = _assemble(n, [_random_rows(np.random.default_rng(7), 0, n, [(0, n)], 9)])
        rs = [0, 517, 1700, 2303, n] if name == "all_to_all" else [0, 800, 800, 2000, n]
        return A, np.array(rs, dtype=np.int64), [0, 1, 2, 3], True
    if name == "no_halo":
        rs = [0, 1000, 2101, 3000]
        parts = [_random_rows(rng, a, b, [(a, b)], 7) for a, b in zip(rs[:-1], rs[1:])]
        return _assemble(3000, parts), np.array(rs, dtype=np.int64), [0, 1, 2], True
    if name == "all_boundary":
        rs = [0, 700, 1500, 2100]
        parts = []
        for p, (a, b) in enumerate(zip(rs[:-1], rs[1:])):
            parts.append(_random_rows(rng, a, b, [(a, b)], 4))
            others = np.concatenate([np.arange(x, y) for q, (x, y) in enumerate(zip(rs[:-1], rs[1:])) if q != p])
            parts.append((np.arange(a, b), rng.choice(others, b - a), rng.uniform(-1, 1, b - a)))  # one remote column per row
        return _assemble(2100, parts), np.array(rs, dtype=np.int64), [0, 1, 2], True
    if name == "one_way":
        n, cut = 2500, 1301
        parts = [_random_rows(rng, 0, cut, [(0, n)], 6), _random_rows(rng, cut, n, [(cut, n)], 6)]
        return _assemble(n, parts), np.array([0, cut, n], dtype=np.int64), [0, 1], True
    if name == "skipped_owner":
        rs = [0, 600, 1300, 1900, 2600]
        parts = [_random_rows(rng, 0, 600, [(0, 1300), (1900, 2600)], 6)]
        parts += [_random_rows(rng, a, b, [(0, 600), (a, b)], 6) for a, b in zip(rs[1:-1], rs[2:])]
        return _assemble(2600, parts), np.array(rs, dtype=np.int64), [0, 1, 2, 3], True
    if name == "ties":
        # rank 0: boundary rows 100, 401, 702, 1003, then every 50th: a run of 100, three of 300, short ones after
        n, cut = 3000, 2000
        brows = np.concatenate([[100, 401, 702, 1003], np.arange(1050, cut, 50)])
        parts = [_random_rows(rng, 0, cut, [(0, cut)], 5), _random_rows(rng, cut, n, [(0, n)], 5),
                 (brows, rng.integers(cut, n, brows.size), rng.uniform(-1, 1, brows.size))]
        return _assemble(n, parts), np.array([0, cut, n], dtype=np.int64), [0, 1], True
    if name == "untidy":
        # rows of 0..8 entries in random order; boundary rows repeat remote columns; some rows repeat the diagonal (the
        # last entry wins) and some rows are empty
        rs = [0, 900, 1801, 2700]
        n = 2700
        rows, cols, vals = _random_rows(rng, 0, n, [(0, n)], 6, diag=False)
        near = rng.random(rows.size) < 0.8  # most entries near the diagonal, so that interior rows exist
        cols = np.where(near, np.clip(rows + rng.integers(-40, 41, rows.size), 0, n - 1), cols)
        dup = rng.random(rows.size) < 0.3  # repeated (row, column) pairs with values of their own
        rows, cols = np.concatenate([rows, rows[dup]]), np.concatenate([cols, cols[dup]])
        vals = np.concatenate([vals, rng.uniform(-1, 1, int(dup.sum()))])
        drows = np.arange(n)
        d2 = drows[rng.random(n) < 0.2]  # a second diagonal entry
        rows, cols = np.concatenate([rows, drows, d2]), np.concatenate([cols, drows, d2])
        vals = np.concatenate([vals, rng.uniform(1, 2, n), rng.uniform(-2, -1, d2.size)])
        shuffle = rng.permutation(rows.size)
        rows, cols, vals = rows[shuffle], cols[shuffle], vals[shuffle]
        keep = ~np.isin(rows, rng.choice(n, 150, replace=False))  # empty rows
        return crs_from_coo(n, rows[keep], cols[keep], vals[keep], n), np.array(rs, dtype=np.int64), [0, 1, 2], False
    if name == "long":
        # two ranks of more than 140 000 rows (three chunks of the 256-block scan each) and a third that is not run
        rs = [0, 140001, 281003, 290000]
        n = rs[-1]
        rows = np.repeat(np.arange(n), 3)
        cols = np.clip(rows + rng.integers(-300, 301, rows.size), 0, n - 1)
        far = rng.random(rows.size) < 0.04  # scattered remote columns all over the other ranks
        cols = np.where(far, rng.integers(0, n, rows.size), cols)
        vals = rng.uniform(-1, 1, rows.size)
        rows, cols = np.concatenate([rows, np.arange(n)]), np.concatenate([cols, np.arange(n)])
        vals = np.concatenate([vals, rng.uniform(1, 2, n)])
        shuffle = rng.permutation(rows.size)
        return crs_from_coo(n, rows[shuffle], cols[shuffle], vals[shuffle], n), np.array(rs, dtype=np.int64), [0, 1], True
    raise KeyError(name)


def check_case_property(name, A, row_starts, plans):
    """The input really has the property the case is there for (plans: ref_halo_plan of every rank)."""
    P = len(row_starts) - 1
    nl = np.diff(row_starts)
    n_halo = [len(h) for h, _, _ in plans]
    n_send = [int(send_lists([(h, r) for h, r, _ in plans], p)[0].sum()) for p in range(P)]
    if name == "all_to_all":
        for p in range(P):
            sc = send_lists([(h, r) for h, r, _ in plans], p)[0]
            assert np.count_nonzero((plans[p][1] > 0) | (sc > 0)) >= 3
        assert len(set(nl.tolist())) == P  # uneven cuts
    elif name == "empty_rank":
        assert np.count_nonzero(nl == 0) == 1 and P == 4
    elif name == "no_halo":
        assert P == 3 and all(h == 0 for h in n_halo) and all(plans[p][2] == (0, int(nl[p])) for p in range(P))
    elif name == "all_boundary":
        assert all(plans[p][2][0] == plans[p][2][1] for p in range(P)) and all(h > 0 for h in n_halo)
    elif name == "one_way":
        assert P == 2 and n_halo[0] > 0 and n_send[0] == 0 and n_halo[1] == 0 and n_send[1] > 0
    elif name == "skipped_owner":
        recv = plans[0][1]
        assert P == 4 and recv[1] > 0 and recv[2] == 0 < recv[3]
    elif name == "ties":
        runs = interior_runs(local_rows(A, 0, int(row_starts[1])), row_starts, 0)
        first = int(np.argmax(runs))
        assert np.count_nonzero(runs == runs.max()) >= 3 and first > 0  # a shorter run comes before the tied ones
        a, b = plans[0][2]
        assert (a, b) == (101, 401)  # the first of the tied runs
    elif name == "untidy":
        for p in range(P):
            Al = local_rows(A, int(row_starts[p]), int(row_starts[p + 1]))
            col = Al.col.astype(np.int64)
            remote = (col < row_starts[p]) | (col >= row_starts[p + 1])
            rows = row_index(Al)
            key = rows * A.n_cols + col
            assert len(np.unique(key[remote])) < int(remote.sum())  # a remote column repeated inside a row
            brow = np.zeros(Al.n_rows, dtype=bool)
            brow[rows[remote]] = True
            inrow_unsorted = (np.diff(col) < 0) & (np.diff(rows) == 0)
            assert np.any(inrow_unsorted & brow[rows[1:]])  # unsorted columns in a boundary row
            assert np.any(np.diff(Al.row_ptr) == 0) and 0 < plans[p][2][1] - plans[p][2][0] < Al.n_rows
    elif name == "long":
        for p in (0, 1):
            assert nl[p] >= 140000 and (nl[p] + 255) // 256 > 512
            Al = local_rows(A, int(row_starts[p]), int(row_starts[p + 1]))
            col = Al.col.astype(np.int64)
            remote = (col < row_starts[p]) | (col >= row_starts[p + 1])
            chunk = row_index(Al)[remote] // 65536  # rows of one chunk of 256 block sums
            assert set(chunk.tolist()) == {0, 1, 2}
            assert abs(Al.nnz / Al.n_rows - 4.0) < 0.01


def case_plans(A, row_starts):
    P = len(row_starts) - 1
    return [ref_halo_plan(local_rows(A, int(row_starts[p]), int(row_starts[p + 1])), row_starts, p) for p in range(P)]


# ---- replicated world (distributed CG) ----------------------------------------------------------------------------------

def replicated_world(P, n_local, last_low_boundary, seed):
    """Rank 0's rows and the global matrix of A = I (x) B + S (x) C + S^T (x) C^T (S: cyclic shift of P ranks).  B: random
    symmetric, about 8 entries per row; C: sparse, its rows and columns scattered over [5, last_low_boundary] and the last
    quarter of the rows, so that the interior run of every rank is (last_low_boundary + 1, first high boundary row) with
    boundary rows on both sides.  Diagonal = sum |off-diagonal| + 1.  Returns (A_glob, A_loc0, row_starts)."""
    rng = np.random.default_rng(seed)
    nl = n_local
    i = rng.integers(0, nl, 4 * nl)
    j = rng.integers(0, nl, 4 * nl)
    pairs = np.unique(np.minimum(i, j) * nl + np.maximum(i, j))  # every pair once: the blocks feed triangular sweeps
    i, j = pairs // nl, pairs % nl
    i, j = i[i != j], j[i != j]
    v = rng.uniform(-1, 1, i.size)
    Bi, Bj, Bv = np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([v, v])
    hi0 = 3 * nl // 4
    pool = np.concatenate([rng.choice(np.arange(5, last_low_boundary), min(60, last_low_boundary // 3), replace=False),
                           [last_low_boundary], rng.choice(np.arange(hi0, nl - 3), min(80, nl // 12), replace=False)])
    Ci, Cj = rng.choice(pool, 2 * pool.size), rng.choice(pool, 2 * pool.size)
    Ci, Cj = np.concatenate([Ci, pool]), np.concatenate([Cj, rng.permutation(pool)])  # every pool row is a boundary row
    Cv = rng.uniform(-1, 1, Ci.size)
    rows, cols, vals = [], [], []
    for p in range(P):
        up, dn = (p + 1) % P, (p - 1) % P
        rows += [Bi + p * nl, Ci + p * nl, Cj + p * nl]
        cols += [Bj + p * nl, Cj + up * nl, Ci + dn * nl]
        vals += [Bv, Cv, Cv]
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    n = P * nl
    diag = np.bincount(rows, weights=np.abs(vals), minlength=n) + 1.0
    rows, cols, vals = np.concatenate([rows, np.arange(n)]), np.concatenate([cols, np.arange(n)]), np.concatenate([vals, diag])
    order = np.lexsort((cols, rows))  # ascending columns inside a row
    A = crs_from_coo(n, rows[order], cols[order], vals[order], n)
    rs = np.arange(P + 1, dtype=np.int64) * nl
    return A, local_rows(A, 0, nl), rs
