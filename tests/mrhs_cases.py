"""Vectorised numpy generators for the multi-right-hand-side tests at sizes past the layer's grid caps and at the SpMM
tile's edges (tests/test_gpu_mrhs_scale.py, tests/test_gpu_spmm_edges.py); no GPU.  tests/test_mrhs_cases_cpu.py proves
the properties the GPU tests rely on.  The caps below restate the constants of the sources they are named after."""
import numpy as np

from oracle.pyoracle import CRS

# ---- the caps of the layer (csrc) ----
LOCKSTEP_T = 256            # kSolverT: lanes of a workgroup of an elementwise pass (bis_lockstep.hpp)
LOCKSTEP_MAX_BLOCKS = 2048  # kMaxReduceBlocks: lockstep_grid's cap
MVEC_DIAG_MAX_BLOCKS = 16384  # kMpMaxBlocks (bis_mprecond.hip), workgroups of 256 lanes
MVEC_COPY_MAX_BLOCKS = 8192   # copy_grid (bis_spmm.hip), workgroups of 256 lanes
LEVEL_BLOCKS_PER_CU = 32    # launch_level (bis_sptrsm.hip): n_cus * 32 workgroups of 256 lanes per level
WAVE_BLOCKS_PER_CU = 4      # kWaveBlocksPerCU: launch_wave's residency cap, n_cus * 4 / device_share workgroups of 4 waves
FEW_LEVELS = 64             # kFewLevels: more levels take the persistent form
SPMM_LDS = 3840             # kSpmmLds
SPMM_MAX_CHUNK = 4096       # kSpmmMaxChunk


def lockstep_act(k):
    """working lanes of a workgroup of a lock-step pass: the largest multiple of k in 256"""
    return (LOCKSTEP_T // k) * k


def lockstep_strides(n, k):
    """n k elements do not fit lockstep_grid's 2048 workgroups of act lanes: the passes take a second trip"""
    return n * k > LOCKSTEP_MAX_BLOCKS * lockstep_act(k)


def spmm_cap(k):
    """non-zeros of an LDS tile of spmm_rowblock_kernel (bis_spmm.hip: spmm_cap)"""
    return ((SPMM_LDS // k) & ~3) - 4


def wave_grid(n, max_level_width, n_cus, share=1, resident=WAVE_BLOCKS_PER_CU):
    """(grid, cap) of launch_wave (bis_sptrsm.hip)"""
    wg = (4 * max_level_width + 3) // 4 + 1
    cap = max(1, n_cus * resident // share)
    return max(1, min(wg, (n + 3) // 4, cap)), cap


def level_grid(width, k, n_cus):
    """(grid, cap) of launch_level for a level of `width` rows"""
    cap = n_cus * LEVEL_BLOCKS_PER_CU
    return max(1, min((width * k + 255) // 256, cap)), cap


# ---- matrices ----

def spd_band(n, half, seed):
    """Random symmetric, strictly diagonally dominant band (by a factor 1.1 .. 1.5): SPD.  tests/test_gpu_mcg.py::spd_band
    entry for entry (the same draws in the same order), built from the diagonals."""
    return crs_from_diagonals(n, spd_band_diagonals(n, half, seed))


def crs_from_diagonals(n, diags):
    """CRS of the square matrix with entry (r, r + d) = diags[d][min(r, r + d)] for every offset d in diags, columns ascending."""
    offs = sorted(diags)
    r = np.arange(n)
    cols = np.stack([r + d for d in offs], axis=1)                       # (n, n_offs)
    vals = np.empty(cols.shape)
    for i, d in enumerate(offs):
        v = np.asarray(diags[d], dtype=np.float64)
        assert len(v) == n - abs(d)
        vals[:, i] = 0.0
        if d >= 0:
            vals[:n - d, i] = v
        else:
            vals[-d:, i] = v
    keep = (cols >= 0) & (cols < n)
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    return CRS(n, rp, cols[keep].astype(np.int32), vals[keep])


def band_matvec(n, diags, X, dtype=np.longdouble):
    """A X for the matrix of crs_from_diagonals with sums in `dtype`; X is n or n x k."""
    X = np.asarray(X, dtype=dtype)
    Y = np.zeros_like(X)
    for d, v in diags.items():
        v = np.asarray(v, dtype=dtype)
        v = v if X.ndim == 1 else v[:, None]
        if d >= 0:
            Y[:n - d] += v * X[d:]
        else:
            Y[-d:] += v * X[:n + d]
    return Y


def spd_band_diagonals(n, half, seed):
    """the diagonals of spd_band(n, half, seed) as band_matvec takes them"""
    rng = np.random.default_rng(seed)
    off = {d: rng.uniform(-1, 1, n - d) for d in range(1, half + 1)}
    absum = np.zeros(n)
    for d, v in off.items():
        absum[:n - d] += np.abs(v)
        absum[d:] += np.abs(v)
    diag = absum * rng.uniform(1.1, 1.5, n) + 1e-3
    return {0: diag, **{d: off[d] for d in off}, **{-d: off[d] for d in off}}


def layered_lower(widths, fan, seed, scaled=True):
    """(T, D): a strictly lower triangle whose dependency levels are `widths` by construction, in row order: level l holds
    the next widths[l] rows.  Level 0's rows are empty; every row of level l > 0 holds one column of level l - 1 and
    fan - 1 further distinct columns drawn from all rows of the earlier levels (fewer where there are fewer such rows),
    columns ascending.  Row r's entries and its diagonal carry the row's scale 10^(-6..6), the entries divided by their
    count + 1, the diagonal in [1, 2] scale (as ragged_lower of tests/test_gpu_sptrsm.py), so that solutions stay finite."""
    rng = np.random.default_rng(seed)
    widths = [int(w) for w in widths]
    starts = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
    n = int(starts[-1])
    cols, cnts = [], [np.zeros(widths[0], dtype=np.int64)]
    for l in range(1, len(widths)):
        w, lo, hi = widths[l], int(starts[l - 1]), int(starts[l])
        cnt = min(fan, hi)
        c = np.empty((w, cnt), dtype=np.int64)
        c[:, 0] = rng.integers(lo, hi, w)
        if cnt > 1:
            c[:, 1:] = rng.integers(0, hi, (w, cnt - 1))
        for _ in range(1000):  # redraw the extra columns of the rows that hold a column twice
            s = np.sort(c, axis=1)
            bad = np.nonzero((s[:, 1:] == s[:, :-1]).any(axis=1))[0]
            if not len(bad):
                break
            c[bad, 1:] = rng.integers(0, hi, (len(bad), cnt - 1))
        else:
            raise AssertionError("layered_lower: could not draw distinct columns")
        cols.append(np.sort(c, axis=1).ravel())
        cnts.append(np.full(w, cnt, dtype=np.int64))
    cnt = np.concatenate(cnts)
    rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    col = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32)
    scale = 10.0 ** rng.uniform(-6, 6, n) if scaled else np.ones(n)
    per_entry = np.repeat(scale / (cnt + 1), cnt)
    val = per_entry * rng.uniform(-1, 1, len(col))
    D = scale * rng.uniform(1, 2, n)
    return CRS(n, rp, col, val), D


def mirror(T):
    """The strictly upper triangle with entry (n-1-r, n-1-c) for every entry (r, c) of the strictly lower T, columns
    ascending (tests/test_gpu_sptrsm.py::mirror): the non-zero stream reversed."""
    n = T.n_rows
    lens = np.diff(T.row_ptr)[::-1]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return CRS(n, rp, (n - 1 - np.asarray(T.col, dtype=np.int64))[::-1].astype(np.int32), np.ascontiguousarray(T.val[::-1]))


def level_widths(T, backward=False):
    """The widths of the dependency levels by a plain longest-path computation (level = 1 + the deepest dependency)."""
    n = T.n_rows
    rp, col = np.asarray(T.row_ptr, dtype=np.int64), np.asarray(T.col)
    lvl = np.zeros(n, dtype=np.int64)
    for r in (range(n - 1, -1, -1) if backward else range(n)):
        a, b = rp[r], rp[r + 1]
        if b > a:
            lvl[r] = lvl[col[a:b]].max() + 1
    return np.bincount(lvl).tolist() if n else []


def rows_at_cap(K, seed, extra=0, n_cols=4000):
    """(A, long_rows): a rectangular CRS matrix whose longest rows have exactly spmm_cap(K) - 3 + extra entries -- four of
    them, starting at offsets = 0, 1, 2, 3 (mod 4) of the non-zero stream; filler rows of 1, 2, 3 entries before each long
    row set the alignment, an empty row and a few short rows follow.  The long rows' columns are distinct and unsorted.
    extra = 0: max_row_nnz + 3 == cap(K), the longest row that still takes the LDS tile (at alignment 3 it fills the tile
    to the last slot); extra = 1: the shortest that takes the serial fallback."""
    rng = np.random.default_rng(seed)
    L = spmm_cap(K) - 3 + extra
    lens, long_rows, nnz = [], [], 0
    for align in (0, 1, 2, 3):
        need = (align - nnz) % 4
        for f in ([1, 3] if need == 0 else [need]):
            lens.append(f)
            nnz += f
        assert nnz % 4 == align
        long_rows.append(len(lens))
        lens.append(L)
        nnz += L
    lens += [0, 2, 1, 3, 0]
    rows = []
    for i, m in enumerate(lens):
        c = rng.choice(n_cols, m, replace=False)
        rows.append(c if i in long_rows else np.sort(c))
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    A = CRS(len(lens), rp, np.concatenate(rows).astype(np.int32), rng.uniform(-1, 1, int(rp[-1])), n_cols=n_cols)
    return A, long_rows


def band_lower_full(n, half, seed):
    """(diags, T, D_inv): every entry of the strictly lower band of half-width `half` -- diags[d][i] is entry (i + d, i) for
    d = 1 .. half (entries in (-1, 1) / half) -- its CRS arrays (columns ascending: r - half .. r - 1), and a reciprocal
    diagonal in [0.5, 1]."""
    rng = np.random.default_rng(seed)
    diags = {d: rng.uniform(-1, 1, n - d) / half for d in range(1, half + 1)}
    T = crs_from_diagonals(n, {-d: v for d, v in diags.items()})
    return diags, T, 1.0 / rng.uniform(1, 2, n)


def spmm_band_ref(diags, X):
    """bis_spmm's bits for the triangle of band_lower_full on the n x k block X: per row and column acc = 0, then for
    d = half .. 1 (CRS order) acc = acc + val_d * x[r - d], product and sum rounded separately (include/bis_hip.h) -- numpy
    does not fuse.  Rows r >= half are vectorised over rows and columns; the first `half` rows are shorter: a plain loop."""
    X = np.asarray(X, dtype=np.float64)
    n, half = X.shape[0], max(diags)
    Y = np.zeros_like(X)
    for d in range(half, 0, -1):  # rows half .. n - 1 hold every diagonal
        v = diags[d][half - d:]                      # entry (r, r - d), r = half .. n - 1
        Y[half:] = Y[half:] + v[:, None] * X[half - d:n - d]
    for r in range(min(half, n)):
        acc = np.zeros(X.shape[1])
        for d in range(r, 0, -1):
            acc = acc + diags[d][r - d] * X[r - d]
        Y[r] = acc
    return Y


def mitrsv_ref(diags, D_inv, B, sweeps):
    """bis_mitrsv's bits on the triangle of band_lower_full: x_0 = b D_inv, x_{s+1} = (b - T x_s) D_inv, every operation rounded."""
    Dc = D_inv[:, None]
    X = (B * 1.0) * Dc
    for _ in range(sweeps):
        X = (B - spmm_band_ref(diags, X)) * Dc
    return X


def rhs_columns(A_matvec, n, k, seed):
    """tests/test_gpu_mcg.py::columns with the product A 1 supplied by the caller: (B, X0), n x k."""
    rng = np.random.default_rng(seed)
    B = np.empty((n, k))
    X0 = np.zeros((n, k))
    scales = (1e-6, 1.0, 1e6)
    for j in range(k):
        if j == 0:
            B[:, j] = A_matvec(np.ones(n))
        elif j == 1:
            B[:, j] = rng.uniform(-1, 1, n)
        elif j == 2:
            B[:, j] = 0.0
            B[n // 3, j] = 1.0
        else:
            B[:, j] = scales[(j - 3) % 3] * rng.uniform(-1, 1, n)
        if j == 2:
            X0[:, j] = np.random.default_rng(2).uniform(-1, 1, n)
        elif j not in (0, 1, 3, 6):
            X0[:, j] = rng.uniform(-1, 1, n) * scales[(j - 3) % 3]
    return B, X0


def numpy_cg(matvec, b, x0, tol, max_iters, d=None):
    """Plain float64 CG (Jacobi-preconditioned with the diagonal d): (iterations, converged) under the stop test
    ||r|| < tol ||r_0||."""
    x = x0.copy()
    r = b - matvec(x)
    r0 = np.linalg.norm(r)
    z = r / d if d is not None else r
    p = z.copy()
    rz = r @ z
    for it in range(1, max_iters + 1):
        Ap = matvec(p)
        alpha = rz / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        if np.linalg.norm(r) < tol * r0:
            return it, True
        z = r / d if d is not None else r
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return max_iters, False


# ---- the sizes of tests/test_gpu_mrhs_scale.py (tests/test_mrhs_cases_cpu.py: each crosses its cap at n_cus = 256) ----
N_LOCKSTEP = 180001          # n k > 2048 act for every k >= 3 (k = 3 needs n > 174,080)
WAVE_WIDTHS = [1100] * 70    # 77,000 rows, 70 levels: widest level + 1 > 4 n_cus
WAVE_WIDTHS_SMALL = [300] * 70
WAVE_SHARE = 8
N_DIAG = 524301              # n k > 16,384 * 256 at k = 8
N_COPY = 2 ** 21 + 5         # n > 8,192 * 256


def level_w0(n_cus):
    """rows of level 0 of the per-level case: 5,000 more than n_cus 32 256 / 8, what one trip of the capped grid covers at k = 8"""
    return n_cus * LEVEL_BLOCKS_PER_CU * 256 // 8 + 5000
