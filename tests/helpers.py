"""Shared helpers for the parity tests (test infrastructure)."""
import json
import os

import numpy as np

from oracle.pyoracle import CRS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_MATS = ["FDM-2d-16", "matrix_band_klein", "hpcg8", "hpcg_4x6x5",
               "anderson8_shift9", "anderson6_raw"]


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, f"golden_{name}.npz")))


def crs_of(g, prefix):
    rp = g[prefix + "_rp"]
    return CRS(len(rp) - 1, rp, g[prefix + "_col"], g[prefix + "_val"])


def load_ilu_edges():
    """The ILU(0) edge-case fixture (tests/golden/make_golden.py --ilu-edges-only): {case: dict(A, Ls, Us, L_D, U_D, y,
    pc_ilu0, exact)} -- input CRS, the reference's factor_ILU0_old factors, its ILU(0) apply of y, and whether every
    operation of the factorisation is exact (then any correctly rounded implementation gives the same bits)."""
    g = np.load(os.path.join(GOLDEN, "golden_ilu_edges.npz"))
    out = {}
    for name, exact in zip(g["names"], g["exact"]):
        name = str(name)
        out[name] = dict(A=crs_of(g, name + "__A"), Ls=crs_of(g, name + "__Ls"), Us=crs_of(g, name + "__Us"),
                         L_D=g[name + "__LD"], U_D=g[name + "__UD"], y=g[name + "__y"], pc_ilu0=g[name + "__pc_ilu0"],
                         exact=bool(exact))
    return out


def has_repeated_column(A):
    """Some row of A holds a column more than once."""
    return any(len(np.unique(A.col[A.row_ptr[r]:A.row_ptr[r + 1]])) < A.row_ptr[r + 1] - A.row_ptr[r]
               for r in range(A.n_rows))


def load_histories():
    with open(os.path.join(GOLDEN, "histories.json")) as f:
        return json.load(f)


def load_histories_mid():
    """Mid-size reference histories (tests/golden/make_golden.py --mid-only): inputs are generator strings."""
    with open(os.path.join(GOLDEN, "histories_mid.json")) as f:
        return json.load(f)


def gen_from_cli_arg(orc, arg):
    """The oracle's matrix for a host-CLI generator string (hpcg:N | anderson:L,shift=S | fem:X,Y,Z)."""
    kind, rest = arg.split(":")
    parts = rest.split(",")
    nums = [int(p) for p in parts if "=" not in p]
    kw = {k: float(v) for k, v in (p.split("=") for p in parts if "=" in p)}
    if kind == "hpcg":
        return orc.gen_hpcg(*nums)
    if kind == "anderson":
        return orc.gen_anderson(nums[0], shift=kw.get("shift", 0.0))
    if kind == "unstr":
        return orc.gen_unstr(*nums)
    return orc.gen_fem(*nums)


def parse_hist_key(key):
    name, solver, pc, kws = key.split("|")
    kw = {}
    for item in filter(None, kws.split(",")):
        k, v = item.split("=")
        kw[k] = (v == "True") if v in ("True", "False") else int(v)
    return name, solver, pc, kw


def relerr(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    denom = np.max(np.abs(b)) if b.size else 1.0
    if denom == 0.0:
        denom = 1.0
    return float(np.max(np.abs(a - b)) / denom) if a.size else 0.0


def hist_dev(h, g):
    """max_k |h_k - g_k| / g_0 over the common window."""
    n = min(len(h), len(g))
    h = np.asarray(h[:n])
    g = np.asarray(g[:n])
    return float(np.max(np.abs(h - g)) / g[0])


# Residual-history parity gate (SURVEY.md section 8d / section 7 "parity
# tolerance").  All deviations are max_k |r_k - r_k^ref| / r_0.
#   CG / Jacobi / GS / SGS      : 1e-10 over the whole history
#   BiCGSTAB                    : 1e-10 over the first 2 iterations, 1e-4 over
#       the whole history -- BiCGSTAB amplifies rounding differences (1e-16
#       -> 6e-7 at iteration 3 on matrix_band_klein -bi -p sgs): the
#       reference itself moves by 9.3e-6 between 1 and 8 threads (HPCG-64,
#       SURVEY.md section 7) and by 6.3e-5 against a differently-rounded
#       restatement on matrix_band_klein (-bi -p gs)
#   GMRES                       : 1e-10 over the whole history (preconditioned
#       residual estimate |g_{j+1}|)
# Iteration counts are compared exactly only where the stopping decision is
# not a rounding tie: TOL = 1e-14 puts the threshold at the rounding floor, so
# two correct implementations may stop one rounding-level iteration apart
# (seen for GMRES on FDM-2d-16: 34 vs 51 iterations with |dr| = 4e-14 r0).
HIST_TOL = {"cg": 1e-10, "j": 1e-10, "gs": 1e-10, "sgs": 1e-10, "gm": 1e-10,
            "bi": 1e-4}


def load_histories_r4():
    """Round-4 reference histories (tests/golden/make_golden.py --r4-only): the first 100 CG iterations on the raw
    (indefinite) Anderson operator, and the unstructured config-5 input with the solver pairs of configs 5 and 4."""
    with open(os.path.join(GOLDEN, "histories_r4.json")) as f:
        return json.load(f)


def permute_crs(A, perm):
    """B = P A P^T for perm[new] = old, entries keeping their order inside a row (what bis_mat_permute builds)."""
    perm = np.asarray(perm, dtype=np.int64)
    n = A.n_rows
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    lens = np.diff(A.row_ptr)[perm]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    src = np.repeat(A.row_ptr[:-1][perm] - rp[:-1], lens) + np.arange(rp[-1])
    return CRS(n, rp, inv[A.col[src]].astype(np.int32), A.val[src])


def check_history(r, e, solver, scale=1.0, stable_window=False, long_history=False):
    """stable_window: compare only the part of the reference history that is
    independent of rounding (golden `stable_len`: where the reference and the
    oracle -- same algorithm, different rounding -- still agree to 1e-9 r0).
    Used for the GPU path; the few BiCGSTAB runs that sit at a breakdown
    ((r0~, v) cancelling exactly: matrix_band_klein -bi -p gs reaches 38
    iterations in the reference, 30 in the oracle, and an exact 0/0 with a tree
    reduction) cannot be compared past that point by any implementation."""
    g = np.array(e["hist"])
    h = np.asarray(r["hist"])
    if stable_window and e.get("stable_len", len(g)) < len(g):
        n = max(1, min(e["stable_len"], len(h)))
        assert len(h) >= min(e["stable_len"], len(g)) or not np.all(np.isfinite(h))
        assert hist_dev(h[:n], g[:n]) <= 1e-8
        return
    tol = HIST_TOL[solver] * scale
    unstable = bool(np.any(g > 1e3 * g[0])) or not np.all(np.isfinite(g))
    if unstable:
        # divergent / chaotic in the reference itself: compare until the
        # history leaves 1e3 * r0 (at most 50 iterations), loosely
        bad = ~(g <= 1e3 * g[0])
        n = int(np.argmax(bad)) if np.any(bad) else len(g)
        n = max(1, min(n, 50, len(h)))
        assert hist_dev(h[:n], g[:n]) <= 1e-8
        return
    if solver == "bi":
        k = min(3, len(g), len(h))
        assert hist_dev(h[:k], g[:k]) <= 1e-10 * scale
    assert hist_dev(h, g) <= tol
    if e["iters"] is not None and solver in ("cg", "j", "gs", "sgs"):
        n = min(len(h), len(g))
        if len(h) != len(g):
            # TOL = 1e-14 puts the stopping threshold inside the rounding floor, where the iteration at which a run
            # crosses it is a property of its rounding, not of the algorithm: 2 iterations on the small inputs, up to
            # 10 % of a long history.  HPCG-32 -sgs: the reference's last eight residuals wander between 1.63e-12 and
            # 1.84e-12 around the threshold 1.648e-12; it stops at 895, the GPU at 892, 6e-16 r0 apart.  HPCG-48 -cg:
            # the reference (sequential sums of 10^5 terms in its dots) needs 104 iterations, the GPU (tree sums) 96,
            # the two histories 9e-13 r0 apart at most.  The histories themselves are held to `tol` over the common
            # window above, and the shorter run's last residual to `tol` of the longer one's at the same index below.
            # (the wide allowance is for the mid-size inputs only -- `long_history` -- whose stopping iteration is the
            # rounding noise described above; the small goldens hold at 2.  Either way the longer run's extra entries
            # must already sit at the floor the comparison itself resolves: the shorter run has crossed the threshold, the longer one
            # is within `tol` r0 of it at that index, and every residual behind stays below 2 tol r0 + 10 x the threshold.)
            assert abs(len(h) - len(g)) <= (max(2, len(g) // 10) if long_history else 2)
            assert abs(h[n - 1] - g[n - 1]) <= tol * g[0]
            longer = h if len(h) > len(g) else g
            stop = e.get("stopping") or 1e-14 * g[0]
            assert np.all(np.asarray(longer[n - 1:]) <= 2.0 * tol * g[0] + 10.0 * max(stop, 1e-14 * g[0]))
        else:
            assert r["converged"] == e["converged"]


# ---- SpMV matrix catalogue, per-row reference and option scopes (test_gpu_option_paths.py, test_gpu_kernels.py) ----

def random_spmv_case(seed):
    """Seeded random SpMV input across the format decisions (row lengths around the lane-per-row limit, value pools around
    255 / 256 / 257, banded / windowed / scattered columns, with and without a full diagonal, empty rows, rectangular):
    (A, x, rp64) -- rp64 is the row-pointer width the case asks for (option force_rp64)."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 6000))
    n_cols = n + int(rng.integers(0, 2)) * int(rng.integers(0, 500))
    max_len = int(rng.choice([1, 3, 7, 27, 39, 40, 41, 45]))
    lens = rng.integers(0, max_len + 1, n)
    if rng.integers(0, 2):
        lens[rng.integers(0, n, max(1, n // 10))] = 0
    lens = np.minimum(lens, n_cols)
    pool_n = int(rng.choice([1, 2, 17, 255, 256, 257, 400]))
    pool = np.unique(rng.uniform(-4, 4, pool_n + 8))[:pool_n]
    style = int(rng.integers(0, 3))  # 0 band around the row, 1 a few far windows, 2 scattered
    full_diag = bool(rng.integers(0, 2)) and n_cols >= n
    rp = np.concatenate([[0], np.cumsum(lens)])
    col = np.empty(rp[-1], dtype=np.int32)
    val = np.empty(rp[-1])
    offs = rng.integers(0, max(n_cols - 64, 1), 5)
    for r in range(n):
        k0, k1 = rp[r], rp[r + 1]
        m = k1 - k0
        if m == 0:
            continue
        if style == 0:
            cand = np.arange(max(0, r - 60), min(n_cols, r + 61))
        elif style == 1:
            cand = np.unique(np.concatenate([(o + np.arange(64)) % n_cols for o in offs] + [np.array([min(r, n_cols - 1)])]))
        else:
            cand = np.arange(n_cols)
        c = rng.choice(cand, size=min(m, len(cand)), replace=False)
        if len(c) < m:
            c = np.concatenate([c, rng.choice(cand, size=m - len(c))])  # duplicates allowed
        if full_diag and r not in c:
            c[0] = r
        col[k0:k1] = np.sort(c) if rng.integers(0, 2) else c
        val[k0:k1] = rng.choice(pool, size=m)
        if full_diag:
            hit = np.nonzero(col[k0:k1] == r)[0]
            val[k0 + hit[:1]] = rng.uniform(5, 6)  # a distinct diagonal value per row
    A = CRS(n, rp, col, val, n_cols=n_cols)
    x = rng.uniform(-1, 1, n_cols)
    return A, x, int(rng.integers(0, 2)), dict(n=n, max_len=max_len, pool_n=pool_n, style=style, full_diag=full_diag)


def _crs_from_rows(rows, vals, n_cols):
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int64)
    col = np.array([c for cs in rows for c in cs], dtype=np.int32)
    val = np.array([v for vs in vals for v in vs], dtype=np.float64)
    return CRS(len(rows), rp, col, val, n_cols=n_cols)


def _banded(n, n_cols, half, rng, skip_last_cols=0):
    """Rows of the band [r - half, r + half] (clipped), random values; the last skip_last_cols columns stay unreferenced."""
    m = n_cols - skip_last_cols
    rows = [list(range(max(0, min(r, m - 1) - half), min(m, min(r, m - 1) + half + 1))) for r in range(n)]
    return _crs_from_rows(rows, [rng.uniform(-1, 1, len(c)) for c in rows], n_cols)


def row_blocks(A, chunk):
    """The library's row-block table for a chunk (row_blocks_kernel): block k starts at the first row r with
    row_ptr[r] + r >= k * chunk."""
    rp = np.asarray(A.row_ptr, dtype=np.int64)
    nb = max(1, -(-(int(rp[-1]) + A.n_rows) // chunk))
    key = rp[:A.n_rows + 1] + np.arange(A.n_rows + 1)
    starts = np.searchsorted(key, np.arange(nb, dtype=np.int64) * chunk, side="left")
    return np.concatenate([starts, [A.n_rows]])


def window_fits(A, chunk):
    """Whether the x-window structure (spmv_window = 1) is built for A at this chunk: the LDS budget
    chunk + longest row + 8 <= 6144 doubles and at most 128 tiles of 16 columns per row block (bis_spmv_build_window)."""
    lens = np.diff(A.row_ptr)
    if A.nnz == 0 or A.n_rows == 0 or chunk + int(lens.max()) + 8 > 6144:
        return False
    br = row_blocks(A, chunk)
    rp = np.asarray(A.row_ptr, dtype=np.int64)
    for b in range(len(br) - 1):
        s, e = rp[br[b]], rp[br[b + 1]]
        if len(np.unique(A.col[s:e] // 16)) > 128:
            return False
    return True


SPMV_CATALOGUE = ["blocks1", "blocks7", "blocks8", "blocks9", "blocks15", "blocks17", "blocks23", "blocks25",
                  "small_rows", "long_row", "very_long_row", "chunk_boundary", "empty_edges", "wide_cols", "tall_rows",
                  "unsorted_dups", "extreme_values", "banded_window", "hpcg", "anderson", "random3", "random7"]


def spmv_catalogue_case(name, oracle):
    """(A, rp64) of a named SpMV edge case.  blocksK: rows of 3 non-zeros with K row blocks at chunk 1024 (the XCD-remap
    windows: 8 G +- 1 for G = 2, 3); small_rows: fewer than 256 rows; long_row: one row longer than the chunk;
    very_long_row: a row past the LDS budget of every chunk (the wave-per-row kernel); chunk_boundary: rows that end exactly
    where a 1024-chunk block ends; empty_edges: empty rows at the start and the end of every block; wide_cols / tall_rows:
    n_cols > n_rows and n_cols < n_rows; unsorted_dups: unsorted columns with duplicates; extreme_values: -0.0, 5e-324 and
    +-1.79e308; banded_window: qualifies for the window kernel; hpcg / anderson: generator matrices (value dictionary);
    randomK: test_spmv_formats_randomised_differential's seeds.  rp64 cases also run with 64-bit row pointers."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name.startswith("blocks"):
        k = int(name[6:])
        n = 256 * k - 10  # (3 n + n) / 1024 rounded up = k
        return _banded(n, n, 1, rng), k % 2
    if name == "small_rows":
        return _banded(200, 230, 4, rng, skip_last_cols=20), 0
    if name in ("long_row", "very_long_row"):
        n = 3000 if name == "long_row" else 12000
        L = 1500 if name == "long_row" else 9000
        A = _banded(n, n, 2, rng)
        rows = [list(A.col[A.row_ptr[r]:A.row_ptr[r + 1]]) for r in range(n)]
        vals = [list(A.val[A.row_ptr[r]:A.row_ptr[r + 1]]) for r in range(n)]
        r = n // 3
        rows[r] = sorted(rng.choice(n, L, replace=False).tolist())
        vals[r] = rng.uniform(-1, 1, L).tolist()
        return _crs_from_rows(rows, vals, n), int(name == "very_long_row")
    if name == "chunk_boundary":
        # rows of 7: row_ptr[r] + r = 8 r, so every 128th row ends exactly on a 1024 boundary of the block table
        n = 128 * 20
        rows = [[(r + d) % n for d in range(-3, 4)] for r in range(n)]
        return _crs_from_rows(rows, [rng.uniform(-1, 1, 7) for _ in rows], n), 0
    if name == "empty_edges":
        n = 6000
        lens = rng.integers(1, 9, n)
        for s in range(0, n, 150):
            lens[s:s + 3] = 0
            lens[max(0, s - 3):s] = 0
        lens[:5] = 0
        lens[-5:] = 0
        rows = [sorted(rng.choice(np.arange(max(0, r - 40), min(n, r + 40)), int(lens[r]), replace=False).tolist())
                for r in range(n)]
        return _crs_from_rows(rows, [rng.uniform(-1, 1, len(c)) for c in rows], n), 1
    if name == "wide_cols":
        return _banded(3000, 7000, 3, rng, skip_last_cols=500), 0
    if name == "tall_rows":
        return _banded(7000, 2500, 2, rng, skip_last_cols=100), 1
    if name == "unsorted_dups":
        n = 5000
        rows = []
        for r in range(n):
            mid = min(r, n - 81)  # (the last 50 columns stay unreferenced)
            c = rng.integers(max(0, mid - 30), mid + 31, int(rng.integers(1, 12))).tolist()
            c = c + c[:int(rng.integers(0, 3))]  # duplicates
            rng.shuffle(c)
            rows.append(c)
        return _crs_from_rows(rows, [rng.uniform(-1, 1, len(c)) for c in rows], n), 0
    if name == "extreme_values":
        A = _banded(4000, 4000, 3, rng)
        v = A.val.copy()
        pick = rng.random(len(v))
        v[pick < 0.1] = -0.0
        v[(pick >= 0.1) & (pick < 0.2)] = 5e-324
        v[(pick >= 0.2) & (pick < 0.25)] = 1.79e308
        v[(pick >= 0.25) & (pick < 0.3)] = -1.79e308
        return CRS(A.n_rows, A.row_ptr, A.col, v, n_cols=A.n_cols), 1
    if name == "banded_window":
        return _banded(20000, 20000, 5, rng), 0
    if name == "hpcg":
        return oracle.gen_hpcg(16, 12, 10), 0
    if name == "anderson":
        return oracle.gen_anderson(14, shift=9.0), 1
    if name.startswith("random"):
        A, _, rp64, _ = random_spmv_case(int(name[6:]))
        return A, rp64
    raise KeyError(name)


def spmv_catalogue_x(A, seed=0, scale=1.0):
    """x for a catalogue matrix: uniform in [-scale, scale], -0.0 at some referenced columns, +Inf, -Inf and NaN at columns
    no row references (where there are any)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-scale, scale, A.n_cols)
    used = np.zeros(A.n_cols, dtype=bool)
    used[A.col] = True
    ref = np.nonzero(used)[0]
    x[ref[rng.random(len(ref)) < 0.05]] = -0.0
    free = np.nonzero(~used)[0]
    for k, c in enumerate(free):
        x[c] = (np.inf, -np.inf, np.nan)[k % 3]
    return x


def check_rows(y, A, x, tag=""):
    """Per-row bound against the exact sum of the rounded products: y_hat_i = fsum_j(a_ij x_j) and
    |y_i - y_hat_i| <= (n_i + 2) 2^-53 sum_j |a_ij x_j| + n_i 2^-1074 for every row (a row whose bound is 0 gives exactly 0);
    a row with a non-finite product must give Inf of the same sign where the products hold infinities of one sign only,
    NaN otherwise.  Every row is checked on its own magnitude, not the largest row's."""
    import math
    y = np.asarray(y)
    rp = np.asarray(A.row_ptr, dtype=np.int64)
    with np.errstate(all="ignore"):
        prod = A.val * x[A.col]
    bad = []
    for i in range(A.n_rows):
        p = prod[rp[i]:rp[i + 1]]
        n_i = len(p)
        if not np.all(np.isfinite(p)):
            if np.any(np.isnan(p)) or (np.any(p == np.inf) and np.any(p == -np.inf)):
                ok = bool(np.isnan(y[i]))
            else:
                ok = y[i] == (np.inf if np.any(p == np.inf) else -np.inf)
        else:
            try:
                exact = math.fsum(p.tolist())
                mag = math.fsum(np.abs(p).tolist())
                bound = (n_i + 2) * 2.0 ** -53 * mag + n_i * 2.0 ** -1074
            except OverflowError:  # the exact sum leaves the double range: only the class can be held
                exact, bound = None, math.inf
            if exact is None:
                ok = not np.isnan(y[i])
            elif bound == 0.0:
                ok = y[i] == 0.0
            else:
                ok = bool(abs(y[i] - exact) <= bound)
        if not ok:
            bad.append(i)
            if len(bad) >= 5:
                break
    assert not bad, f"{tag}: rows {bad} outside their own bound: y={[y[i] for i in bad]}"


class OptionScope:
    """Sets library options for a block and resets every one of them to -1 afterwards; checks that ctx.options() is back
    at its baseline.  Options read when a matrix is built (chunks, packed forms, the window) need the matrix created
    inside the scope."""

    def __init__(self, ctx, **opts):
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        self.base = self.ctx.options()
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.opts:
            self.ctx.set_option(k, -1)
        assert self.ctx.options() == self.base
        return False
