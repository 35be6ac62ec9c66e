"""basic_iterative_solvers_amd -- MI355X (gfx950) implementation of the SpMV +
preconditioner-apply + BLAS-1 hot path of DanecLacey/basic_iterative_solvers.

The product is the C-ABI library `lib/libbis_hip.so` (include/bis_hip.h),
hand-written HIP for gfx950, plus the C++ host layer under `host/` that mirrors
the reference's operator surface.  This Python module is only a thin ctypes
binding used by the tests, `bench.py` and `__graft_entry__.py`; it adds no
compute path of its own and there is no CPU fallback: without a usable gfx950
device `Context()` raises.
"""
import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "lib", "libbis_hip.so")

PC = dict(none=0, j=1, gs=2, bgs=3, sgs=4, **{"2st": 5, "s2st": 6, "ilu0": 7, "ilu0it": 8, "fsai": 9, "mg": 10, "bj": 11})

_lib = None


class BisError(RuntimeError):
    pass


def load_library():
    """dlopen the in-tree C-ABI library (never builds, never falls back)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BisError(
                f"{LIB_PATH} is missing: build it with "
                "`python -m basic_iterative_solvers_amd.build` (hipcc, gfx950)")
        _lib = C.CDLL(LIB_PATH)
        _lib.bis_last_error.restype = C.c_char_p
        _lib.bis_ctx_stream.restype = C.c_void_p
        _lib.bis_mat_sweep_kernel.restype = C.c_char_p
        _lib.bis_mat_spmv_kernel.restype = C.c_char_p
        _lib.bis_mat_ilu0_kernel.restype = C.c_char_p
        _lib.bis_itrsv_kernel.restype = C.c_char_p
        _lib.bis_mat_spmm_kernel.restype = C.c_char_p
        _lib.bis_mat_sweepm_kernel.restype = C.c_char_p
        _lib.bis_mat_fsai_kernel.restype = C.c_char_p
        _lib.bis_mat_iluk_kernel.restype = C.c_char_p
        _lib.bis_spgemm_kernel.restype = C.c_char_p
        _lib.bis_mg_operand.restype = C.c_void_p
        _lib.bis_mg_level_prolongator.restype = C.c_void_p
        _lib.bis_mg_level_restrictor.restype = C.c_void_p
        _lib.bis_mg_level_matrix.restype = C.c_void_p
        _lib.bis_bj_operand.restype = C.c_void_p
    return _lib


def _i64(v):
    return C.c_int64(int(v))


def iluk_limits():
    """(max_level, max_visit) of Context.iluk (bis_iluk_limits): the largest level-of-fill, and the vertices the symbolic
    search of one row may visit."""
    ml, mv = C.c_int(), C.c_int()
    load_library().bis_iluk_limits(C.byref(ml), C.byref(mv))
    return ml.value, mv.value


def spgemm_limits():
    """dict(wave_cap, row_cap, row_cap_max, batch) of Context.spgemm (bis_spgemm_limits): the products per row up to which
    one wave / the row path takes a row (row_cap is the default of option spgemm_row_cap, row_cap_max its largest
    value), and the default of option spgemm_batch."""
    w, r, m, b = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    load_library().bis_spgemm_limits(C.byref(w), C.byref(r), C.byref(m), C.byref(b))
    return dict(wave_cap=w.value, row_cap=r.value, row_cap_max=m.value, batch=b.value)


class Context:
    """bis_ctx: one device + stream.  Raises if no gfx950 device is usable."""

    def __init__(self, device=0, stream=None):
        self.lib = load_library()
        self.h = C.c_void_p()
        st = self.lib.bis_ctx_create(C.c_int(device), C.c_void_p(stream), C.byref(self.h))
        if st != 0:
            raise BisError(f"bis_ctx_create failed (status {st}): no usable gfx950 device; "
                           "this package has no CPU fallback")

    def check(self, st):
        if st != 0:
            raise BisError(f"status {st}: {self.lib.bis_last_error(self.h).decode()}")

    def close(self):
        if self.h:
            self.lib.bis_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def sync(self):
        self.check(self.lib.bis_sync(self.h))

    def set_option(self, name, value):
        if self.lib.bis_set_option(name.encode(), C.c_int(int(value))) != 0:
            raise BisError(f"bis_set_option: unknown option {name}")

    def options(self):
        """The options in effect (bis_options_describe): every option not at its default + the BIS_* variables found in the
        environment at first use -- for bench / test records."""
        import json
        n = self.lib.bis_options_describe(None, C.c_int(0))
        buf = C.create_string_buffer(n + 1)
        self.lib.bis_options_describe(buf, C.c_int(n + 1))
        return json.loads(buf.value.decode())

    def device_info(self):
        arch = C.create_string_buffer(64)
        n_cus = C.c_int()
        hbm = C.c_int64()
        self.check(self.lib.bis_device_info(self.h, arch, C.c_size_t(64), C.byref(n_cus),
                                            C.byref(hbm)))
        return dict(arch=arch.value.decode(), n_cus=n_cus.value, hbm_bytes=hbm.value)

    # ---- vectors -----------------------------------------------------------
    def alloc(self, n):
        p = C.c_void_p()
        self.check(self.lib.bis_vec_alloc(self.h, _i64(n), C.byref(p)))
        return Vec(self, p.value, int(n), True)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        v = self.alloc(arr.size)
        self.check(self.lib.bis_vec_upload(self.h, C.c_void_p(v.ptr), arr.ctypes, _i64(arr.size)))
        return v

    # ---- matrices ----------------------------------------------------------
    def matrix(self, crs):
        """Upload a host CRS (object with n_rows, n_cols, row_ptr(int64), col, val)."""
        h = C.c_void_p()
        rp = np.ascontiguousarray(crs.row_ptr, dtype=np.int64)
        col = np.ascontiguousarray(crs.col, dtype=np.int32)
        val = np.ascontiguousarray(crs.val, dtype=np.float64)
        nnz = int(rp[-1]) if len(rp) else 0
        if nnz < 2 ** 31 - 16:
            rp32 = rp.astype(np.int32)
            st = self.lib.bis_mat_create(self.h, _i64(crs.n_rows), _i64(crs.n_cols), _i64(nnz),
                                         rp32.ctypes, col.ctypes, val.ctypes, C.byref(h))
        else:
            st = self.lib.bis_mat_create64(self.h, _i64(crs.n_rows), _i64(crs.n_cols), _i64(nnz),
                                           rp.ctypes, col.ctypes, val.ctypes, C.byref(h))
        self.check(st)
        return Mat(self, h)

    def gen_hpcg(self, nx, ny=None, nz=None, row0=0, row1=None):
        ny = nx if ny is None else ny
        nz = nx if nz is None else nz
        row1 = nx * ny * nz if row1 is None else row1
        h = C.c_void_p()
        self.check(self.lib.bis_mat_gen_hpcg(self.h, _i64(nx), _i64(ny), _i64(nz), _i64(row0),
                                             _i64(row1), C.byref(h)))
        return Mat(self, h)

    def gen_anderson(self, L, t=1.0, W=5.0, shift=0.0, seed=1, row0=0, row1=None):
        row1 = L ** 3 if row1 is None else row1
        h = C.c_void_p()
        self.check(self.lib.bis_mat_gen_anderson(self.h, _i64(L), C.c_double(t), C.c_double(W),
                                                 C.c_double(shift), C.c_uint64(seed),
                                                 _i64(row0), _i64(row1), C.byref(h)))
        return Mat(self, h)

    def gen_fem(self, nx, ny=None, nz=None, keep=85, seed=1, row0=0, row1=None):
        ny = nx if ny is None else ny
        nz = nx if nz is None else nz
        row1 = 3 * nx * ny * nz if row1 is None else row1
        h = C.c_void_p()
        self.check(self.lib.bis_mat_gen_fem(self.h, _i64(nx), _i64(ny), _i64(nz), C.c_int(keep),
                                            C.c_uint64(seed), _i64(row0), _i64(row1), C.byref(h)))
        return Mat(self, h)

    def gen_unstr(self, nx, ny=None, nz=None, keep=85, seed=1):
        """fem: under a seeded random symmetric row permutation, ascending columns, no grid hint (config 5's unstructured input)."""
        ny = nx if ny is None else ny
        nz = nx if nz is None else nz
        h = C.c_void_p()
        self.check(self.lib.bis_mat_gen_unstr(self.h, _i64(nx), _i64(ny), _i64(nz), C.c_int(keep), C.c_uint64(seed),
                                              None, C.byref(h)))
        return Mat(self, h)

    def multicolour(self, A):
        """B = P A P^T grouped by colour; returns (B, perm[new]=old as numpy int32, n_colours)."""
        n = A.n_rows
        store = self.alloc((n + 1) // 2 + 1)
        h, nc = C.c_void_p(), C.c_int()
        self.check(self.lib.bis_mat_multicolour(self.h, A.h, C.byref(h), C.c_void_p(store.ptr), C.byref(nc)))
        perm = store.to_host().view(np.int32)[:n].copy()
        store.free()
        return Mat(self, h), perm, nc.value

    def bfs_order(self, A, rcm=False):
        """Breadth-first / reverse Cuthill-McKee permutation on the device (perm[new] = old, numpy int32)."""
        n = A.n_rows
        store = self.alloc((n + 1) // 2 + 1)
        self.check(self.lib.bis_mat_bfs_order(self.h, A.h, C.c_int(int(rcm)), C.c_void_p(store.ptr)))
        perm = store.to_host().view(np.int32)[:n].copy()
        store.free()
        return perm

    def permute(self, A, perm):
        """B = P A P^T on the device for perm[new] = old."""
        n = len(perm)
        raw = np.zeros((n + 1) // 2 + 1)
        raw.view(np.int32)[:n] = np.asarray(perm, dtype=np.int32)
        store = self.upload(raw)
        h = C.c_void_p()
        try:
            self.check(self.lib.bis_mat_permute(self.h, A.h, C.c_void_p(store.ptr), C.byref(h)))
        finally:
            store.free()
        return Mat(self, h)

    def scale_sym(self, A, init=0.0):
        """-scale on the device: returns the scale vector s (Vec); A's values are scaled in place."""
        s = self.alloc(A.n_rows)
        self.init_vector(s, init)
        self.check(self.lib.bis_mat_scale_sym(self.h, A.h, C.c_void_p(s.ptr)))
        return s

    def gather(self, out, vec, perm):
        """out[i] = vec[perm[i]] on the device (perm: numpy int32, uploaded for the call)."""
        n = len(perm)
        raw = np.zeros((n + 1) // 2 + 1)
        raw.view(np.int32)[:n] = np.asarray(perm, dtype=np.int32)
        store = self.upload(raw)
        self.check(self.lib.bis_vec_gather(self.h, C.c_void_p(out.ptr), C.c_void_p(vec.ptr), C.c_void_p(store.ptr), _i64(n)))
        self.sync()
        store.free()

    def scatter(self, out, vec, perm):
        """out[perm[i]] = vec[i] on the device (perm: numpy int32, uploaded for the call)."""
        n = len(perm)
        raw = np.zeros((n + 1) // 2 + 1)
        raw.view(np.int32)[:n] = np.asarray(perm, dtype=np.int32)
        store = self.upload(raw)
        self.check(self.lib.bis_vec_scatter(self.h, C.c_void_p(out.ptr), C.c_void_p(vec.ptr), C.c_void_p(store.ptr), _i64(n)))
        self.sync()
        store.free()

    def tune_placement(self, A, max_trials=6):
        """Keep the fastest of up to max_trials re-allocations of A's streamed arrays; returns (first_ms, best_ms)."""
        f, b = C.c_double(), C.c_double()
        self.check(self.lib.bis_mat_tune_placement(self.h, A.h, C.c_int(max_trials), C.byref(f), C.byref(b)))
        return f.value, b.value

    def split_strict(self, A):
        n = A.n_rows
        D, Dinv = self.alloc(n), self.alloc(n)
        hl, hu = C.c_void_p(), C.c_void_p()
        self.check(self.lib.bis_mat_split_strict(self.h, A.h, C.byref(hl), C.byref(hu),
                                                 C.c_void_p(D.ptr), C.c_void_p(Dinv.ptr)))
        return Mat(self, hl), Mat(self, hu), D, Dinv

    def mat_diag(self, A, row_offset=0):
        """(D, 1/D) of a row block with global column indices (bis_mat_diag)."""
        D, Dinv = self.alloc(A.n_rows), self.alloc(A.n_rows)
        self.check(self.lib.bis_mat_diag(self.h, A.h, _i64(row_offset), C.c_void_p(D.ptr), C.c_void_p(Dinv.ptr)))
        return D, Dinv

    def diag_block(self, A, row_offset=0):
        """Square diagonal block of a row block with global columns (bis_mat_diag_block)."""
        h = C.c_void_p()
        self.check(self.lib.bis_mat_diag_block(self.h, A.h, _i64(row_offset), C.byref(h)))
        return Mat(self, h)

    def ilu0(self, A, pivot_tol=1e-8, pivot_repl=1e-4):
        n = A.n_rows
        L_D, U_D = self.alloc(n), self.alloc(n)
        hl, hu = C.c_void_p(), C.c_void_p()
        self.check(self.lib.bis_mat_ilu0(self.h, A.h, C.c_double(pivot_tol), C.c_double(pivot_repl),
                                         C.byref(hl), C.byref(hu), C.c_void_p(L_D.ptr),
                                         C.c_void_p(U_D.ptr)))
        return Mat(self, hl), L_D, Mat(self, hu), U_D

    def iluk(self, A, level, pivot_tol=1e-8, pivot_repl=1e-4):
        """(Ls, L_D, Us, U_D, n_fill): ILU(level) with level-of-fill (bis_mat_iluk); level 0 is ilu0.  The factors go to
        preconditioners "ilu0" / "ilu0it" like those of ilu0; n_fill counts the positions added to A's pattern."""
        n = A.n_rows
        L_D, U_D = self.alloc(n), self.alloc(n)
        hl, hu, nf = C.c_void_p(), C.c_void_p(), C.c_int64()
        self.check(self.lib.bis_mat_iluk(self.h, A.h, C.c_int(int(level)), C.c_double(pivot_tol), C.c_double(pivot_repl),
                                         C.byref(hl), C.byref(hu), C.c_void_p(L_D.ptr), C.c_void_p(U_D.ptr), C.byref(nf)))
        return Mat(self, hl), L_D, Mat(self, hu), U_D, nf.value

    def iluk_symbolic(self, A, level):
        """(P, n_fill): A padded with explicit +0.0 at the fill positions of level <= `level` (bis_mat_iluk_symbolic)."""
        h, nf = C.c_void_p(), C.c_int64()
        self.check(self.lib.bis_mat_iluk_symbolic(self.h, A.h, C.c_int(int(level)), C.byref(h), C.byref(nf)))
        return Mat(self, h), nf.value

    def fsai(self, A):
        """(G, Gt, n_fallback): the factorized sparse approximate inverse of A on the pattern of tril(A), M^-1 = Gt G
        (bis_mat_fsai); preconditioner "fsai" takes Ls=G, Us=Gt.  n_fallback counts the rows that became e_i / sqrt(|a_ii|)."""
        hg, hgt, nf = C.c_void_p(), C.c_void_p(), C.c_int64()
        self.check(self.lib.bis_mat_fsai(self.h, A.h, C.byref(hg), C.byref(hgt), C.byref(nf)))
        return Mat(self, hg), Mat(self, hgt), nf.value

    def spgemm(self, A, B):
        """C = A B as a new Mat (bis_spgemm); Mat.spgemm_kernel() names the path that made it."""
        h = C.c_void_p()
        self.check(self.lib.bis_spgemm(self.h, A.h, B.h, C.byref(h)))
        return Mat(self, h)

    def mg(self, A, cycle=None, cycle_levels=0, smooth=False, prolong_omega=0.0, smoother=None, degree=2, ratio=None, est_steps=10,
           safety=1.1, **params):
        """The aggregation multigrid hierarchy of A (bis_mg_create): an MG object.  Parameters: max_levels, coarse_limit,
        coarsening (0 / "auto", 1 / "grid", 2 / "mis"), nu, coarse_sweeps, omega, coarse_scale.  `cycle` (0 / "v", 1 / "w",
        2 / "k", 3 / "kgcr") and `cycle_levels` go to MG.set_cycle after creation; without `cycle` the hierarchy stays V.
        `smooth` builds smoothed aggregation (bis_mg_create_smoothed) with the factor `prolong_omega` (0: 4/3).
        `smoother` (0 / "jacobi", 1 / "cheb") with `degree`, `ratio`, `est_steps`, `safety` goes to MG.set_smoother; without it
        the hierarchy relaxes with its weights, as before.  Preconditioner "mg" takes Ls=MG.operand."""
        m = MG(self, A, smooth=smooth, prolong_omega=prolong_omega, **params)
        try:
            if cycle is not None:
                m.set_cycle(cycle, cycle_levels)
            if smoother is not None:
                m.set_smoother(smoother, degree=degree, ratio=ratio, est_steps=est_steps, safety=safety)
        except Exception:
            m.free()
            raise
        return m

    def bjacobi(self, A, block_size=None, block_ptr=None, symmetrize=False):
        """The block-Jacobi handle of A (bis_bj_create): a BJ object.  Uniform blocks of `block_size` (1..32) consecutive rows,
        or the blocks of `block_ptr` (n_blocks + 1 ascending row indices from 0 to n); `symmetrize` makes every inverse block
        equal its transpose bit for bit (for CG and MINRES).  Preconditioner "bj" takes Ls=BJ.operand."""
        return BJ(self, A, block_size, block_ptr, symmetrize)

    # ---- kernels (kernels.hpp names) ---------------------------------------
    def spmv(self, A, x, y):
        self.check(self.lib.bis_spmv(self.h, A.h, C.c_void_p(x.ptr), C.c_void_p(y.ptr)))

    def spmm(self, A, X, Y, k):
        """Y = A X for k interleaved vectors (X[c*k + j], Y[r*k + j]; bis_spmm)."""
        self.check(self.lib.bis_spmm(self.h, A.h, C.c_void_p(X.ptr), C.c_void_p(Y.ptr), C.c_int(int(k))))

    def mvec_set_col(self, X, n, k, j, v):
        """Column j of the interleaved n x k block X = the plain vector v (bis_mvec_set_col)."""
        self.check(self.lib.bis_mvec_set_col(self.h, C.c_void_p(X.ptr), _i64(n), C.c_int(int(k)), C.c_int(int(j)), C.c_void_p(v.ptr)))

    def mvec_get_col(self, v, X, n, k, j):
        """The plain vector v = column j of the interleaved n x k block X (bis_mvec_get_col)."""
        self.check(self.lib.bis_mvec_get_col(self.h, C.c_void_p(v.ptr), C.c_void_p(X.ptr), _i64(n), C.c_int(int(k)), C.c_int(int(j))))

    def sptrsv(self, Ls, x, D, b):
        self.check(self.lib.bis_sptrsv(self.h, Ls.h, C.c_void_p(x.ptr), C.c_void_p(D.ptr),
                                       C.c_void_p(b.ptr)))

    def bsptrsv(self, Us, x, D, b):
        self.check(self.lib.bis_bsptrsv(self.h, Us.h, C.c_void_p(x.ptr), C.c_void_p(D.ptr),
                                        C.c_void_p(b.ptr)))

    def sptrsm(self, Ls, X, D, B, k):
        """X_j = (D + Ls)^-1 B_j for k interleaved vectors (bis_sptrsm); X may alias B."""
        self.check(self.lib.bis_sptrsm(self.h, Ls.h, C.c_void_p(X.ptr), C.c_void_p(D.ptr), C.c_void_p(B.ptr), C.c_int(int(k))))

    def bsptrsm(self, Us, X, D, B, k):
        """X_j = (D + Us)^-1 B_j for k interleaved vectors (bis_bsptrsm); X may alias B."""
        self.check(self.lib.bis_bsptrsm(self.h, Us.h, C.c_void_p(X.ptr), C.c_void_p(D.ptr), C.c_void_p(B.ptr), C.c_int(int(k))))

    def mitrsv(self, T, D_inv, B, X, work, n_sweeps, k):
        """bis_itrsv on every column of the interleaved n x k block B (bis_mitrsv); work: n x k entries of scratch."""
        self.check(self.lib.bis_mitrsv(self.h, T.h, C.c_void_p(D_inv.ptr), C.c_void_p(B.ptr), C.c_void_p(X.ptr),
                                       C.c_void_p(work.ptr) if work is not None else C.c_void_p(), C.c_int(int(n_sweeps)), C.c_int(int(k))))

    def mvec_div_diag(self, R, A, D, n, k):
        """R[i,j] = A[i,j] / (1.0 * D[i]) on interleaved n x k blocks (bis_mvec_div_diag)."""
        self.check(self.lib.bis_mvec_div_diag(self.h, C.c_void_p(R.ptr), C.c_void_p(A.ptr), C.c_void_p(D.ptr), _i64(n), C.c_int(int(k))))

    def mvec_mul_diag(self, R, A, D, n, k):
        """R[i,j] = A[i,j] * 1.0 * D[i] on interleaved n x k blocks (bis_mvec_mul_diag)."""
        self.check(self.lib.bis_mvec_mul_diag(self.h, C.c_void_p(R.ptr), C.c_void_p(A.ptr), C.c_void_p(D.ptr), _i64(n), C.c_int(int(k))))

    def itrsv(self, T, D_inv, b, x, work, n_sweeps):
        """x ~ (D + T)^-1 b by n_sweeps Jacobi-Richardson steps on the strict triangle T (bis_itrsv); work: n entries of scratch."""
        self.check(self.lib.bis_itrsv(self.h, T.h, C.c_void_p(D_inv.ptr), C.c_void_p(b.ptr), C.c_void_p(x.ptr),
                                      C.c_void_p(work.ptr) if work is not None else C.c_void_p(), C.c_int(int(n_sweeps))))

    def _ew3(self, fn, r, a, b, scale, n=None):
        n = r.n if n is None else n
        self.check(fn(self.h, C.c_void_p(r.ptr), C.c_void_p(a.ptr), C.c_void_p(b.ptr), _i64(n),
                      C.c_double(scale)))

    def subtract_vectors(self, r, a, b, scale=1.0, n=None):
        self._ew3(self.lib.bis_subtract_vectors, r, a, b, scale, n)

    def sum_vectors(self, r, a, b, scale=1.0, n=None):
        self._ew3(self.lib.bis_sum_vectors, r, a, b, scale, n)

    def elemwise_mult_vectors(self, r, a, b, scale=1.0, n=None):
        self._ew3(self.lib.bis_elemwise_mult_vectors, r, a, b, scale, n)

    def elemwise_div_vectors(self, r, a, b, scale=1.0, n=None):
        self._ew3(self.lib.bis_elemwise_div_vectors, r, a, b, scale, n)

    def compute_residual(self, A, x, b, res, tmp):
        self.check(self.lib.bis_compute_residual(self.h, A.h, C.c_void_p(x.ptr), C.c_void_p(b.ptr),
                                                 C.c_void_p(res.ptr), C.c_void_p(tmp.ptr)))

    def dot(self, a, b, n=None):
        out = C.c_double()
        self.check(self.lib.bis_dot(self.h, C.c_void_p(a.ptr), C.c_void_p(b.ptr),
                                    _i64(a.n if n is None else n), C.byref(out)))
        return out.value

    def euclidean_vec_norm(self, v, n=None):
        out = C.c_double()
        self.check(self.lib.bis_euclidean_vec_norm(self.h, C.c_void_p(v.ptr),
                                                   _i64(v.n if n is None else n), C.byref(out)))
        return out.value

    def scale(self, r, v, scalar, n=None):
        self.check(self.lib.bis_scale(self.h, C.c_void_p(r.ptr), C.c_void_p(v.ptr),
                                      C.c_double(scalar), _i64(r.n if n is None else n)))

    def init_vector(self, v, val, n=None):
        self.check(self.lib.bis_init_vector(self.h, C.c_void_p(v.ptr), C.c_double(val),
                                            _i64(v.n if n is None else n)))

    def copy_vector(self, out, inp, n=None):
        self.check(self.lib.bis_copy_vector(self.h, C.c_void_p(out.ptr), C.c_void_p(inp.ptr),
                                            _i64(out.n if n is None else n)))

    def normalize_x(self, x_new, x_old, D, b):
        self.check(self.lib.bis_normalize_x(self.h, C.c_void_p(x_new.ptr), C.c_void_p(x_old.ptr),
                                            C.c_void_p(D.ptr), C.c_void_p(b.ptr), _i64(x_new.n)))

    def multi_axpy(self, V, ldv, y_host, n_vec, out, n):
        y = np.ascontiguousarray(y_host, dtype=np.float64)
        self.check(self.lib.bis_multi_axpy(self.h, C.c_void_p(V.ptr), _i64(ldv), y.ctypes,
                                           C.c_int(n_vec), C.c_void_p(out.ptr), _i64(n)))

    def apply_preconditioner(self, pc, n, Ls, Us, A_D, A_D_inv, L_D, U_D, out, inp, tmp, work,
                             outer=1, inner=0):
        def p(v):
            return C.c_void_p(v.ptr) if v is not None else C.c_void_p()
        self.check(self.lib.bis_apply_preconditioner(
            self.h, C.c_int(PC[pc] if isinstance(pc, str) else pc), _i64(n),
            Ls.h if Ls is not None else C.c_void_p(), Us.h if Us is not None else C.c_void_p(),
            p(A_D), p(A_D_inv), p(L_D), p(U_D), p(out), p(inp), p(tmp), p(work),
            C.c_int(outer), C.c_int(inner)))

    def mapply_preconditioner(self, pc, n, k, Ls, Us, A_D, A_D_inv, L_D, U_D, out, inp, tmp, work, outer=1, inner=0):
        """bis_apply_preconditioner on interleaved n x k blocks (bis_mapply_preconditioner)."""
        def p(v):
            return C.c_void_p(v.ptr) if v is not None else C.c_void_p()
        self.check(self.lib.bis_mapply_preconditioner(
            self.h, C.c_int(PC[pc] if isinstance(pc, str) else pc), _i64(n), C.c_int(int(k)),
            Ls.h if Ls is not None else C.c_void_p(), Us.h if Us is not None else C.c_void_p(),
            p(A_D), p(A_D_inv), p(L_D), p(U_D), p(out), p(inp), p(tmp), p(work),
            C.c_int(outer), C.c_int(inner)))

    # ---- fused CG ------------------------------------------------------------
    def cg(self, A, b, x, A_D=None):
        return CG(self, A, b, x, A_D)

    def mcg(self, A, B, X, k, A_D=None):
        return MCG(self, A, B, X, k, A_D)

    def mbicgstab(self, A, B, X, k):
        return MBiCGSTAB(self, A, B, X, k)

    def mgmres(self, A, B, X, k, restart=10):
        return MGMRES(self, A, B, X, k, restart)

    def fgmres(self, A, b, x, restart=10):
        return FGMRES(self, A, b, x, restart)

    def minres(self, A, b, x):
        return MINRES(self, A, b, x)

    def idr(self, A, b, x, s=4):
        return IDR(self, A, b, x, s)

    def lsmr(self, A, b, x, At=None, damp=0.0, col_scaling=None):
        return LSMR(self, A, b, x, At, damp, col_scaling)

    def eigs(self, A, k=4, which="SA", ncv=None, tol=1e-10, v0=None, n=None):
        return Eigs(self, A, k, which, ncv, tol, v0, n)

    def svds(self, A, k=4, which="LM", ncv=None, tol=1e-10, v0=None, At=None, shape=None):
        return SVDS(self, A, k, which, ncv, tol, v0, At, shape)

    # ---- measurement ---------------------------------------------------------
    def stat(self, kind, A, D, b, x, Ls=None, Us=None):
        return Stat(self, kind, A, D, b, x, Ls, Us)

    def profile(self, on):
        self.check(self.lib.bis_profile_enable(self.h, C.c_int(int(on))))

    def profile_read(self):
        n = C.c_int64()
        ms = C.c_double()
        self.check(self.lib.bis_profile_read(self.h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def profile_read_sweeps(self):
        """(sweeps, summed ms) of the bis_sptrsv / bis_bsptrsv calls made while profiling was on (HIP events on the library's stream)."""
        n = C.c_int64()
        ms = C.c_double()
        self.check(self.lib.bis_profile_read_sweeps(self.h, C.byref(n), C.byref(ms)))
        return n.value, ms.value


class Vec:
    """A device vector: raw `double*` + length (what the reference passes as
    `double *`).  `offset(k)` gives the pointer-arithmetic view `&v[k]`
    (gmres.hpp:169)."""

    def __init__(self, ctx, ptr, n, owner):
        self.ctx, self.ptr, self.n, self.owner = ctx, ptr, n, owner

    def offset(self, k, n=None):
        return Vec(self.ctx, self.ptr + 8 * int(k), self.n - int(k) if n is None else n, False)

    def to_host(self):
        out = np.empty(self.n, dtype=np.float64)
        self.ctx.check(self.ctx.lib.bis_vec_download(self.ctx.h, out.ctypes, C.c_void_p(self.ptr),
                                                     _i64(self.n)))
        return out

    def set(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        assert arr.size == self.n
        self.ctx.check(self.ctx.lib.bis_vec_upload(self.ctx.h, C.c_void_p(self.ptr), arr.ctypes,
                                                   _i64(self.n)))

    def free(self):
        if self.owner and self.ptr:
            self.ctx.lib.bis_vec_free(self.ctx.h, C.c_void_p(self.ptr))
            self.ptr = 0


class Mat:
    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h
        n_rows, n_cols, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        ctx.lib.bis_mat_info(h, C.byref(n_rows), C.byref(n_cols), C.byref(nnz))
        self.n_rows, self.n_cols, self.nnz = n_rows.value, n_cols.value, nnz.value

    @property
    def rp_width(self):
        return int(self.ctx.lib.bis_mat_rp_width(self.h))

    def spmv_stream_info(self):
        """(col_bytes, val_bytes, n_dict, form) of the SpMV's streams for this matrix (bis_mat_spmv_stream_info)."""
        c, v, d, f = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(self.ctx.lib.bis_mat_spmv_stream_info(self.ctx.h, self.h, C.byref(c), C.byref(v), C.byref(d), C.byref(f)))
        return c.value, v.value, d.value, f.value

    def spmv_streamed_bytes(self):
        """Bytes one SpMV launch moves at least with the matrix' current stream format (bis_mat_spmv_streamed_bytes)."""
        b = C.c_int64()
        self.ctx.check(self.ctx.lib.bis_mat_spmv_streamed_bytes(self.ctx.h, self.h, C.byref(b)))
        return b.value

    def debug_ptrs(self):
        """Device addresses (row_ptr, col, val) of the CRS arrays (bis_mat_debug_ptrs)."""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.ctx.check(self.ctx.lib.bis_mat_debug_ptrs(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def win8_tuning(self):
        """(re-allocations tried, kernel ms on the first allocation, kernel ms on the one kept) of the placement search the library
        made when it built the matrix' window + sliced-ELL stream (bis_mat_win8_tuning); zeros without one."""
        t, a, b = C.c_int(), C.c_double(), C.c_double()
        self.ctx.lib.bis_mat_win8_tuning(self.h, C.byref(t), C.byref(a), C.byref(b))
        return t.value, a.value, b.value

    def win8_layout(self):
        """(chunks, explicit chunks, slices, blocks, implied) of the matrix' window + sliced-ELL stream (bis_mat_win8_layout);
        zeros without one."""
        ch, ex, sl = C.c_int64(), C.c_int64(), C.c_int64()
        bl, im = C.c_int(), C.c_int()
        self.ctx.lib.bis_mat_win8_layout(self.h, C.byref(ch), C.byref(ex), C.byref(sl), C.byref(bl), C.byref(im))
        return ch.value, ex.value, sl.value, bl.value, bool(im.value)

    def colslab_info(self):
        """(K, one-pass ms, K-passes ms): the column slabs the SpMV of this matrix runs on (0: none) and the build-time trial's
        times (bis_mat_colslab_info)."""
        k, a, b = C.c_int(), C.c_double(), C.c_double()
        self.ctx.lib.bis_mat_colslab_info(self.h, C.byref(k), C.byref(a), C.byref(b))
        return k.value, a.value, b.value

    def sweep_kernel(self, backward=False):
        """Name of the kernel the last forward / backward sweep on this triangle ran (bis_mat_sweep_kernel)."""
        return self.ctx.lib.bis_mat_sweep_kernel(self.h, C.c_int(int(backward))).decode()

    def sweepm_kernel(self, backward=False):
        """What the last multi-vector forward / backward sweep on this triangle launched, with its instance (bis_mat_sweepm_kernel)."""
        return self.ctx.lib.bis_mat_sweepm_kernel(self.h, C.c_int(int(backward))).decode()

    def spmv_kernel(self, fused=False):
        """Name of the kernel (and template instance) the last plain / fused-dot SpMV of this matrix launched (bis_mat_spmv_kernel)."""
        return self.ctx.lib.bis_mat_spmv_kernel(self.h, C.c_int(int(fused))).decode()

    def spmm_kernel(self):
        """Name of the path and template instance the last bis_spmm on this matrix launched (bis_mat_spmm_kernel)."""
        return self.ctx.lib.bis_mat_spmm_kernel(self.h).decode()

    def spmm_streamed_bytes(self, k):
        """12 nnz + rp_width (n_rows + 1) + 8 k (n_cols + n_rows) (bis_mat_spmm_streamed_bytes)."""
        b = C.c_int64()
        if self.ctx.lib.bis_mat_spmm_streamed_bytes(self.h, C.c_int(int(k)), C.byref(b)) != 0:
            raise BisError("bis_mat_spmm_streamed_bytes: bad arguments")
        return b.value

    def ilu0_kernel(self):
        """Name of the elimination kernel that factorised this ILU(0) L factor (bis_mat_ilu0_kernel); "" for other matrices."""
        return self.ctx.lib.bis_mat_ilu0_kernel(self.h).decode()

    def iluk_kernel(self):
        """The symbolic search that made this ILU(k) pattern or L factor, e.g. "iluk_search_kernel RP=32 two searches"
        (bis_mat_iluk_kernel); "" for other matrices."""
        return self.ctx.lib.bis_mat_iluk_kernel(self.h).decode()

    def fsai_kernel(self):
        """The instance of fsai_rows_kernel that computed this FSAI factor G, e.g. "fsai_rows_kernel M=32 RP=32"
        (bis_mat_fsai_kernel); "" for other matrices."""
        return self.ctx.lib.bis_mat_fsai_kernel(self.h).decode()

    def itrsv_kernel(self):
        """Name of the path the last bis_itrsv step on this triangle took (bis_itrsv_kernel): "itrsv_fused_rowblock" or
        "itrsv spmv+epilogue form=F"."""
        return self.ctx.lib.bis_itrsv_kernel(self.h).decode()

    def spgemm_kernel(self):
        """The path(s) of bis_spgemm that made this product: "spgemm_row_kernel", "spgemm_sort_fallback" or both
        (bis_spgemm_kernel); "" for other matrices."""
        return self.ctx.lib.bis_spgemm_kernel(self.h).decode()

    def transpose(self):
        """A^T as a new Mat (bis_mat_transpose)."""
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.bis_mat_transpose(self.ctx.h, self.h, C.byref(h)))
        return Mat(self.ctx, h)

    def row_norms(self):
        """The 2-norms of the rows as a new Vec (bis_mat_row_norms); the column norms of A are A.transpose().row_norms()."""
        out = self.ctx.alloc(self.n_rows)
        self.ctx.check(self.ctx.lib.bis_mat_row_norms(self.ctx.h, self.h, C.c_void_p(out.ptr)))
        return out

    def round_f32(self):
        """Round every value to fp32 in place in the fp64 CRS array and flag the matrix fp32-exact (bis_mat_round_f32): its SpMV
        may then stream 4-byte values (form 8).  Returns the largest relative change of a value."""
        m = C.c_double()
        self.ctx.check(self.ctx.lib.bis_mat_round_f32(self.ctx.h, self.h, C.byref(m)))
        return m.value

    def grid_hint(self):
        """(nx, ny, nz, dof) of the structured-grid hint the matrix carries (bis_mat_grid_hint); zeros without one."""
        g = (C.c_int64 * 4)()
        self.ctx.check(self.ctx.lib.bis_mat_grid_hint(self.h, g))
        return tuple(g)

    def retune(self):
        """Rebuild everything derived from the CRS arrays (bis_mat_retune): required after writing values in place."""
        self.ctx.check(self.ctx.lib.bis_mat_retune(self.ctx.h, self.h))

    def set_grid_hint(self, nx, ny, nz, dof=1):
        self.ctx.check(self.ctx.lib.bis_mat_set_grid_hint(self.h, _i64(nx), _i64(ny), _i64(nz), C.c_int(dof)))

    def download(self):
        rp = np.zeros(self.n_rows + 1, dtype=np.int64)
        col = np.zeros(self.nnz, dtype=np.int32)
        val = np.zeros(self.nnz, dtype=np.float64)
        self.ctx.check(self.ctx.lib.bis_mat_download(self.ctx.h, self.h, rp.ctypes, col.ctypes,
                                                     val.ctypes))
        return rp, col, val

    def free(self):
        if self.h:
            self.ctx.lib.bis_mat_destroy(self.ctx.h, self.h)
            self.h = C.c_void_p()


class MGParams(C.Structure):
    """bis_mg_params."""
    _fields_ = [("max_levels", C.c_int), ("coarse_limit", C.c_int64), ("coarsening", C.c_int), ("nu", C.c_int),
                ("coarse_sweeps", C.c_int), ("omega", C.c_double), ("coarse_scale", C.c_double)]


class MGSmoother(C.Structure):
    """bis_mg_smoother."""
    _fields_ = [("kind", C.c_int), ("degree", C.c_int), ("ratio", C.c_double), ("est_steps", C.c_int), ("safety", C.c_double)]


class MG:
    """bis_mg: an aggregation multigrid hierarchy of A; one cycle of it (V unless set_cycle chose W or K) is the
    preconditioner "mg" (pass `.operand` as Ls)."""

    COARSENING = dict(auto=0, grid=1, mis=2)
    CYCLE = dict(v=0, w=1, k=2, kgcr=3)
    SMOOTHER = dict(jacobi=0, cheb=1)
    # lambda_max / lambda_min of the Chebyshev smoother: the fewest CG iterations in total over HPCG 16^3 and 32^3 and the
    # unstructured 8^3 input, plain and smoothed, degree 2 and 3, among 4, 10, 20 and 30 (docs/EXPERIMENTS.md)
    DEFAULT_RATIO = 4.0

    def __init__(self, ctx, A, max_levels=10, coarse_limit=256, coarsening=0, nu=1, coarse_sweeps=4, omega=0.0, coarse_scale=1.0,
                 smooth=False, prolong_omega=0.0):
        self.ctx, self._keep = ctx, A
        self.h = C.c_void_p()
        self.smoothed = bool(smooth)
        p = MGParams(int(max_levels), int(coarse_limit), int(self.COARSENING.get(coarsening, coarsening)), int(nu),
                     int(coarse_sweeps), float(omega), float(coarse_scale))
        if self.smoothed:
            ctx.check(ctx.lib.bis_mg_create_smoothed(ctx.h, A.h, C.byref(p), C.c_double(float(prolong_omega)), C.byref(self.h)))
        else:
            if prolong_omega:
                raise BisError("MG: prolong_omega needs smooth=True")
            ctx.check(ctx.lib.bis_mg_create(ctx.h, A.h, C.byref(p), C.byref(self.h)))
        n = C.c_int()
        rows, nnz, kinds = (C.c_int64 * 16)(), (C.c_int64 * 16)(), (C.c_int * 16)()
        ctx.lib.bis_mg_info(self.h, C.byref(n), rows, nnz, kinds)
        self.levels = n.value
        self.rows, self.nnz, self.kinds = list(rows[:n.value]), list(nnz[:n.value]), list(kinds[:n.value])
        self.operand = Mat(ctx, C.c_void_p(ctx.lib.bis_mg_operand(self.h)))

    def level_matrix(self, l):
        """Level l's matrix as a Mat the hierarchy owns (level 0: A)."""
        h = self.ctx.lib.bis_mg_level_matrix(self.h, C.c_int(int(l)))
        if not h:
            raise BisError(f"MG.level_matrix: no level {l}")
        return Mat(self.ctx, C.c_void_p(h))

    def prolongator(self, l):
        """P of the transition from level l as a Mat the hierarchy owns (bis_mg_level_prolongator); None on the coarsest
        level and on a hierarchy without smoothed prolongators."""
        h = self.ctx.lib.bis_mg_level_prolongator(self.h, C.c_int(int(l)))
        return Mat(self.ctx, C.c_void_p(h)) if h else None

    def restrictor(self, l):
        """R = P^T of the transition from level l, like prolongator (bis_mg_level_restrictor)."""
        h = self.ctx.lib.bis_mg_level_restrictor(self.h, C.c_int(int(l)))
        return Mat(self.ctx, C.c_void_p(h)) if h else None

    def prolong_omega(self, l):
        """omega_l of the transition from level l (bis_mg_level_prolong_omega); None where there is no prolongator."""
        w = C.c_double()
        return w.value if self.ctx.lib.bis_mg_level_prolong_omega(self.h, C.c_int(int(l)), C.byref(w)) == 0 else None

    def aggregates(self, l):
        """agg[i] of every row of level l (numpy int32); the coarsest level has none."""
        out = np.zeros(self.rows[l], dtype=np.int32)
        self.ctx.check(self.ctx.lib.bis_mg_level_aggregates(self.ctx.h, self.h, C.c_int(int(l)), out.ctypes))
        return out

    def weights(self, l):
        """The smoother weights w of level l (numpy float64)."""
        out = np.zeros(self.rows[l], dtype=np.float64)
        self.ctx.check(self.ctx.lib.bis_mg_level_weights(self.ctx.h, self.h, C.c_int(int(l)), out.ctypes))
        return out

    def set_cycle(self, cycle, levels=0):
        """The cycle of this hierarchy (bis_mg_set_cycle; blocking): 0 / "v", 1 / "w", 2 / "k" (conjugate K-cycle, for SPD
        A under CG), 3 / "kgcr" (GCR K-cycle, any A) on the first `levels` transitions (0: all but the last)."""
        if isinstance(cycle, str):
            if cycle not in self.CYCLE:
                raise BisError(f"MG.set_cycle: cycle {cycle!r} is none of {sorted(self.CYCLE)}")
            cycle = self.CYCLE[cycle]
        self.ctx.check(self.ctx.lib.bis_mg_set_cycle(self.ctx.h, self.h, C.c_int(int(cycle)), C.c_int(int(levels))))

    @property
    def cycle(self):
        """(cycle, cycle_levels) as set (bis_mg_cycle)."""
        c, k = C.c_int(), C.c_int()
        self.ctx.check(self.ctx.lib.bis_mg_cycle(self.h, C.byref(c), C.byref(k)))
        return c.value, k.value

    def set_smoother(self, kind, degree=2, ratio=None, est_steps=10, safety=1.1):
        """The smoother of this hierarchy (bis_mg_set_smoother; blocking): 0 / "jacobi", or 1 / "cheb": one Chebyshev
        polynomial of `degree` (1..8) in W A per sweep, built for [lambda_max / ratio, lambda_max] (ratio None:
        DEFAULT_RATIO), lambda_max from the row-sum bound, tightened by `est_steps` (0..100) steps of a power iteration
        times `safety`."""
        if isinstance(kind, str):
            if kind not in self.SMOOTHER:
                raise BisError(f"MG.set_smoother: kind {kind!r} is none of {sorted(self.SMOOTHER)}")
            kind = self.SMOOTHER[kind]
        s = MGSmoother(int(kind), int(degree), float(self.DEFAULT_RATIO if ratio is None else ratio), int(est_steps), float(safety))
        self.ctx.check(self.ctx.lib.bis_mg_set_smoother(self.ctx.h, self.h, C.byref(s)))

    def smoother(self):
        """dict(kind, degree, ratio, est_steps, safety) as set (bis_mg_smoother_info); a Jacobi hierarchy reports zeros."""
        s = MGSmoother()
        self.ctx.check(self.ctx.lib.bis_mg_smoother_info(self.h, C.byref(s)))
        return dict(kind=s.kind, degree=s.degree, ratio=s.ratio, est_steps=s.est_steps, safety=s.safety)

    def spectrum(self, l):
        """dict(bound, estimate, lambda_max, lambda_min) of level l under the Chebyshev smoother (bis_mg_level_spectrum);
        None on a Jacobi hierarchy and outside the hierarchy."""
        v = [C.c_double() for _ in range(4)]
        if self.ctx.lib.bis_mg_level_spectrum(self.h, C.c_int(int(l)), *[C.byref(x) for x in v]) != 0:
            return None
        return dict(zip(("bound", "estimate", "lambda_max", "lambda_min"), (x.value for x in v)))

    def cheb_coeffs(self, l):
        """(c1, c2) of level l, numpy arrays of `degree` (bis_mg_level_cheb_coeffs); None where spectrum is."""
        k = self.smoother()["degree"]
        c1, c2 = np.zeros(max(k, 1)), np.zeros(max(k, 1))
        if self.ctx.lib.bis_mg_level_cheb_coeffs(self.h, C.c_int(int(l)), c1.ctypes, c2.ctypes) != 0:
            return None
        return c1[:k], c2[:k]

    def apply(self, out, inp):
        """out = M^-1 inp: one cycle (bis_mg_apply); out may alias inp."""
        self.ctx.check(self.ctx.lib.bis_mg_apply(self.ctx.h, self.h, C.c_void_p(out.ptr), C.c_void_p(inp.ptr)))

    def free(self):
        if self.h:
            self.ctx.lib.bis_mg_destroy(self.ctx.h, self.h)
            self.h = C.c_void_p()


class BJParams(C.Structure):
    """bis_bj_params."""
    _fields_ = [("block_size", C.c_int), ("block_ptr", C.POINTER(C.c_int32)), ("n_blocks", C.c_int64), ("symmetrize", C.c_int)]


class BJ:
    """bis_bj: the inverted dense diagonal blocks of A; their block-diagonal product is the preconditioner "bj" (pass
    `.operand` as Ls, or the object itself as the type).  A is not kept by the library."""

    def __init__(self, ctx, A, block_size=None, block_ptr=None, symmetrize=False):
        self.ctx = ctx
        self.h = C.c_void_p()
        if block_ptr is not None:
            bp = np.ascontiguousarray(block_ptr, dtype=np.int32)
            p = BJParams(0 if block_size is None else int(block_size), bp.ctypes.data_as(C.POINTER(C.c_int32)), len(bp) - 1,
                         int(bool(symmetrize)))
        else:
            if block_size is None:
                raise BisError("Context.bjacobi: give block_size or block_ptr")
            p = BJParams(int(block_size), None, 0, int(bool(symmetrize)))
        ctx.check(ctx.lib.bis_bj_create(ctx.h, A.h, C.byref(p), C.byref(self.h)))
        self.n_blocks, self.max_block, self.value_count = self.info()
        self.operand = Mat(ctx, C.c_void_p(ctx.lib.bis_bj_operand(self.h)))

    def info(self):
        """(n_blocks, rows of the largest block, stored values = the sum of the squared block sizes) (bis_bj_info)."""
        nb, mb, vc = C.c_int64(), C.c_int(), C.c_int64()
        self.ctx.lib.bis_bj_info(self.h, C.byref(nb), C.byref(mb), C.byref(vc))
        return nb.value, mb.value, vc.value

    def blocks(self):
        """(values, offsets): inverse block b row-major at values[offsets[b]:offsets[b + 1]] (bis_bj_blocks)."""
        vals = np.zeros(self.value_count, dtype=np.float64)
        offs = np.zeros(self.n_blocks + 1, dtype=np.int64)
        self.ctx.check(self.ctx.lib.bis_bj_blocks(self.ctx.h, self.h, vals.ctypes, offs.ctypes))
        return vals, offs

    def apply(self, out, inp):
        """out = M^-1 inp (bis_bj_apply); out may alias inp."""
        self.ctx.check(self.ctx.lib.bis_bj_apply(self.ctx.h, self.h, C.c_void_p(out.ptr), C.c_void_p(inp.ptr)))

    def mapply(self, out, inp, k):
        """The same on k interleaved columns (bis_bj_mapply); out may alias inp."""
        self.ctx.check(self.ctx.lib.bis_bj_mapply(self.ctx.h, self.h, C.c_void_p(out.ptr), C.c_void_p(inp.ptr), C.c_int(int(k))))

    def free(self):
        if self.h:
            self.ctx.lib.bis_bj_destroy(self.ctx.h, self.h)
            self.h = C.c_void_p()


def _handle_pc(pc, Ls):
    """set_preconditioner's first argument may be an MG or a BJ object: its type with its operand as Ls."""
    if isinstance(pc, MG):
        return "mg", pc.operand
    if isinstance(pc, BJ):
        return "bj", pc.operand
    return pc, Ls


class _Solver:
    """What the solver handles share; a class names its library symbols bis_<_sym>_*."""

    _sym = None

    def _fn(self, what):
        return getattr(self.ctx.lib, f"bis_{self._sym}_{what}")

    def set_preconditioner(self, pc, Ls=None, Us=None, A_D=None, A_D_inv=None, L_D=None, U_D=None, outer=1, inner=0):
        """The preconditioner of the solve, before init: a PC name or number with the operands its type reads; an MG or a BJ
        object stands for "mg" / "bj" with its operand as Ls."""
        def p(v):
            return C.c_void_p(v.ptr) if v is not None else C.c_void_p()
        pc, Ls = _handle_pc(pc, Ls)
        self._keep_pc = (Ls, Us, A_D, A_D_inv, L_D, U_D)
        self.ctx.check(self._fn("set_preconditioner")(
            self.ctx.h, self.h, C.c_int(PC[pc] if isinstance(pc, str) else pc),
            Ls.h if Ls is not None else C.c_void_p(), Us.h if Us is not None else C.c_void_p(),
            p(A_D), p(A_D_inv), p(L_D), p(U_D), C.c_int(outer), C.c_int(inner)))

    def iterate(self, n):
        self.ctx.check(self._fn("iterate")(self.ctx.h, self.h, C.c_int(int(n))))

    def free(self):
        if self.h:
            self._fn("destroy")(self.ctx.h, self.h)
            self.h = C.c_void_p()


class CG(_Solver):
    _sym = "cg"

    def __init__(self, ctx, A, b, x, A_D=None):
        self.ctx = ctx
        self.h = C.c_void_p()
        ctx.check(ctx.lib.bis_cg_create(ctx.h, A.h, C.c_void_p(A_D.ptr) if A_D else C.c_void_p(),
                                        C.c_void_p(b.ptr), C.c_void_p(x.ptr), C.byref(self.h)))

    def init(self, tol):
        r0 = C.c_double()
        self.ctx.check(self.ctx.lib.bis_cg_init(self.ctx.h, self.h, C.c_double(tol), C.byref(r0)))
        return r0.value

    def status(self, hist_cap=4096):
        iters, conv = C.c_int(), C.c_int()
        hist = np.zeros(hist_cap)
        self.ctx.check(self.ctx.lib.bis_cg_status(self.ctx.h, self.h, C.byref(iters), C.byref(conv),
                                                  hist.ctypes, C.c_int(hist_cap)))
        return iters.value, bool(conv.value), hist[:min(iters.value + 1, hist_cap)].copy()


class MCG(_Solver):
    """k CG solves in lock-step on one matrix stream (bis_mcg_*): B, X are n x k interleaved device blocks."""

    _sym = "mcg"

    def __init__(self, ctx, A, B, X, k, A_D=None):
        self.ctx, self.k = ctx, int(k)
        self.h = C.c_void_p()
        self._keep = (A, B, X, A_D)
        ctx.check(ctx.lib.bis_mcg_create(ctx.h, A.h, C.c_void_p(A_D.ptr) if A_D else C.c_void_p(),
                                         C.c_void_p(B.ptr), C.c_void_p(X.ptr), C.c_int(self.k), C.byref(self.h)))

    def init(self, tol):
        r0 = np.zeros(self.k)
        self.ctx.check(self.ctx.lib.bis_mcg_init(self.ctx.h, self.h, C.c_double(tol), r0.ctypes))
        return r0

    def status(self, j, hist_cap=4096):
        iters, conv = C.c_int(), C.c_int()
        hist = np.zeros(hist_cap)
        self.ctx.check(self.ctx.lib.bis_mcg_status(self.ctx.h, self.h, C.c_int(int(j)), C.byref(iters), C.byref(conv),
                                                   hist.ctypes, C.c_int(hist_cap)))
        return iters.value, bool(conv.value), hist[:min(iters.value + 1, hist_cap)].copy()


class MBiCGSTAB(_Solver):
    """k BiCGSTAB solves in lock-step (bis_mbicgstab_*): B, X are n x k interleaved device blocks; two SpMMs and two
    preconditioner applies per iteration for all columns."""

    _sym = "mbicgstab"

    def __init__(self, ctx, A, B, X, k):
        self.ctx, self.k = ctx, int(k)
        self.h = C.c_void_p()
        self._keep = (A, B, X)
        ctx.check(ctx.lib.bis_mbicgstab_create(ctx.h, A.h, C.c_void_p(B.ptr), C.c_void_p(X.ptr), C.c_int(self.k), C.byref(self.h)))

    def init(self, tol):
        r0 = np.zeros(self.k)
        self.ctx.check(self.ctx.lib.bis_mbicgstab_init(self.ctx.h, self.h, C.c_double(tol), r0.ctypes))
        return r0

    def status(self, j, hist_cap=4096):
        iters, conv = C.c_int(), C.c_int()
        hist = np.zeros(hist_cap)
        self.ctx.check(self.ctx.lib.bis_mbicgstab_status(self.ctx.h, self.h, C.c_int(int(j)), C.byref(iters), C.byref(conv),
                                                         hist.ctypes, C.c_int(hist_cap)))
        return iters.value, bool(conv.value), hist[:min(iters.value + 1, hist_cap)].copy()


class MGMRES(_Solver):
    """k restarted GMRES(restart) solves in lock-step (bis_mgmres_*): B, X are n x k interleaved device blocks; one SpMM and one
    preconditioner apply per iteration for all columns, the Gram-Schmidt coefficients and the Givens algebra stay on the
    device.  X of a live column is x_old of its cycle: `solution` gives the explicit iterate."""

    _sym = "mgmres"

    def __init__(self, ctx, A, B, X, k, restart=10):
        self.ctx, self.k, self.restart = ctx, int(k), int(restart)
        self.h = C.c_void_p()
        self._keep = (A, B, X)
        ctx.check(ctx.lib.bis_mgmres_create(ctx.h, A.h, C.c_void_p(B.ptr), C.c_void_p(X.ptr), C.c_int(self.k),
                                            C.c_int(self.restart), C.byref(self.h)))

    def init(self, tol):
        r0 = np.zeros(self.k)
        self.ctx.check(self.ctx.lib.bis_mgmres_init(self.ctx.h, self.h, C.c_double(tol), r0.ctypes))
        return r0

    def status(self, j, hist_cap=4096):
        """(iterations, converged, history): the history has iterations + 1 + restarts entries (n_hist of bis_mgmres_status)."""
        iters, conv, n_hist = C.c_int(), C.c_int(), C.c_int()
        hist = np.zeros(hist_cap)
        self.ctx.check(self.ctx.lib.bis_mgmres_status(self.ctx.h, self.h, C.c_int(int(j)), C.byref(iters), C.byref(conv),
                                                      C.byref(n_hist), hist.ctypes, C.c_int(hist_cap)))
        return iters.value, bool(conv.value), hist[:min(n_hist.value, hist_cap)].copy()

    def solution(self, out):
        """The explicit x of every column into the n x k block `out` (bis_mgmres_solution); the solve does not change."""
        self.ctx.check(self.ctx.lib.bis_mgmres_solution(self.ctx.h, self.h, C.c_void_p(out.ptr)))


class FGMRES(_Solver):
    """Restarted flexible GMRES(restart) on one right-hand side as a device schedule (bis_fgmres_*): the preconditioner stands
    on the right and may change from step to step (an MG K-cycle), the history is the true residual's.  x changes only at a
    restart or a stop: `solution` gives the explicit iterate."""

    _sym = "fgmres"

    def __init__(self, ctx, A, b, x, restart=10):
        self.ctx, self.restart = ctx, int(restart)
        self.h = C.c_void_p()
        self._keep = (A, b, x)
        ctx.check(ctx.lib.bis_fgmres_create(ctx.h, A.h, C.c_void_p(b.ptr), C.c_void_p(x.ptr), C.c_int(self.restart),
                                            C.byref(self.h)))

    def init(self, tol):
        r0 = C.c_double()
        self.ctx.check(self.ctx.lib.bis_fgmres_init(self.ctx.h, self.h, C.c_double(tol), C.byref(r0)))
        return r0.value

    def status(self, hist_cap=4096):
        """(iterations, converged, history): the history has iterations + 1 + restarts entries (n_hist of bis_fgmres_status)."""
        iters, conv, n_hist = C.c_int(), C.c_int(), C.c_int()
        hist = np.zeros(hist_cap)
        self.ctx.check(self.ctx.lib.bis_fgmres_status(self.ctx.h, self.h, C.byref(iters), C.byref(conv), C.byref(n_hist),
                                                      hist.ctypes, C.c_int(hist_cap)))
        return iters.value, bool(conv.value), hist[:min(n_hist.value, hist_cap)].copy()

    def solution(self, out):
        """The explicit iterate into the n-vector `out` (bis_fgmres_solution); the solve does not change."""
        self.ctx.check(self.ctx.lib.bis_fgmres_solution(self.ctx.h, self.h, C.c_void_p(out.ptr)))


class MINRES(_Solver):
    """Preconditioned MINRES on one right-hand side as a device schedule (bis_minres_*): symmetric A, definite or not, and
    one fixed symmetric positive definite preconditioner (not checked).  The history is phibar: the residual norm in the
    M^-1 norm, the 2-norm without a preconditioner; it never increases.  x is the iterate of the last history entry."""

    _sym = "minres"

    def __init__(self, ctx, A, b, x):
        self.ctx = ctx
        self.h = C.c_void_p()
        self._keep = (A, b, x)
        ctx.check(ctx.lib.bis_minres_create(ctx.h, A.h, C.c_void_p(b.ptr), C.c_void_p(x.ptr), C.byref(self.h)))

    def init(self, tol):
        r0 = C.c_double()
        self.ctx.check(self.ctx.lib.bis_minres_init(self.ctx.h, self.h, C.c_double(tol), C.byref(r0)))
        return r0.value

    def status(self, hist_cap=4096):
        """(iterations, converged, history[0 .. iterations])"""
        iters, conv = C.c_int(), C.c_int()
        hist = np.zeros(hist_cap)
        self.ctx.check(self.ctx.lib.bis_minres_status(self.ctx.h, self.h, C.byref(iters), C.byref(conv),
                                                      hist.ctypes, C.c_int(hist_cap)))
        return iters.value, bool(conv.value), hist[:min(iters.value + 1, hist_cap)].copy()


class IDR(_Solver):
    """Right-preconditioned IDR(s), 1 <= s <= 8, on one right-hand side as a device schedule (bis_idr_*): nonsymmetric A,
    one fixed preconditioner (not checked), short recurrences and no restart; one SpMV, one apply and one history entry per
    iteration.  The history is the recurrence of the true residual norm.  x is the iterate of the last history entry."""

    _sym = "idr"

    def __init__(self, ctx, A, b, x, s=4):
        self.ctx, self.s = ctx, int(s)
        self.h = C.c_void_p()
        self._keep = (A, b, x)
        ctx.check(ctx.lib.bis_idr_create(ctx.h, A.h, C.c_void_p(b.ptr), C.c_void_p(x.ptr), C.c_int(self.s), C.byref(self.h)))

    def set_shadow(self, P):
        """The shadow space: an n x s array (column j is P[:, j]) instead of the hashed default; before init."""
        P = np.asfortranarray(P, dtype=np.float64)
        if P.ndim != 2 or P.shape[1] != self.s:
            raise BisError(f"IDR.set_shadow: P must have {self.s} columns")
        self.ctx.check(self.ctx.lib.bis_idr_set_shadow(self.ctx.h, self.h, P.ctypes))

    def init(self, tol):
        r0 = C.c_double()
        self.ctx.check(self.ctx.lib.bis_idr_init(self.ctx.h, self.h, C.c_double(tol), C.byref(r0)))
        return r0.value

    def status(self, hist_cap=4096):
        """(iterations, converged, history[0 .. iterations])"""
        iters, conv = C.c_int(), C.c_int()
        hist = np.zeros(hist_cap)
        self.ctx.check(self.ctx.lib.bis_idr_status(self.ctx.h, self.h, C.byref(iters), C.byref(conv),
                                                   hist.ctypes, C.c_int(hist_cap)))
        return iters.value, bool(conv.value), hist[:min(iters.value + 1, hist_cap)].copy()


class LSMR(_Solver):
    """LSMR on one right-hand side as a device schedule (bis_lsmr_*): min ||A x - b||^2 + damp^2 ||x||^2 for a rectangular
    A of any shape.  `At` is A.transpose() (made and owned by the handle when None).  `col_scaling` is a Vec d of n positive
    entries, or "norm": d = 1 / the column norms of A, computed on the device, 1 where a norm is 0; the iteration then runs
    on A diag(d) and damping acts on x / d.  `hist` estimates the residual of the normal equations and never increases,
    `hist_r` the norm of the (stacked) residual.  x is the iterate of the last history entry.  No preconditioner."""

    _sym = "lsmr"
    REASON = {0: "live", 1: "tol_r", 2: "tol_ar", 3: "breakdown", 4: "non-finite"}

    def __init__(self, ctx, A, b, x, At=None, damp=0.0, col_scaling=None):
        self.ctx = ctx
        self.h = C.c_void_p()
        self._own = []
        if b.n < A.n_rows or x.n < A.n_cols:
            raise BisError(f"LSMR: b needs {A.n_rows} entries and x {A.n_cols}")
        try:
            if isinstance(col_scaling, str):
                if col_scaling != "norm":
                    raise BisError(f"LSMR: unknown col_scaling {col_scaling!r}")
                if At is None:
                    At = A.transpose()
                    self._own.append(At)
                col_scaling = At.row_norms()
                self._own.append(col_scaling)
                ctx.check(ctx.lib.bis_lsmr_scaling_from_norms(ctx.h, C.c_void_p(col_scaling.ptr), _i64(A.n_cols),
                                                              C.c_void_p(col_scaling.ptr)))
            elif col_scaling is not None and col_scaling.n != A.n_cols:
                raise BisError(f"LSMR: col_scaling has {col_scaling.n} entries, A has {A.n_cols} columns")
            self._keep = (A, At, b, x, col_scaling)
            ctx.check(ctx.lib.bis_lsmr_create(ctx.h, A.h, At.h if At is not None else C.c_void_p(), C.c_void_p(b.ptr),
                                               C.c_void_p(x.ptr), C.byref(self.h)))
            if damp:
                ctx.check(ctx.lib.bis_lsmr_set_damping(ctx.h, self.h, C.c_double(damp)))
            if col_scaling is not None:
                ctx.check(ctx.lib.bis_lsmr_set_col_scaling(ctx.h, self.h, C.c_void_p(col_scaling.ptr)))
        except Exception:
            self.free()
            raise
        self.col_scaling = col_scaling

    def set_preconditioner(self, *args, **kwargs):
        raise BisError("LSMR has no preconditioner (bis_lsmr_*): use col_scaling")

    def set_damping(self, damp):
        self.ctx.check(self.ctx.lib.bis_lsmr_set_damping(self.ctx.h, self.h, C.c_double(damp)))

    def set_col_scaling(self, d):
        """d: a Vec of n entries, or None to clear; before init."""
        if d is not None and d.n != self._keep[0].n_cols:
            raise BisError(f"LSMR: col_scaling has {d.n} entries, A has {self._keep[0].n_cols} columns")
        self.ctx.check(self.ctx.lib.bis_lsmr_set_col_scaling(self.ctx.h, self.h, C.c_void_p(d.ptr) if d is not None else C.c_void_p()))
        self._keep = self._keep[:4] + (d,)
        self.col_scaling = d

    def init(self, tol_r, tol_ar=None):
        """(r0, ar0); tol_ar=None: the same value as tol_r."""
        r0, ar0 = C.c_double(), C.c_double()
        self.ctx.check(self.ctx.lib.bis_lsmr_init(self.ctx.h, self.h, C.c_double(tol_r), C.c_double(tol_r if tol_ar is None else tol_ar),
                                                  C.byref(r0), C.byref(ar0)))
        return r0.value, ar0.value

    def status(self, hist_cap=4096):
        """dict(iters, converged, reason, hist (the ar column), hist_r), histories with entries 0 .. iters."""
        iters, conv, reason = C.c_int(), C.c_int(), C.c_int()
        hist, hist_r = np.zeros(hist_cap), np.zeros(hist_cap)
        self.ctx.check(self.ctx.lib.bis_lsmr_status(self.ctx.h, self.h, C.byref(iters), C.byref(conv), C.byref(reason),
                                                    hist.ctypes, hist_r.ctypes, C.c_int(hist_cap)))
        cnt = min(iters.value + 1, hist_cap)
        return dict(iters=iters.value, converged=bool(conv.value), reason=reason.value, hist=hist[:cnt].copy(), hist_r=hist_r[:cnt].copy())

    def free(self):
        super().free()
        for o in self._own:
            o.free()
        self._own = []


class Eigs(_Solver):
    """Thick-restart Lanczos with full re-orthogonalisation as a device schedule (bis_eigs_*): the k smallest ("SA"),
    largest ("LA") or largest in magnitude ("LM") eigenpairs of a symmetric matrix.  `ncv` is the basis size, k < ncv <=
    min(n, 64) (None: min(n, 64, max(2k + 1, 20))); `v0` a Vec of n entries (None: column 0 of IDR's hashed shadow space).
    A=None with n= is the caller-applied mode: `iterate` is refused, every product is the caller's, between `op_begin()` and
    `op_end()` on the context's stream (shift-and-invert with a MINRES handle).  No preconditioner."""

    _sym = "eigs"
    WHICH = {"SA": 0, "LA": 1, "LM": 2}
    REASON = {0: "live", 1: "converged", 2: "invariant", 3: "jacobi", 4: "bad_start"}

    def __init__(self, ctx, A, k=4, which="SA", ncv=None, tol=1e-10, v0=None, n=None):
        self.ctx = ctx
        self.h = C.c_void_p()
        if which not in self.WHICH:
            raise BisError(f"Eigs: which must be one of SA, LA, LM, not {which!r}")
        if A is None and n is None:
            raise BisError("Eigs: the caller-applied mode (A=None) needs n=")
        self.n = int(A.n_rows if A is not None else n)
        self.k, self.which, self.tol = int(k), which, float(tol)
        self._keep = (A, v0)
        ctx.check(ctx.lib.bis_eigs_create(ctx.h, A.h if A is not None else C.c_void_p(), _i64(self.n), C.c_int(self.k),
                                          C.c_int(0 if ncv is None else int(ncv)), C.c_int(self.WHICH[which]), C.byref(self.h)))
        self.ncv = int(ncv) if ncv is not None else min(self.n, 64, max(2 * self.k + 1, 20))
        if v0 is not None:
            try:
                self.set_start(v0)
            except Exception:
                self.free()
                raise

    def set_preconditioner(self, *args, **kwargs):
        raise BisError("Eigs has no preconditioner (bis_eigs_*)")

    def set_start(self, v0):
        """v0: a Vec of n entries, or None for the default; before init."""
        if v0 is not None and v0.n < self.n:
            raise BisError(f"Eigs: v0 has {v0.n} entries, the operator has {self.n} rows")
        self.ctx.check(self.ctx.lib.bis_eigs_set_start(self.ctx.h, self.h, C.c_void_p(v0.ptr) if v0 is not None else C.c_void_p()))
        self._keep = (self._keep[0], v0)

    def init(self, tol=None):
        if tol is not None:
            self.tol = float(tol)
        self.ctx.check(self.ctx.lib.bis_eigs_init(self.ctx.h, self.h, C.c_double(self.tol)))

    def iterate(self, cycles=1):
        self.ctx.check(self.ctx.lib.bis_eigs_iterate(self.ctx.h, self.h, C.c_int(int(cycles))))

    def op_begin(self):
        """(inp, out): two Vec views of n entries; enqueue out = OP inp on the context's stream, then call op_end()."""
        inp, out = C.c_void_p(), C.c_void_p()
        self.ctx.check(self.ctx.lib.bis_eigs_op_begin(self.ctx.h, self.h, C.byref(inp), C.byref(out)))
        return Vec(self.ctx, inp.value, self.n, False), Vec(self.ctx, out.value, self.n, False)

    def op_end(self):
        self.ctx.check(self.ctx.lib.bis_eigs_op_end(self.ctx.h, self.h))

    def status(self, hist_cap=4096):
        """dict(products, restarts, stopped, converged, reason, nconv, values, est, hist, hist_nconv): values and estimates of
        the last restart in rank order, the histories with one entry per restart."""
        prod, rest, stop, conv, reason, nconv = (C.c_int() for _ in range(6))
        values, est = np.zeros(self.k), np.zeros(self.k)
        hist, hist_n = np.zeros(hist_cap), np.zeros(hist_cap)
        self.ctx.check(self.ctx.lib.bis_eigs_status(self.ctx.h, self.h, C.byref(prod), C.byref(rest), C.byref(stop), C.byref(conv),
                                                    C.byref(reason), C.byref(nconv), values.ctypes, est.ctypes, hist.ctypes,
                                                    hist_n.ctypes, C.c_int(hist_cap)))
        cnt = min(rest.value, hist_cap)
        return dict(products=prod.value, restarts=rest.value, stopped=bool(stop.value), converged=bool(conv.value),
                    reason=reason.value, nconv=nconv.value, values=values, est=est, hist=hist[:cnt].copy(),
                    hist_nconv=hist_n[:cnt].astype(np.int64))

    def vectors(self):
        """The Ritz vectors of the last restart in rank order as a host n x k array."""
        X = self.ctx.alloc(self.n * self.k)
        try:
            self.ctx.check(self.ctx.lib.bis_eigs_vectors(self.ctx.h, self.h, C.c_void_p(X.ptr), _i64(self.n)))
            return X.to_host().reshape(self.k, self.n).T.copy()
        finally:
            X.free()

    def solve(self, max_cycles=100, batch=4):
        """init, then iterate in batches of `batch` cycles and poll until the solve stops or max_cycles are enqueued; status()."""
        self.init()
        done = 0
        while done < max_cycles:
            step = min(batch, max_cycles - done)
            self.iterate(step)
            done += step
            st = self.status()
            if st["stopped"]:
                return st
        return self.status()


class SVDS(_Solver):
    """Golub-Kahan-Lanczos bidiagonalisation with thick restart as a device schedule (bis_svds_*): the k largest ("LM") or
    smallest ("SM") singular triplets of a rows x cols matrix of any shape.  `ncv` is the basis size, k < ncv <=
    min(rows, cols, 64) (None: min(rows, cols, 64, max(2k + 1, 20))); `v0` a Vec of min(rows, cols) entries (None: column 0 of
    IDR's hashed shadow space); `At` is A.transpose() (made and owned by the handle when None).  A=None with shape=(rows,
    cols) is the caller-applied mode: `iterate` is refused, every product is the caller's, between `op_begin()` and
    `op_end()` on the context's stream.  SM uses plain Ritz values: slow on ill-conditioned matrices.  No preconditioner."""

    _sym = "svds"
    WHICH = {"LM": 0, "SM": 1}
    REASON = {0: "live", 1: "converged", 2: "invariant", 3: "jacobi", 4: "bad_start"}

    def __init__(self, ctx, A, k=4, which="LM", ncv=None, tol=1e-10, v0=None, At=None, shape=None):
        self.ctx = ctx
        self.h = C.c_void_p()
        if which not in self.WHICH:
            raise BisError(f"SVDS: which must be one of LM, SM, not {which!r}")
        if A is None and shape is None:
            raise BisError("SVDS: the caller-applied mode (A=None) needs shape=(rows, cols)")
        self.rows, self.cols = (int(A.n_rows), int(A.n_cols)) if A is not None else (int(shape[0]), int(shape[1]))
        self.ns = min(self.rows, self.cols)
        self.k, self.which, self.tol = int(k), which, float(tol)
        self._keep = (A, At, v0)
        ctx.check(ctx.lib.bis_svds_create(ctx.h, A.h if A is not None else C.c_void_p(), At.h if At is not None else C.c_void_p(),
                                          _i64(self.rows), _i64(self.cols), C.c_int(self.k), C.c_int(0 if ncv is None else int(ncv)),
                                          C.c_int(self.WHICH[which]), C.byref(self.h)))
        self.ncv = int(ncv) if ncv is not None else min(self.ns, 64, max(2 * self.k + 1, 20))
        if v0 is not None:
            try:
                self.set_start(v0)
            except Exception:
                self.free()
                raise

    def set_preconditioner(self, *args, **kwargs):
        raise BisError("SVDS has no preconditioner (bis_svds_*)")

    def set_start(self, v0):
        """v0: a Vec of min(rows, cols) entries, or None for the default; before init."""
        if v0 is not None and v0.n < self.ns:
            raise BisError(f"SVDS: v0 has {v0.n} entries, the short side of the operator has {self.ns}")
        self.ctx.check(self.ctx.lib.bis_svds_set_start(self.ctx.h, self.h, C.c_void_p(v0.ptr) if v0 is not None else C.c_void_p()))
        self._keep = self._keep[:2] + (v0,)

    def init(self, tol=None):
        if tol is not None:
            self.tol = float(tol)
        self.ctx.check(self.ctx.lib.bis_svds_init(self.ctx.h, self.h, C.c_double(self.tol)))

    def iterate(self, cycles=1):
        self.ctx.check(self.ctx.lib.bis_svds_iterate(self.ctx.h, self.h, C.c_int(int(cycles))))

    def op_begin(self):
        """(inp, out, transposed): two Vec views; enqueue out = A inp (transposed False) or out = A^T inp (True) on the
        context's stream, then call op_end()."""
        inp, out, tr = C.c_void_p(), C.c_void_p(), C.c_int()
        self.ctx.check(self.ctx.lib.bis_svds_op_begin(self.ctx.h, self.h, C.byref(inp), C.byref(out), C.byref(tr)))
        n_in, n_out = (self.rows, self.cols) if tr.value else (self.cols, self.rows)
        return Vec(self.ctx, inp.value, n_in, False), Vec(self.ctx, out.value, n_out, False), bool(tr.value)

    def op_end(self):
        self.ctx.check(self.ctx.lib.bis_svds_op_end(self.ctx.h, self.h))

    def status(self, hist_cap=4096):
        """dict(products, restarts, stopped, converged, reason, nconv, sigma_ref, values, est, hist, hist_nconv): values and
        estimates of the last restart in rank order, the histories with one entry per restart."""
        prod, rest, stop, conv, reason, nconv = (C.c_int() for _ in range(6))
        sref = C.c_double()
        values, est = np.zeros(self.k), np.zeros(self.k)
        hist, hist_n = np.zeros(hist_cap), np.zeros(hist_cap)
        self.ctx.check(self.ctx.lib.bis_svds_status(self.ctx.h, self.h, C.byref(prod), C.byref(rest), C.byref(stop), C.byref(conv),
                                                    C.byref(reason), C.byref(nconv), C.byref(sref), values.ctypes, est.ctypes,
                                                    hist.ctypes, hist_n.ctypes, C.c_int(hist_cap)))
        cnt = min(rest.value, hist_cap)
        return dict(products=prod.value, restarts=rest.value, stopped=bool(stop.value), converged=bool(conv.value),
                    reason=reason.value, nconv=nconv.value, sigma_ref=sref.value, values=values, est=est, hist=hist[:cnt].copy(),
                    hist_nconv=hist_n[:cnt].astype(np.int64))

    def vectors(self):
        """(U, V): the left (rows x k) and right (cols x k) singular vectors of the last restart in rank order, on the host."""
        U, V = self.ctx.alloc(self.rows * self.k), self.ctx.alloc(self.cols * self.k)
        try:
            self.ctx.check(self.ctx.lib.bis_svds_vectors(self.ctx.h, self.h, C.c_void_p(U.ptr), _i64(self.rows), C.c_void_p(V.ptr),
                                                         _i64(self.cols)))
            return U.to_host().reshape(self.k, self.rows).T.copy(), V.to_host().reshape(self.k, self.cols).T.copy()
        finally:
            U.free()
            V.free()

    def solve(self, max_cycles=100, batch=4):
        """init, then iterate in batches of `batch` cycles and poll until the solve stops or max_cycles are enqueued; status()."""
        self.init()
        done = 0
        while done < max_cycles:
            step = min(batch, max_cycles - done)
            self.iterate(step)
            done += step
            st = self.status()
            if st["stopped"]:
                return st
        return self.status()


# ---- multi-GPU (1-D row partition) -------------------------------------------
class Stat:
    """Jacobi / Gauss-Seidel / symmetric Gauss-Seidel as device schedules (bis_stat_*)."""
    KIND = {"j": 0, "gs": 1, "sgs": 2}

    def __init__(self, ctx, kind, A, D, b, x, Ls=None, Us=None):
        self.ctx = ctx
        self.h = C.c_void_p()
        self._keep = (A, D, b, x, Ls, Us)
        ctx.check(ctx.lib.bis_stat_create(ctx.h, C.c_int(self.KIND[kind]), A.h, Ls.h if Ls else None, Us.h if Us else None,
                                          C.c_void_p(D.ptr), C.c_void_p(b.ptr), C.c_void_p(x.ptr), C.byref(self.h)))

    def init(self, tol):
        r0 = C.c_double()
        self.ctx.check(self.ctx.lib.bis_stat_init(self.ctx.h, self.h, C.c_double(tol), C.byref(r0)))
        return r0.value

    def iterate(self, n):
        self.ctx.check(self.ctx.lib.bis_stat_iterate(self.ctx.h, self.h, C.c_int(int(n))))

    def status(self, hist_cap=4096):
        it, conv = C.c_int(), C.c_int()
        hist = np.zeros(hist_cap)
        self.ctx.check(self.ctx.lib.bis_stat_status(self.ctx.h, self.h, C.byref(it), C.byref(conv), hist.ctypes, C.c_int(hist_cap)))
        return it.value, bool(conv.value), hist[:min(it.value + 1, hist_cap)]

    def solution(self, out):
        self.ctx.check(self.ctx.lib.bis_stat_solution(self.ctx.h, self.h, C.c_void_p(out.ptr)))

    def free(self):
        if self.h:
            self.ctx.lib.bis_stat_destroy(self.ctx.h, self.h)
            self.h = None


class CommOps(C.Structure):
    _fields_ = [("user", C.c_void_p),
                ("allreduce_sum", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int)),
                ("exchange", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int64),
                                         C.c_int))]


def halo_plan(n_local, row_ptr, col_global, n_ranks, rank, row_starts):
    """Host-only planning (bis_halo_plan): returns (halo_cols, recv_counts, interior)."""
    lib = load_library()
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
    col = np.ascontiguousarray(col_global, dtype=np.int32)
    rs = np.ascontiguousarray(row_starts, dtype=np.int64)
    n_halo = C.c_int64()
    recv = np.zeros(n_ranks, dtype=np.int64)
    interior = np.zeros(2, dtype=np.int64)
    st = lib.bis_halo_plan(_i64(n_local), rp.ctypes, col.ctypes, C.c_int(n_ranks), C.c_int(rank),
                           rs.ctypes, C.byref(n_halo), None, _i64(0), recv.ctypes, interior.ctypes)
    if st != 0:
        raise BisError(f"bis_halo_plan failed: {st}")
    halo = np.zeros(n_halo.value, dtype=np.int32)
    st = lib.bis_halo_plan(_i64(n_local), rp.ctypes, col.ctypes, C.c_int(n_ranks), C.c_int(rank),
                           rs.ctypes, C.byref(n_halo), halo.ctypes, _i64(halo.size), recv.ctypes,
                           interior.ctypes)
    if st != 0:
        raise BisError(f"bis_halo_plan failed: {st}")
    return halo, recv, interior


class Dist:
    """bis_dist: the row-partitioned operator of one rank."""

    def __init__(self, ctx, A_local, rank, n_ranks, row_starts):
        self.ctx, self.rank, self.n_ranks = ctx, rank, n_ranks
        self.row_starts = np.ascontiguousarray(row_starts, dtype=np.int64)
        self.h = C.c_void_p()
        ctx.check(ctx.lib.bis_dist_create(ctx.h, A_local.h, C.c_int(rank), C.c_int(n_ranks),
                                          self.row_starts.ctypes, C.byref(self.h)))
        A_local.h = C.c_void_p()  # consumed
        nl, ne = C.c_int64(), C.c_int64()
        ctx.lib.bis_dist_vec_len(self.h, C.byref(nl), C.byref(ne))
        self.n_local, self.n_ext = nl.value, ne.value
        self._keep = None

    def halo_info(self):
        n_halo = C.c_int64()
        recv = np.zeros(self.n_ranks, dtype=np.int64)
        self.ctx.lib.bis_dist_halo_info(self.h, C.byref(n_halo), None, _i64(0), recv.ctypes)
        halo = np.zeros(n_halo.value, dtype=np.int32)
        self.ctx.lib.bis_dist_halo_info(self.h, C.byref(n_halo), halo.ctypes, _i64(halo.size),
                                        recv.ctypes)
        return halo, recv

    def set_send_lists(self, send_counts, send_cols):
        sc = np.ascontiguousarray(send_counts, dtype=np.int64)
        cols = np.ascontiguousarray(send_cols, dtype=np.int32)
        self.ctx.check(self.ctx.lib.bis_dist_set_send_lists(self.ctx.h, self.h, sc.ctypes, cols.ctypes))

    def set_comm(self, ops):
        self._keep = ops  # keep the callbacks alive
        self.ctx.check(self.ctx.lib.bis_dist_set_comm(self.ctx.h, self.h, C.byref(ops)))

    def use_rccl(self, unique_id_bytes):
        buf = C.create_string_buffer(bytes(unique_id_bytes), 128)
        self.ctx.check(self.ctx.lib.bis_dist_use_rccl(self.ctx.h, self.h, buf))

    def spmv(self, x_ext, y):
        self.ctx.check(self.ctx.lib.bis_dist_spmv(self.ctx.h, self.h, C.c_void_p(x_ext.ptr),
                                                  C.c_void_p(y.ptr)))

    def dot(self, a, b):
        out = C.c_double()
        dev = self.ctx.alloc(1)
        self.ctx.check(self.ctx.lib.bis_dist_dot(self.ctx.h, self.h, C.c_void_p(a.ptr),
                                                 C.c_void_p(b.ptr), C.c_void_p(dev.ptr), C.byref(out)))
        dev.free()
        return out.value

    def stats(self):
        nh, ns, ni = C.c_int64(), C.c_int64(), C.c_int64()
        nn, nr = C.c_int(), C.c_int()
        self.ctx.lib.bis_dist_stats(self.h, C.byref(nh), C.byref(ns), C.byref(ni), C.byref(nn), C.byref(nr))
        return dict(halo_entries=nh.value, send_entries=ns.value, halo_bytes_per_spmv=8 * (nh.value + ns.value),
                    interior_rows=ni.value, neighbours=nn.value, rccl_ranks_seen=nr.value)

    def spmv_stream_info(self):
        """(col_bytes, val_bytes, n_dict, form) of the interior rows' SpMV (bis_dist_spmv_stream_info)."""
        c, v, n, f = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(self.ctx.lib.bis_dist_spmv_stream_info(self.ctx.h, self.h, C.byref(c), C.byref(v), C.byref(n), C.byref(f)))
        return c.value, v.value, n.value, f.value

    def spmv_streamed_bytes(self):
        """Bytes this rank's distributed SpMV moves at least per launch triple (bis_dist_spmv_streamed_bytes)."""
        b = C.c_int64()
        self.ctx.check(self.ctx.lib.bis_dist_spmv_streamed_bytes(self.ctx.h, self.h, C.byref(b)))
        return b.value

    def profile_read(self):
        ne, na = C.c_int64(), C.c_int64()
        te, ta = C.c_double(), C.c_double()
        self.ctx.check(self.ctx.lib.bis_dist_profile_read(self.ctx.h, self.h, C.byref(ne), C.byref(te),
                                                          C.byref(na), C.byref(ta)))
        return dict(exchanges=ne.value, exchange_ms=te.value, allreduces=na.value, allreduce_ms=ta.value)

    def cg(self, b, x, A_D=None):
        cg = CG.__new__(CG)
        cg.ctx = self.ctx
        cg.h = C.c_void_p()
        self.ctx.check(self.ctx.lib.bis_dist_cg_create(
            self.ctx.h, self.h, C.c_void_p(A_D.ptr) if A_D else C.c_void_p(), C.c_void_p(b.ptr),
            C.c_void_p(x.ptr), C.byref(cg.h)))
        return cg

    def free(self):
        if self.h:
            self.ctx.lib.bis_dist_destroy(self.ctx.h, self.h)
            self.h = C.c_void_p()


def rccl_unique_id(ctx):
    buf = C.create_string_buffer(128)
    ctx.check(ctx.lib.bis_rccl_unique_id(ctx.h, buf))
    return bytes(buf.raw)
