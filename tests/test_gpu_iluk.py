"""GPU: ILU(k) with level-of-fill (bis_iluk.hip + the fill mode of bis_ilu0.hip) against tests/iluk_ref.py.

Patterns must equal the reference's exactly (27-point grids, whose filled rows sit at and beyond the wave width, and a seeded
structurally unsymmetric pattern with shuffled rows, with 32- and 64-bit row pointers); values meet the ILU gate of
test_gpu_ilu0_edges.py (1e-13 per factor) and, on a small case with an exact-fma reference, agree bit for bit; every ILU(0)
kernel setting gives the default's bits; level 0 IS Context.ilu0; L U = P on P's positions and ILU(n) is the complete
factorisation; rows that fill past kIluMaxRow take the lane-per-row kernel; a row beyond the search table's capacity is
refused; CG needs fewer iterations with more fill."""
import ctypes as C

import numpy as np
import pytest

import iluk_ref as ref
from helpers import OptionScope, relerr
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

KTOL = 1e-13         # the ILU gate of test_gpu_ilu0_edges.py
KILU_MAX_ROW = 1024  # bis_ilu0.hip kIluMaxRow
# the settings of test_gpu_ilu0_edges._ILU_CONFIGS
_ILU_CONFIGS = [dict(ilu0_wave=w, ilu0_persistent=p, ilu0_wgs=g) for w in (0, -1) for p in (0, -1) for g in (1, 2, 4)
                if not (p == 0 and g != 4)]


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    base = c.options()
    yield c
    assert c.options() == base
    c.close()


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def hpcg(nx):
    """The 27-point matrix of the generator: 26 on the diagonal, -1 towards every neighbour, natural order."""
    idx = np.arange(nx ** 3).reshape(nx, nx, nx)  # [z, y, x]
    rows, cols = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                src = idx[max(0, -dz):nx - max(0, dz), max(0, -dy):nx - max(0, dy), max(0, -dx):nx - max(0, dx)]
                dst = idx[max(0, dz):nx - max(0, -dz), max(0, dy):nx - max(0, -dy), max(0, dx):nx - max(0, -dx)]
                rows.append(src.ravel())
                cols.append(dst.ravel())
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    val = np.where(rows == cols, 26.0, -1.0)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nx ** 3))])
    return CRS(nx ** 3, rp, cols.astype(np.int32), val)


def unsymmetric(n, seed, per_row=3, band=12):
    """Seeded, structurally unsymmetric, diagonally dominant; near entries, a few far ones, columns shuffled inside the rows."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), per_row)
    cols = np.clip(rows + rng.integers(-band, band + 1, rows.size), 0, n - 1)
    far = rng.random(rows.size) < 0.04
    cols[far] = rng.integers(0, n, int(far.sum()))
    rows, cols = np.concatenate([rows, np.arange(n)]), np.concatenate([cols, np.arange(n)])
    _, first = np.unique(rows.astype(np.int64) * n + cols, return_index=True)
    rows, cols = rows[first], cols[first]
    val = rng.uniform(-1, 1, rows.size)
    val[rows == cols] = 2.0 * per_row + 2.0 + rng.uniform(0, 1, int((rows == cols).sum()))
    order = np.lexsort((rng.random(rows.size), rows))
    rows, cols, val = rows[order], cols[order], val[order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return CRS(n, rp, cols.astype(np.int32), val)


def long_rows(n):
    """Row 0 dense, column 0 stored in 8 scattered rows, a tridiagonal rest: at level 1 those 8 rows fill completely."""
    hit = set(int(r) for r in np.linspace(n // 7, n - 3, 8).astype(int))
    rows, cols, val = [], [], []
    rng = np.random.default_rng(n)
    for i in range(n):
        c = set([i] + ([i - 1] if i else []) + ([i + 1] if i + 1 < n else []))
        if i == 0:
            c = set(range(n))
        if i in hit:
            c.add(0)
        c = sorted(c)
        rows += [i] * len(c)
        cols += c
        val += [8.0 + rng.uniform(0, 1) if j == i else rng.uniform(-1, 1) / 64 for j in c]
    rows = np.asarray(rows)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return CRS(n, rp, np.asarray(cols, dtype=np.int32), np.asarray(val)), sorted(hit)


_MATS = {}


def mat(name):
    if name not in _MATS:
        kind, arg = name.split(":")
        _MATS[name] = hpcg(int(arg)) if kind == "hpcg" else unsymmetric(int(arg), 4100 + int(arg))
    return _MATS[name]


_REF = {}


def reference(name, k, exact=False):
    """(Ls, L_D, Us, U_D, P, n_fill) of the restatement, computed once per case and left alone."""
    key = (name, k, exact)
    if key not in _REF:
        _REF[key] = ref.iluk(mat(name), k, exact=exact)
    return _REF[key]


def factor(ctx, A, k, **kw):
    dA = ctx.matrix(A)
    try:
        dLs, dL_D, dUs, dU_D, n_fill = ctx.iluk(dA, k, **kw)
    finally:
        dA.free()
    n = A.n_rows
    out = dict(Ls=CRS(n, *dLs.download()), L_D=dL_D.to_host(), Us=CRS(n, *dUs.download()), U_D=dU_D.to_host(), n_fill=n_fill,
               numeric=dLs.ilu0_kernel(), symbolic=dLs.iluk_kernel(), hint=(dLs.grid_hint(), dUs.grid_hint()))
    for h in (dLs, dL_D, dUs, dU_D):
        h.free()
    return out


def same_pattern(a, b, tag):
    assert np.array_equal(a.row_ptr, b.row_ptr) and np.array_equal(a.col, b.col), (tag, "pattern")


def assert_factors(got, want, exact, tag):
    wLs, wL_D, wUs, wU_D = want[:4]
    for k, (a, b) in enumerate(((got["Ls"], wLs), (got["Us"], wUs))):
        same_pattern(a, b, (tag, "LU"[k]))
        if exact:
            assert np.array_equal(_bits(a.val), _bits(b.val)), (tag, "LU"[k])
        else:
            err = relerr(a.val, b.val)
            print(tag, "LU"[k], "relative error", err)
            assert err <= KTOL, (tag, "LU"[k], err)
    assert np.array_equal(_bits(got["L_D"]), _bits(wL_D)), (tag, "L_D")
    if exact:
        assert np.array_equal(_bits(got["U_D"]), _bits(wU_D)), (tag, "U_D")
    else:
        assert relerr(got["U_D"], wU_D) <= KTOL, (tag, "U_D")


def expected_numeric(max_row, cfg):
    if max_row > KILU_MAX_ROW or cfg.get("ilu0_wave", -1) == 0:
        return "ilu0_level_kernel"
    return "ilu0_level_wave_kernel" if cfg.get("ilu0_persistent", -1) == 0 else "ilu0_persistent_kernel"


def dense(F, diag=None):
    n = F.n_rows
    M = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(F.row_ptr))
    M[rows, F.col] = F.val
    if diag is not None:
        M[np.arange(n), np.arange(n)] = diag
    return M


@pytest.mark.parametrize("rp64", [-1, 1])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("name", ["hpcg:6", "unsym:300"])
def test_pattern_equals_the_reference(ctx, name, k, rp64):
    """The padded matrix: pattern, n_fill, A's values at A's positions, +0.0 (the bits) at the fill positions; the search
    that ran is named, one search for the symmetric pattern and two for the other."""
    A = mat(name)
    P, n_fill = reference(name, k)[4:]
    if name == "hpcg:6":  # rows at the wave width for k = 1, across it beyond
        longest = int(np.diff(P.row_ptr).max())
        assert (longest <= 64) == (k == 1) and longest > 32
    with OptionScope(ctx, force_rp64=rp64):
        dA = ctx.matrix(A)
        dP, got_fill = ctx.iluk_symbolic(dA, k)
        got = CRS(A.n_rows, *dP.download())
        kernel, hint = dP.iluk_kernel(), dP.grid_hint()
        dP.free(); dA.free()
    same_pattern(got, P, (name, k))
    assert got_fill == n_fill == P.nnz - A.nnz and n_fill > 0
    assert np.array_equal(_bits(got.val), _bits(P.val))
    assert kernel == "iluk_search_kernel RP=%d %s" % (64 if rp64 == 1 else 32,
                                                     "one search, transposed" if name.startswith("hpcg") else "two searches")
    assert hint == (0, 0, 0, 0)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_values_on_the_grid(ctx, k):
    got = factor(ctx, mat("hpcg:8"), k)
    want = reference("hpcg:8", k)
    assert_factors(got, want, False, ("hpcg:8", k))
    assert got["n_fill"] == want[5]
    assert got["numeric"] == "ilu0_persistent_kernel" and got["symbolic"].endswith("one search, transposed")


@pytest.mark.parametrize("k", [1, 3])
def test_values_bit_for_bit_with_the_exact_fma(ctx, k):
    """48 rows, unsymmetric: the restatement with one correctly rounded fma per update gives the device's bits."""
    got = factor(ctx, mat("unsym:48"), k)
    assert_factors(got, reference("unsym:48", k, exact=True), True, ("unsym:48", k))


def test_every_kernel_setting_gives_the_same_bits(ctx):
    A = mat("hpcg:8")
    base = factor(ctx, A, 2)
    longest = int(np.diff(reference("hpcg:8", 2)[4].row_ptr).max())
    assert base["numeric"] == expected_numeric(longest, {})
    for cfg in _ILU_CONFIGS:
        with OptionScope(ctx, **cfg):
            got = factor(ctx, A, 2)
        assert got["numeric"] == expected_numeric(longest, cfg), (cfg, got["numeric"])
        assert_factors(got, (base["Ls"], base["L_D"], base["Us"], base["U_D"]), True, cfg)


def test_level_zero_is_ilu0(ctx):
    """Bit for bit, with the non-zero rule: the stored zero at (1, 2) stays a zero at level 0 and fills at level 1 (its level
    is 0: the position is A's own, so level 1 adds no position, only the update)."""
    rp = np.array([0, 3, 6, 9])
    col = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2], dtype=np.int32)
    val = np.array([4.0, 1.0, 1.0, 1.0, 4.0, 0.0, 1.0, 1.0, 4.0])
    small = CRS(3, rp, col, val)
    for A in (small, mat("hpcg:6"), mat("unsym:300")):
        got = factor(ctx, A, 0)
        dA = ctx.matrix(A)
        dLs, dL_D, dUs, dU_D = ctx.ilu0(dA)
        want = (CRS(A.n_rows, *dLs.download()), dL_D.to_host(), CRS(A.n_rows, *dUs.download()), dU_D.to_host())
        assert got["numeric"] == dLs.ilu0_kernel() and got["symbolic"] == "" and got["n_fill"] == 0
        for h in (dLs, dL_D, dUs, dU_D, dA):
            h.free()
        assert_factors(got, want, True, "level 0")
    got0, got1 = factor(ctx, small, 0), factor(ctx, small, 1)
    assert got0["Us"].col.tolist() == [1, 2, 2] and got0["Us"].val[2] == 0.0
    assert got1["n_fill"] == 0 and got1["Us"].val[2] == -0.25
    # a generated grid: level 0 keeps the hint of ilu0's factors, level 1 carries none
    dA = ctx.gen_hpcg(8)
    l0, l1 = ctx.iluk(dA, 0), ctx.iluk(dA, 1)
    i0 = ctx.ilu0(dA)
    assert l0[0].grid_hint() == i0[0].grid_hint() and l0[2].grid_hint() == i0[2].grid_hint()
    assert l1[0].grid_hint() == (0, 0, 0, 0) and l1[2].grid_hint() == (0, 0, 0, 0)
    for h in list(l0[:4]) + list(l1[:4]) + list(i0) + [dA]:
        h.free()


def test_l_times_u_equals_p_on_the_pattern(ctx):
    A = mat("hpcg:8")
    got = factor(ctx, A, 2)
    P = reference("hpcg:8", 2)[4]
    LU = (dense(got["Ls"]) + np.eye(A.n_rows)) @ dense(got["Us"], got["U_D"])
    rows = np.repeat(np.arange(A.n_rows), np.diff(P.row_ptr))
    err = np.abs(LU[rows, P.col] - P.val).max()
    print("max |(LU - P)_ij| on P:", err)
    assert err <= 1e-12 * np.abs(A.val).max()


def test_level_sixteen_on_sixteen_rows_is_the_complete_factorisation(ctx):
    A = ref.random_pattern(16, 0.2, False, 616)
    got = factor(ctx, A, 16)
    LU = (dense(got["Ls"]) + np.eye(16)) @ dense(got["Us"], got["U_D"])
    DA = dense(A)
    err = np.abs(LU - DA).max()
    print("max |LU - A|:", err, "norm", np.linalg.norm(DA))
    assert err <= 1e-13 * np.linalg.norm(DA)


def test_rows_that_fill_past_the_wave_kernels_limit(ctx):
    n = 1500
    A, hit = long_rows(n)
    P, n_fill = ref.padded(A, ref.symbolic_two_search(A, 1))
    lens = np.diff(P.row_ptr)
    assert all(lens[r] == n for r in hit) and n > KILU_MAX_ROW
    got = factor(ctx, A, 1)
    assert got["numeric"] == "ilu0_level_kernel" and got["n_fill"] == n_fill
    assert_factors(got, ref.numeric(P), False, "long rows")


def test_capacity_is_refused_loudly(ctx):
    from basic_iterative_solvers_amd import iluk_limits
    max_level, max_visit = iluk_limits()
    A, _ = long_rows(max_visit + 64)
    dA = ctx.matrix(A)
    h, h2, nf = C.c_void_p(), C.c_void_p(), C.c_int64(-7)
    assert ctx.lib.bis_mat_iluk_symbolic(ctx.h, dA.h, C.c_int(1), C.byref(h), C.byref(nf)) == 6  # BIS_ERR_UNSUPPORTED
    msg = ctx.lib.bis_last_error(ctx.h).decode()
    assert "row 0 " in msg and str(max_visit) in msg, msg  # the dense row itself is the first beyond the table
    assert not h and nf.value == -7
    L_D, U_D = ctx.alloc(A.n_rows), ctx.alloc(A.n_rows)
    assert ctx.lib.bis_mat_iluk(ctx.h, dA.h, C.c_int(1), C.c_double(1e-8), C.c_double(1e-4), C.byref(h), C.byref(h2),
                                C.c_void_p(L_D.ptr), C.c_void_p(U_D.ptr), C.byref(nf)) == 6
    assert not h and not h2 and nf.value == -7
    for v in (L_D, U_D, dA):
        v.free()


def _cg(ctx, dA, fac, pc, b, tol, inner=0):
    dLs, dL_D, dUs, dU_D = fac[:4]
    n = len(b)
    uinv = ctx.alloc(n)
    ctx.elemwise_div_vectors(uinv, dL_D, dU_D)
    db, dx = ctx.upload(b), ctx.upload(np.zeros(n))
    cg = ctx.cg(dA, db, dx)
    cg.set_preconditioner(pc, Ls=dLs, Us=dUs, A_D=dL_D, A_D_inv=uinv, L_D=dL_D, U_D=dU_D, inner=inner)
    r0 = cg.init(tol)
    cg.iterate(200)
    iters, conv, hist = cg.status()
    x = dx.to_host()
    for h in (cg, db, dx, uinv):
        h.free()
    return iters, conv, x, r0


def test_cg_needs_fewer_iterations_with_more_fill(ctx):
    """hpcg 12^3, b = 1, x_0 = 0, stop at 1e-8 ||r_0||: strictly fewer iterations at level 1 than at 0, no more at 2 than at 1
    (the restatement on the CPU: 11 / 8 / 6); the true residual meets the tolerance up to the rounding of one residual
    evaluation, n eps (||A||_inf ||x||_inf + ||b||_inf)."""
    A = mat("hpcg:12")
    n, tol = A.n_rows, 1e-8
    b = np.ones(n)
    S = A.to_scipy()
    dA = ctx.matrix(A)
    counts = []
    for k in (0, 1, 2):
        fac = ctx.iluk(dA, k)
        iters, conv, x, r0 = _cg(ctx, dA, fac, "ilu0", b, tol)
        assert conv and r0 == np.sqrt(n)
        slack = n * 2.0 ** -52 * (abs(S).sum(axis=1).max() * np.abs(x).max() + 1.0)
        assert np.linalg.norm(b - S @ x) <= tol * r0 + slack, k
        counts.append(iters)
        if k == 2:  # the same factors, rounded to fp32, through the iterative triangular solves
            for F in (fac[0], fac[2]):
                F.round_f32()
            it_iters, it_conv, x, r0 = _cg(ctx, dA, fac, "ilu0it", b, tol, inner=6)
            assert it_conv and np.linalg.norm(b - S @ x) <= tol * r0 + slack
            print("ilu0it after round_f32, level 2:", it_iters, "iterations")
        for h in fac[:4]:
            h.free()
    dA.free()
    print("CG iterations at level 0 / 1 / 2:", counts)
    assert counts[1] < counts[0] and counts[2] <= counts[1]


def test_two_calls_give_the_same_bits(ctx):
    A = mat("unsym:300")
    a, b = factor(ctx, A, 2), factor(ctx, A, 2)
    assert_factors(a, (b["Ls"], b["L_D"], b["Us"], b["U_D"]), True, "second call")
    assert a["n_fill"] == b["n_fill"] and a["symbolic"] == b["symbolic"] == "iluk_search_kernel RP=32 two searches"


def test_input_errors(ctx):
    from basic_iterative_solvers_amd import BisError
    A = mat("unsym:48")
    dA = ctx.matrix(A)
    for call in (ctx.iluk, ctx.iluk_symbolic):
        with pytest.raises(BisError, match="status 2"):  # BIS_ERR_INVALID
            call(dA, 17)
        with pytest.raises(BisError, match="status 2"):
            call(dA, -1)
    dA.free()
    rp, col, val = A.row_ptr.copy(), A.col.copy(), A.val.copy()
    # a column repeated inside row 5
    dup = CRS(48, np.concatenate([rp[:6], rp[6:] + 1]), np.insert(col, rp[6], col[rp[5]]), np.insert(val, rp[6], 0.5))
    # row 7 without its diagonal
    d = rp[7] + int(np.nonzero(col[rp[7]:rp[8]] == 7)[0][0])
    nod = CRS(48, np.concatenate([rp[:8], rp[8:] - 1]), np.delete(col, d), np.delete(val, d))
    for M, status in ((dup, 6), (nod, 5)):  # BIS_ERR_UNSUPPORTED, BIS_ERR_NO_DIAG
        dM = ctx.matrix(M)
        for call in (ctx.iluk, ctx.iluk_symbolic):
            with pytest.raises(BisError, match="status %d" % status):
                call(dM, 1)
        dM.free()
