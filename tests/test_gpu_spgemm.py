"""GPU: bis_spgemm and bis_mat_transpose (bis_spgemm.hip) against tests/spgemm_ref.py.

The gate is "the same bits": row pointers, columns and values of the device product equal the restatement's, on the row
path, on the sort fallback (spgemm_row_cap = 0), with batches small enough that the product takes many of them and one row
exceeds a batch, and with 64-bit row pointers.  The restatement is computed once per input and shared."""
import ctypes as C

import numpy as np
import pytest

import spgemm_ref as ref
import test_gpu_mg as base
from helpers import OptionScope, check_rows

pytestmark = pytest.mark.gpu
INVALID = 2
ROW, SORT, BOTH = "spgemm_row_kernel", "spgemm_sort_fallback", "spgemm_row_kernel + spgemm_sort_fallback"
same_bits, host_crs = base.same_bits, base.host_crs


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


def sparse_random(rng, n, m, per_row, empty_every=0, sort=True):
    rp, col, val = [0], [], []
    for i in range(n):
        k = 0 if (empty_every and i % empty_every == 1) else int(rng.integers(1, per_row + 1))
        c = rng.choice(m, size=min(k, m), replace=False)
        c = np.sort(c) if sort else c
        col.extend(c.tolist())
        val.extend(rng.uniform(-1, 1, len(c)).tolist())
        rp.append(len(col))
    return ref.crs(n, m, rp, col, val)


def dense_row_band():
    """A band of half-width 2 on 3000 rows with row 17 dense: the products of row 17 of A A (about 18000) exceed any row
    cap, and every row that holds column 17 has more than 3000."""
    n = 3000
    rng = np.random.default_rng(23)
    rp, col, val = [0], [], []
    for i in range(n):
        c = np.arange(n) if i == 17 else np.arange(max(0, i - 2), min(n, i + 3))
        col.extend(c.tolist())
        val.extend(rng.uniform(-1, 1, len(c)).tolist())
        rp.append(len(col))
    return ref.crs(n, n, rp, col, val)


def pairs(ctx):
    """name -> (A, B) on the host."""
    rng = np.random.default_rng(19)
    hp = host_crs(ctx.gen_hpcg(8, 7, 6))
    band = ref.crs_from_dense(base.band600())
    T = ref.crs(600, 75, np.arange(601), np.arange(600) // 8, np.ones(600))
    A75 = ref.spgemm(band, T)
    Ac, Bc = ref.crs_from_dense(np.array([[1.0, 2.0, 0.0], [0.0, 1.0, 3.0], [0.5, 0.0, -0.5]])), \
        ref.crs_from_dense(np.array([[2.0, 1.0, 0.0, 0.0], [-1.0, 0.0, 4.0, 0.0], [0.0, 0.0, 8.0, 0.0]]))
    rep = ref.crs(4, 5, [0, 3, 4, 4, 7], [2, 0, 2, 4, 1, 1, 3], rng.uniform(-1, 1, 7))
    dense = dense_row_band()
    return {
        "hpcg876": (hp, hp),
        "band600": (band, band),
        "band_600x75_75x600": (A75, ref.transpose(A75)),
        "empty_rows": (sparse_random(rng, 90, 70, 6, empty_every=5), sparse_random(rng, 70, 110, 7, empty_every=3)),
        "cancelling": (Ac, Bc),
        "repeats_unsorted": (rep, sparse_random(rng, 5, 40, 9, sort=False)),
        "dense_row": (dense, dense),
    }


NAMES = ["hpcg876", "band600", "band_600x75_75x600", "empty_rows", "cancelling", "repeats_unsorted", "dense_row"]
# the path of the default options: B with unsorted rows sends every row to the fallback; the dense row exceeds the cap
DEFAULT_PATH = dict(hpcg876=ROW, band600=ROW, band_600x75_75x600=ROW, empty_rows=ROW, cancelling=ROW, repeats_unsorted=SORT, dense_row=BOTH)


@pytest.fixture(scope="module")
def cases(ctx):
    """Per input, made once and left alone: the host pair, the restated product, the device operands."""
    host = pairs(ctx)
    cache = {}

    def get(name):
        if name not in cache:
            A, B = host[name]
            dA = ctx.matrix(A)
            dB = dA if B is A else ctx.matrix(B)
            cache[name] = dict(A=A, B=B, dA=dA, dB=dB, C=ref.spgemm(A, B))
        return cache[name]
    return get


def bound(A, B):
    """u_i = sum over the entries (i, j) of A of nnz(B_j)."""
    return np.bincount(ref.rows_of(A), weights=np.diff(B.row_ptr)[A.col], minlength=A.n_rows).astype(np.int64)


def expected_path(u, cap, b_sorted=True):
    on_row = b_sorted and np.any((u > 0) & (u <= cap))
    on_sort = np.any(u > (cap if b_sorted else 0))
    return BOTH if on_row and on_sort else ROW if on_row else SORT if on_sort else ""


def assert_same_matrix(dC, want, tag):
    got = host_crs(dC)
    assert (dC.n_rows, dC.n_cols) == (want.n_rows, want.n_cols), tag
    assert np.array_equal(got.row_ptr, want.row_ptr), f"{tag}: row pointers"
    assert np.array_equal(got.col, want.col), f"{tag}: columns"
    assert same_bits(got.val, want.val), f"{tag}: values"
    return got


@pytest.mark.parametrize("name", NAMES)
def test_product_has_the_restatements_bits_on_every_path(ctx, cases, name):
    e = cases(name)
    u = bound(e["A"], e["B"])
    dC = ctx.spgemm(e["dA"], e["dB"])
    print(f"{name}: {e['A'].n_rows} x {e['A'].n_cols} times {e['B'].n_rows} x {e['B'].n_cols}: nnz(C) {dC.nnz}, products per row "
          f"up to {int(u.max())}, path '{dC.spgemm_kernel()}'")
    assert dC.spgemm_kernel() == DEFAULT_PATH[name] == expected_path(u, 4096, b_sorted=name != "repeats_unsorted")
    first = assert_same_matrix(dC, e["C"], name)
    assert dC.rp_width == 4 and dC.grid_hint() == (0, 0, 0, 0)
    dC2 = ctx.spgemm(e["dA"], e["dB"])
    second = assert_same_matrix(dC2, e["C"], name + " (second call)")
    assert same_bits(first.val, second.val)
    dC.free(); dC2.free()
    with OptionScope(ctx, spgemm_row_cap=0):
        dC = ctx.spgemm(e["dA"], e["dB"])
        assert dC.spgemm_kernel() == SORT
        assert_same_matrix(dC, e["C"], name + " spgemm_row_cap=0")
        dC.free()
    # batches of at most 1500 products: many batches everywhere but on the tiny pair; the dense row (about 18000) exceeds one
    total = int(u.sum())
    with OptionScope(ctx, spgemm_row_cap=0, spgemm_batch=1500):
        dC = ctx.spgemm(e["dA"], e["dB"])
        assert dC.spgemm_kernel() == SORT
        assert_same_matrix(dC, e["C"], name + " spgemm_batch=1500")
        dC.free()
    if name in ("hpcg876", "band600", "dense_row"):
        assert total > 20 * 1500
    if name == "dense_row":
        assert u.max() > 1500 * 10
    # a cap between the row lengths: the shorter rows on the row path, the longer ones in batches
    cap = max(1, int(np.median(u)))
    with OptionScope(ctx, spgemm_row_cap=cap, spgemm_batch=1500):
        dC = ctx.spgemm(e["dA"], e["dB"])
        assert dC.spgemm_kernel() == expected_path(u, cap, b_sorted=name != "repeats_unsorted")
        assert_same_matrix(dC, e["C"], name + " mixed")
        dC.free()


def test_every_bin_of_the_row_path_is_used(cases):
    """The inputs reach the one-wave kernel (<= 256 products) and the four-wave kernel (up to the cap)."""
    def of(name):
        return bound(cases(name)["A"], cases(name)["B"])
    assert of("hpcg876").max() > 256 and of("hpcg876").min() <= 256
    assert 256 < of("band600").max() <= 4096
    d = of("dense_row")
    assert d.max() > 4096 and np.any((d > 256) & (d <= 4096)) and np.any(d <= 256)


def test_cancelled_entries_stay_in_the_pattern(ctx, cases):
    e = cases("cancelling")
    dC = ctx.spgemm(e["dA"], e["dB"])
    rp, col, val = dC.download()
    assert rp[1] == 3 and col[:3].tolist() == [0, 1, 2] and val[0] == 0.0 and val[1] == 1.0 and val[2] == 8.0
    dC.free()


def test_64_bit_row_pointers(ctx, cases):
    e = cases("hpcg876")
    with OptionScope(ctx, force_rp64=1):
        dA = ctx.matrix(e["A"])
        assert dA.rp_width == 8
        dC = ctx.spgemm(dA, dA)
        assert dC.rp_width == 8 and dC.spgemm_kernel() == ROW
        assert_same_matrix(dC, e["C"], "rp64")
        dT = dA.transpose()
        assert dT.rp_width == 8
        assert_same_matrix(dT, ref.transpose(e["A"]), "rp64 transpose")
        with OptionScope(ctx, spgemm_row_cap=0, spgemm_batch=4000):
            dC2 = ctx.spgemm(dA, e["dA"])  # (mixed widths)
            assert_same_matrix(dC2, e["C"], "rp64 fallback")
            dC2.free()
    for m in (dC, dT, dA):
        m.free()


@pytest.mark.parametrize("name", NAMES)
def test_transpose(ctx, cases, name):
    e = cases(name)
    for key in ("A", "B"):
        H, dM = e[key], e["d" + key]
        dT = dM.transpose()
        got = assert_same_matrix(dT, ref.transpose(H), f"{name} {key}^T")
        assert dT.grid_hint() == (0, 0, 0, 0)
        lens = np.diff(got.row_ptr)
        inner = np.ones(len(got.col), dtype=bool)
        inner[got.row_ptr[:-1][lens > 0]] = False
        assert np.all(np.diff(got.col.astype(np.int64))[inner[1:]] >= 0), "rows of A^T do not ascend"
        dTT = dT.transpose()
        back = host_crs(dTT)
        assert np.array_equal(back.row_ptr, H.row_ptr)
        sorted_rows = all(np.all(np.diff(H.col[H.row_ptr[i]:H.row_ptr[i + 1]].astype(np.int64)) > 0) for i in range(H.n_rows))
        if sorted_rows:
            assert np.array_equal(back.col, H.col) and same_bits(back.val, H.val), f"{name} {key}: (A^T)^T != A"
        dT.free(); dTT.free()


def test_transpose_keeps_the_order_of_repeats_and_a_symmetric_matrix(ctx, cases):
    R = ref.crs(2, 3, [0, 3, 4], [2, 0, 2, 2], [1.0, 2.0, 3.0, 4.0])
    dR = ctx.matrix(R)
    dT = dR.transpose()
    rp, col, val = dT.download()
    assert rp.tolist() == [0, 1, 1, 4] and col.tolist() == [0, 0, 0, 1] and val.tolist() == [2.0, 1.0, 3.0, 4.0]
    dT.free(); dR.free()
    e = cases("band600")  # symmetric bit for bit (band_dense writes both triangles from one draw)
    dT = e["dA"].transpose()
    assert_same_matrix(dT, e["A"], "A^T of a symmetric A")
    dT.free()


def test_error_table(ctx, cases):
    e = cases("empty_rows")
    lib = ctx.lib
    out = C.c_void_p()
    assert lib.bis_spgemm(ctx.h, None, e["dB"].h, C.byref(out)) == INVALID and not out
    assert lib.bis_spgemm(ctx.h, e["dA"].h, None, C.byref(out)) == INVALID and not out
    assert lib.bis_spgemm(ctx.h, e["dA"].h, e["dB"].h, None) == INVALID
    assert lib.bis_spgemm(ctx.h, e["dA"].h, e["dA"].h, C.byref(out)) == INVALID and not out  # 90 x 70 times 90 x 70
    assert lib.bis_mat_transpose(ctx.h, None, C.byref(out)) == INVALID and not out
    assert lib.bis_mat_transpose(ctx.h, e["dA"].h, None) == INVALID
    # n = 0 and nnz = 0: an empty C, BIS_OK
    Z = ctx.matrix(ref.crs(0, 70, [0], [], []))
    dC = ctx.spgemm(Z, e["dB"])
    assert (dC.n_rows, dC.n_cols, dC.nnz) == (0, 110, 0) and dC.spgemm_kernel() == ""
    dC.free()
    E = ctx.matrix(ref.crs(90, 70, np.zeros(91), [], []))
    for path in (dict(), dict(spgemm_row_cap=0)):
        with OptionScope(ctx, **path):
            dC = ctx.spgemm(E, e["dB"])
            rp, col, val = dC.download()
            assert (dC.n_rows, dC.n_cols, dC.nnz) == (90, 110, 0) and not rp.any()
            dC.free()
    dT = E.transpose()
    assert (dT.n_rows, dT.n_cols, dT.nnz) == (70, 90, 0)
    # A has entries, but only towards empty rows of B: no product at all
    only = ctx.matrix(ref.crs(2, 70, [0, 1, 2], [1, 4], [1.0, 2.0]))
    assert np.diff(e["B"].row_ptr)[[1, 4]].tolist() == [0, 0]
    dC = ctx.spgemm(only, e["dB"])
    assert dC.nnz == 0 and dC.n_rows == 2
    for m in (dC, only, dT, E, Z):
        m.free()


def test_spmv_on_a_rectangular_product(ctx, cases):
    e = cases("band_600x75_75x600")
    dA75 = e["dA"]
    x = np.random.default_rng(29).uniform(-1, 1, 75)
    dx, dy = ctx.upload(x), ctx.alloc(600)
    ctx.spmv(dA75, dx, dy)
    check_rows(dy.to_host(), e["A"], x, "600 x 75")
    e2 = cases("empty_rows")
    dC = ctx.spgemm(e2["dA"], e2["dB"])  # 90 x 110
    x = np.random.default_rng(31).uniform(-1, 1, 110)
    dx2, dy2 = ctx.upload(x), ctx.upload(np.full(90, np.nan))
    ctx.spmv(dC, dx2, dy2)
    check_rows(dy2.to_host(), e2["C"], x, "90 x 110 product")
    for v in (dx, dy, dx2, dy2):
        v.free()
    dC.free()
