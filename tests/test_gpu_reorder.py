"""The reordering layer (bis_reorder.hip: multi-colour ordering, -scale, vector gather / scatter; bis_order.hip: BFS / RCM,
bis_mat_permute, the structural-symmetry check) past two 256-row blocks and on adversarial graphs, entry for entry against
the sequential definitions of reorder_ref.py, with 32-bit and with 64-bit row pointers.

Sizes: N1 = 65 836 rows = 257 blocks + 44 (the second trip of the single-workgroup scans, the per-colour scan down 258
blocks), N2 = 524 588 rows = 2049 blocks + 44 (past the grid caps of fill / max / gather / scatter, and a second ticket
for every workgroup of the colouring's persistent grid).  All comparisons are exact except the SpMV on the permuted or
scaled matrix, which is held to helpers.check_rows (per row, against math.fsum).  test_reorder_ref_cpu.py pins the colour
and component counts these cases rely on."""
import functools

import numpy as np
import pytest

import reorder_ref as R
from helpers import check_rows, permute_crs, relerr
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

N1 = 65836
N2 = 524588
KTOL = 1e-13  # kernel-level relative tolerance, as in test_gpu_kernels.py


@pytest.fixture(scope="module", params=[4, 8], ids=["rp32", "rp64"])
def ctx(request):
    """A context of its own per row-pointer width; force_rp64 makes every matrix created from here on carry int64 row
    pointers (each case asserts the width it got)."""
    from basic_iterative_solvers_amd import Context
    c = Context()
    if request.param == 8:
        c.set_option("force_rp64", 1)
    c.rp_width = request.param
    yield c
    if request.param == 8:
        c.set_option("force_rp64", -1)
    c.close()


@pytest.fixture(scope="module")
def vctx():
    """For the vector kernels, which see no row pointers."""
    from basic_iterative_solvers_amd import Context
    c = Context()
    yield c
    c.close()


def _matrix(ctx, A):
    dA = ctx.matrix(A)
    assert dA.rp_width == ctx.rp_width
    return dA


def _same_matrix(dB, want, width):
    assert dB.rp_width == width
    rp, col, val = dB.download()
    assert np.array_equal(rp, want.row_ptr), "row_ptr"
    assert np.array_equal(col, want.col), "col"
    assert np.array_equal(val, want.val), "val"  # (bit for bit: the values are copied)


def _spmv_on(ctx, dB, B, seed, sample=None):
    """y = B x on the device against check_rows.  sample: the rows check_rows walks (its per-row fsum takes 5 s at N2);
    every row is then also held to twice the bound against the float64 row sums, whose own error is one such bound."""
    x = np.random.default_rng(seed).uniform(-1, 1, B.n_cols)
    dx, dy = ctx.upload(x), ctx.alloc(B.n_rows)
    ctx.spmv(dB, dx, dy)
    y = dy.to_host()
    dx.free(); dy.free()
    if sample is None:
        check_rows(y, B, x)
        return
    lens = np.diff(B.row_ptr)
    rows = np.repeat(np.arange(B.n_rows), lens)
    prod = B.val * x[B.col]
    want = np.bincount(rows, weights=prod, minlength=B.n_rows)
    mag = np.bincount(rows, weights=np.abs(prod), minlength=B.n_rows)
    assert np.all(np.abs(y - want) <= 2.0 * (lens + 2) * 2.0 ** -53 * mag)
    idx = np.concatenate([np.arange(B.row_ptr[r], B.row_ptr[r + 1]) for r in sample])
    sub = CRS(len(sample), np.concatenate([[0], np.cumsum(lens[sample])]), B.col[idx], B.val[idx], n_cols=B.n_cols)
    check_rows(y[sample], sub, x)


def _sample_rows(n):
    """The first and the last 1024 rows, 512 rows around the 256-block boundary of the scans, and every 8th row."""
    pick = np.zeros(n, dtype=bool)
    pick[:1024] = pick[-1024:] = pick[65536 - 256:65536 + 256] = True
    pick[::8] = True
    return np.flatnonzero(pick)


# ---- multi-colour ------------------------------------------------------------------------------------------------------

MC_CASES = {
    "banded_N1": lambda: R.banded_sym(N1, 2, 40),
    "banded_N2": lambda: R.banded_sym(N2, 2, 40),
    "ragged": lambda: R.ragged_lower(5000),
    "path_N1": lambda: R.path(N1),
    "clique64": lambda: R.clique_at(1000, 224, 64),
    "unsym": lambda: R.unsym(5000),
    "n1": lambda: R.banded_sym(1, 2, 40),
    "n255": lambda: R.banded_sym(255, 2, 40),
    "n256": lambda: R.banded_sym(256, 2, 40),
    "n257": lambda: R.banded_sym(257, 2, 40),
}


@functools.lru_cache(maxsize=None)
def _mc_ref(name):
    """(A, colours, perm, P A P^T) of a case, computed once for both widths and left unchanged."""
    A = MC_CASES[name]()
    colour = R.greedy_colours(A)
    perm = R.colour_perm(colour)
    return A, colour, perm, permute_crs(A, perm)


def _multicolour_case(ctx, name):
    A, colour, perm, B = _mc_ref(name)
    dA = _matrix(ctx, A)
    dB, perm_dev, n_col = ctx.multicolour(dA)
    dA.free()
    assert n_col == int(colour.max()) + 1
    # perm is the stable sort of the rows by colour: with the colour count it pins the colour of every row
    assert np.array_equal(perm_dev, perm)
    _same_matrix(dB, B, ctx.rp_width)
    return dB, B, perm


@pytest.mark.parametrize("name", ["banded_N1", "banded_N2", "ragged", "clique64", "n1", "n255", "n256", "n257"])
def test_multicolour_equals_sequential_greedy(ctx, name):
    dB, B, _ = _multicolour_case(ctx, name)
    if name == "clique64":
        assert int(_mc_ref(name)[1].max()) + 1 == 64  # `used` is all ones only after the last clique row
    _spmv_on(ctx, dB, B, 5, sample=_sample_rows(N2) if name == "banded_N2" else None)
    dB.free()


def test_multicolour_path_waits_across_every_ticket(ctx):
    """The path graph: every row waits for its predecessor, across all 258 tickets.  Two colours, evens then odds."""
    dB, B, perm = _multicolour_case(ctx, "path_N1")
    assert int(_mc_ref("path_N1")[1].max()) + 1 == 2
    assert np.array_equal(perm, np.concatenate([np.arange(0, N1, 2), np.arange(1, N1, 2)]))
    _spmv_on(ctx, dB, B, 6)
    dB.free()


def test_multicolour_refuses_65_colours_and_goes_on(ctx, oracle):
    from basic_iterative_solvers_amd import BisError
    dA = _matrix(ctx, R.clique_at(1000, 224, 65))
    with pytest.raises(BisError, match="more than 64 colours"):
        ctx.multicolour(dA)
    dA.free()
    A = oracle.gen_hpcg(9, 7, 8)
    colour = R.greedy_colours(A)
    dB, perm, n_col = ctx.multicolour(_matrix(ctx, A))
    assert n_col == 8 == int(colour.max()) + 1
    assert np.array_equal(perm, R.colour_perm(colour))
    _same_matrix(dB, permute_crs(A, perm), ctx.rp_width)


def test_multicolour_unsymmetric_pattern_costs_levels_never_correctness(ctx, oracle):
    """On an unsymmetric pattern the colouring still equals the sequential one (lower entries only), B is P A P^T, and the
    triangular sweeps on B's strict triangles -- which derive their dependency order from B itself, coupled rows of one
    colour included -- agree with the sequential sweeps on the host-permuted matrix.  The comparison is the one of
    test_gpu_kernels.test_sptrsv_few_level_path_bit_exact: B's triangles decompose into a few blocks of independent rows
    and take the streaming form (products rounded, then summed: the kernel tolerance, as everywhere in the suite for that
    form; measured on the MI355X: "spmv_rowblock_kernel", max |dev - seq| = 4.4e-16 forward and backward, both widths);
    a sweep that reports one of the forms carrying the reference's fma chain has to give its bits."""
    few_level = ("spmv_rowblock_kernel (triangular epilogue", "trsv_level_kernel")
    dB, B, _ = _multicolour_case(ctx, "unsym")
    n = B.n_rows
    _, Ls, _, Us = oracle.split_LU(B)
    rows = np.repeat(np.arange(n), np.diff(B.row_ptr))
    D = np.zeros(n)
    D[rows[B.col == rows]] = B.val[B.col == rows]
    assert np.all(D != 0.0)
    dLs, dUs, dD, dDinv = ctx.split_strict(dB)
    assert np.array_equal(dD.to_host(), D)
    b = np.random.default_rng(9).uniform(-1, 1, n)
    x = ctx.upload(b)
    ctx.sptrsv(dLs, x, dD, x)  # x aliases b
    x2, db = ctx.alloc(n), ctx.upload(b)
    ctx.bsptrsv(dUs, x2, dD, db)
    for tag, got, want, kernel in (("forward", x.to_host(), oracle.sptrsv(Ls, D, b.copy()), dLs.sweep_kernel(False)),
                                   ("backward", x2.to_host(), oracle.sptrsv(Us, D, b.copy(), backward=True), dUs.sweep_kernel(True))):
        print(f"{tag} sweep: {kernel}: max |dev - seq| = {float(np.max(np.abs(got - want))):.3g}")
        assert relerr(got, want) <= KTOL, (tag, kernel)
        if not kernel.startswith(few_level):
            assert np.array_equal(got, want), (tag, kernel)


def test_multicolour_refusals(ctx):
    from basic_iterative_solvers_amd import BisError
    with pytest.raises(BisError, match="empty matrix"):
        ctx.multicolour(ctx.matrix(CRS(0, [0], [], [])))
    with pytest.raises(BisError, match="square matrix required"):
        ctx.multicolour(ctx.matrix(CRS(3, [0, 1, 2, 3], [0, 1, 3], [1.0, 1.0, 1.0], n_cols=4)))


# ---- BFS / RCM / permute -----------------------------------------------------------------------------------------------

BFS_CASES = {
    "grid257": lambda: R.grid2d(257),                       # frontiers up to 257 wide: expand_kernel on two blocks
    "grid513_tail": lambda: R.with_tail(R.grid2d(513), 3),  # 263 172 rows: the second component starts at index 263 169
    "hub": lambda: R.hub(20000, 6000),                      # one parent with 6000 children, many degree ties
    "ragged_sym": lambda: R.symmetric_part(R.ragged_lower(5000, empty_every=173)),  # unsorted rows, both kinds of isolated vertex
    "grid_63_isolated": lambda: R.with_isolated(R.grid2d(20), 63),  # exactly 64 components
}


@functools.lru_cache(maxsize=None)
def _bfs_case(name):
    return BFS_CASES[name]()


@functools.lru_cache(maxsize=None)
def _bfs_ref(name, rcm):
    return R.queue_order(_bfs_case(name), rcm)


@pytest.mark.parametrize("rcm", [False, True], ids=["bfs", "rcm"])
@pytest.mark.parametrize("name", list(BFS_CASES))
def test_bfs_rcm_equals_sequential_queue(ctx, name, rcm):
    A = _bfs_case(name)
    dA = _matrix(ctx, A)
    perm = ctx.bfs_order(dA, rcm)
    assert np.array_equal(perm, _bfs_ref(name, rcm))
    dB = ctx.permute(dA, perm)
    _same_matrix(dB, permute_crs(A, perm), ctx.rp_width)
    dA.free(); dB.free()


@pytest.mark.parametrize("rcm", [False, True], ids=["bfs", "rcm"])
def test_bfs_refuses_65_components_and_goes_on(ctx, rcm):
    from basic_iterative_solvers_amd import BisError
    dA = _matrix(ctx, R.with_isolated(R.grid2d(20), 64))
    with pytest.raises(BisError, match="more than 64 connected components"):
        ctx.bfs_order(dA, rcm)
    dA.free()
    A = R.grid2d(20)
    assert np.array_equal(ctx.bfs_order(_matrix(ctx, A), rcm), R.queue_order(A, rcm))


@functools.lru_cache(maxsize=None)
def _banded(n):
    return R.banded_sym(n, 2, 40)


@pytest.mark.parametrize("n,kind", [(N1, "random"), (N2, "random"), (N1, "reversal"), (0, "empty")])
def test_permute_equals_host_permutation(ctx, n, kind):
    A = _banded(n) if n else CRS(0, [0], [], [])
    perm = (np.random.default_rng(n).permutation(n) if kind == "random" else np.arange(n)[::-1]).astype(np.int32)
    dA = _matrix(ctx, A)
    dB = ctx.permute(dA, perm)
    assert dB.n_rows == n
    _same_matrix(dB, permute_crs(A, perm), ctx.rp_width)
    dA.free(); dB.free()


@pytest.mark.parametrize("defect", ["entry_n", "minus_one", "repeat"])
def test_permute_refuses_what_is_no_permutation(ctx, defect):
    from basic_iterative_solvers_amd import BisError
    perm = np.random.default_rng(4).permutation(N1).astype(np.int32)
    perm[40000] = {"entry_n": N1, "minus_one": -1, "repeat": perm[123]}[defect]
    dA = _matrix(ctx, _banded(N1))
    with pytest.raises(BisError, match="not a permutation"):
        ctx.permute(dA, perm)
    dA.free()


# ---- gather / scatter --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256, 257, 524288, N2])
def test_gather_scatter(vctx, n):
    rng = np.random.default_rng(n)
    v = rng.uniform(-1, 1, n)
    perm = rng.permutation(n).astype(np.int32)
    dv, out, back = vctx.upload(v), vctx.upload(np.full(n, np.nan)), vctx.upload(np.full(n, np.nan))
    vctx.gather(out, dv, perm)
    assert np.array_equal(out.to_host(), v[perm])
    vctx.scatter(back, out, perm)  # scatter after gather is the identity
    assert np.array_equal(back.to_host(), v)
    want = np.empty(n)
    want[perm] = v
    out.set(np.full(n, np.nan))
    vctx.scatter(out, dv, perm)
    assert np.array_equal(out.to_host(), want)
    for d in (dv, out, back):
        d.free()


def test_gather_scatter_refuse_in_place(vctx):
    from basic_iterative_solvers_amd import BisError
    v = vctx.upload(np.arange(8.0))
    perm = np.arange(8, dtype=np.int32)[::-1]
    with pytest.raises(BisError, match="bis_vec_gather: bad arguments"):
        vctx.gather(v, v, perm)
    with pytest.raises(BisError, match="bis_vec_scatter: bad arguments"):
        vctx.scatter(v, v, perm)
    assert np.array_equal(v.to_host(), np.arange(8.0))


# ---- -scale ------------------------------------------------------------------------------------------------------------

def _diag_index(A):
    rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
    return np.flatnonzero(A.col == rows)


def _edit(A, fn):
    """A with fn(r, cols, vals) applied to every row's lists."""
    rows, vals = R._rows_of(A)
    for r in range(A.n_rows):
        fn(r, rows[r], vals[r])
    return R._from_rows(rows, vals)


def _scale_input(kind, n):
    A = _banded(n)
    A = CRS(n, A.row_ptr.copy(), A.col.copy(), A.val.copy())
    d = _diag_index(A)
    rng = np.random.default_rng(n + 17)
    if kind == "negative":
        A.val[d] = -A.val[d]
    elif kind == "mixed_sign":
        A.val[d] *= rng.choice([-1.0, 1.0], n)
    elif kind == "twice":  # every 3rd row stores its diagonal a second time, behind the other entries: that value counts
        def twice(r, cols, vals):
            if r % 3 == 0:
                cols.append(r)
                vals.append(-(3.0 + r % 5))
        A = _edit(A, twice)
    elif kind == "no_diag":  # every 7th row stores no diagonal
        def drop(r, cols, vals):
            if r % 7 == 0:
                k = cols.index(r)
                del cols[k], vals[k]
        A = _edit(A, drop)
    elif kind == "tiny_accepted":
        A.val[d[n // 2]] = -1e-16
    else:
        raise KeyError(kind)
    return A


@pytest.mark.parametrize("n", [257, N1])
@pytest.mark.parametrize("kind,init", [("negative", 0.0), ("mixed_sign", 0.0), ("twice", 0.0), ("no_diag", 0.0),
                                       ("no_diag", 0.5), ("tiny_accepted", 0.0)])
def test_scale_sym_edges(ctx, oracle, kind, init, n):
    """bis_mat_scale_sym against scale_ref, and against extract_scale + scale_mat of the oracle where the oracle can
    express the input (it starts from s = 0): scale vector and scaled values bit for bit, then the SpMV on the scaled matrix."""
    A = _scale_input(kind, n)
    s_ref, val_ref, bad = R.scale_ref(A, init)
    assert bad == -1
    if init == 0.0:
        O = CRS(n, A.row_ptr.copy(), A.col.copy(), A.val.copy())
        s_orc, st = oracle.extract_scale(O)
        assert st == 0
        oracle.scale_mat(O, s_orc)
        assert np.array_equal(s_orc, s_ref) and np.array_equal(O.val, val_ref)
    if kind == "tiny_accepted":
        assert s_ref[n // 2] == 1e8
    if kind == "twice":
        assert s_ref[3] == 1.0 / np.sqrt(3.0 + 3 % 5)
    if kind == "no_diag":
        assert s_ref[7] == init
    dA = _matrix(ctx, A)
    s_dev = ctx.scale_sym(dA, init)
    assert np.array_equal(s_dev.to_host(), s_ref)
    S = CRS(n, A.row_ptr, A.col, val_ref)
    _same_matrix(dA, S, ctx.rp_width)
    _spmv_on(ctx, dA, S, 8)
    dA.free(); s_dev.free()


def test_scale_sym_reports_the_lowest_zero_row(ctx, oracle):
    """|a_rr| = 9.9e-17 at rows 700 and 300 (two different blocks): refused, and the row reported is the lowest one -- the
    row at which the sequential extract_scale stops (orc_extract_scale returns 1 + that row)."""
    from basic_iterative_solvers_amd import BisError
    A = _banded(1000)
    A = CRS(1000, A.row_ptr.copy(), A.col.copy(), A.val.copy())
    d = _diag_index(A)
    A.val[d[700]] = 9.9e-17
    A.val[d[300]] = -9.9e-17
    _, st = oracle.extract_scale(CRS(1000, A.row_ptr.copy(), A.col.copy(), A.val.copy()))
    assert st - 1 == 300 == R.scale_ref(A, 0.0)[2]
    dA = _matrix(ctx, A)
    with pytest.raises(BisError, match=r"Zero detected on diagonal at row index 300$"):
        ctx.scale_sym(dA)
    dA.free()
