"""The row-partitioned layer (bis_dist.hip) in ONE process on irregular partitions: the device halo plan, the column
renumbering, the pack kernel, the three-range SpMV, bis_dist_dot, bis_mat_diag, bis_mat_diag_block and the distributed
fused CG, each rank of a partition run in turn against a loop-back transport (dist_loopback.py) and plain numpy
references.  tests/test_dist.py keeps the multi-process transport; this file holds the shapes that never occur in a
stencil cut into slabs: ranks without rows, without a halo, without interior rows, one-way coupling, skipped owners, tied
interior runs, untidy rows, more than 65 536 rows per rank (the chunk carry of the 256-block scan), 64-bit row pointers.

Among several interior runs of equal length the library's choice can be observed only on the host planner, which returns
the run (test_dist_loopback_cpu.py, and here through dist_host_plan); a bis_dist reports the run's length alone."""
import functools

import numpy as np
import pytest

import dist_loopback as L
from helpers import OptionScope

pytestmark = pytest.mark.gpu

NO_DIAG, ZERO_DIAG, INVALID = 5, 4, 2


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def case(name):
    A, rs, ranks, has_diag = L.make_case(name)
    plans = L.case_plans(A, rs)
    L.check_case_property(name, A, rs, plans)  # the input has the property the case is there for
    rng = np.random.default_rng(11)
    n = A.n_rows
    x = rng.uniform(-1, 1, n)
    # dot pairs: a generic one, and one whose products cancel in pairs (+w, -w): a dropped element shows at full size
    a1, b1 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    a2 = rng.uniform(1, 2, n)
    w = np.repeat(rng.uniform(1, 2, (n + 1) // 2), 2)[:n] * np.tile([1.0, -1.0], (n + 1) // 2)[:n]
    b2 = w / a2
    for v in (A.row_ptr, A.col, A.val, x, a1, b1, a2, b2):
        v.setflags(write=False)
    return A, rs, ranks, has_diag, plans, x, ((a1, b1), (a2, b2))


def status_of(err):
    """(status, text) of a BisError raised by Context.check."""
    head, _, text = str(err).partition(": ")
    return int(head.split()[1]), text


def check_diag(ctx, dA, Al, row0, tag):
    from basic_iterative_solvers_amd import BisError
    D_ref, Dinv_ref, status = L.ref_diag(Al, row0)
    if status is None:
        D, Dinv = ctx.mat_diag(dA, row0)
        assert L.same_bits(D.to_host(), D_ref) and L.same_bits(Dinv.to_host(), Dinv_ref), tag
        D.free()
        Dinv.free()
    else:  # (the untidy case has rows without entries: the lowest of them is named)
        with pytest.raises(BisError) as e:
            ctx.mat_diag(dA, row0)
        st, text = status_of(e.value)
        assert st == (ZERO_DIAG if status[0] == "zero" else NO_DIAG) and text.endswith(f"row index {status[1]}"), (tag, text)


def check_diag_block(ctx, dA, Al, row0, rp64, tag):
    ref = L.ref_diag_block(Al, row0)
    dB = ctx.diag_block(dA, row0)
    assert (dB.n_rows, dB.n_cols, dB.nnz) == (Al.n_rows, Al.n_rows, ref.nnz), tag
    if rp64:
        assert dB.rp_width == 8
    rp, col, val = dB.download()
    assert np.array_equal(rp, ref.row_ptr) and np.array_equal(col, ref.col) and L.same_bits(val, ref.val), tag
    dB.free()


def run_case(ctx, name, rp64=False):
    from basic_iterative_solvers_amd import Dist, halo_plan
    A, rs, ranks, _, plans, x, dot_pairs = case(name)
    P = len(rs) - 1
    routed = [(h, r) for h, r, _ in plans]
    for p in ranks:
        tag = f"{name} rank {p}"
        row0, row1 = int(rs[p]), int(rs[p + 1])
        nl = row1 - row0
        Al = L.local_rows(A, row0, row1)
        halo, recv, (a, b) = plans[p]
        h_halo, h_recv, h_int = halo_plan(nl, Al.row_ptr, Al.col, P, p, rs)
        assert np.array_equal(h_halo, halo) and np.array_equal(h_recv, recv) and (int(h_int[0]), int(h_int[1])) == (a, b), tag
        # ---- diagonal and diagonal block of the rows with their global columns
        dA2 = ctx.matrix(Al)
        if rp64:
            assert dA2.rp_width == 8
        check_diag(ctx, dA2, Al, row0, tag)
        check_diag_block(ctx, dA2, Al, row0, rp64, tag)
        dA2.free()
        # ---- plan
        dA = ctx.matrix(Al)
        if rp64:
            assert dA.rp_width == 8
        d = Dist(ctx, dA, p, P, rs)
        d_halo, d_recv = d.halo_info()
        assert np.array_equal(d_halo, halo) and np.array_equal(d_recv, recv), tag
        assert d.n_local == nl and d.n_ext == nl + len(halo), tag
        sc, scols = L.send_lists(routed, p)
        d.set_send_lists(sc, scols)
        tr = L.KnownVectorTransport(x, sc, scols, halo, recv)
        d.set_comm(tr.ops)
        st = d.stats()
        assert st["interior_rows"] == b - a and st["halo_entries"] == len(halo) and st["send_entries"] == int(sc.sum()), (tag, st)
        assert st["neighbours"] == int(np.count_nonzero((recv > 0) | (sc > 0))), (tag, st)
        # ---- SpMV: the halo tail and y start as NaN, so a missing exchange or an unwritten row range shows
        xe = np.full(d.n_ext, np.nan)
        xe[:nl] = x[row0:row1]
        x_ext, y = ctx.upload(xe), ctx.upload(np.full(nl, np.nan))
        with tr.checked():
            d.spmv(x_ext, y)
        exchanges = P > 1 and (int(sc.sum()) > 0 or len(halo) > 0)
        assert tr.log == (["x"] if exchanges else []), (tag, tr.log)
        assert all(tr.sendbuf_exact), f"{tag}: packed send buffer != x[send_cols]"
        L.check_spmv_rows(y.to_host(), L.ref_renumber(Al, halo, row0, row1), np.concatenate([x[row0:row1], x[halo]]), tag)
        # ---- dot: |got - exact| <= (n_local / 2 + 512) 2^-53 sum |a_i b_i| -- no lane's chain of the grid-stride
        # reduction is longer than half this rank's entries; the tree, the host's sum of the other ranks and the final
        # addition fit the 512
        for va, vb in dot_pairs:
            mine, _ = L.ref_dot(va[row0:row1], vb[row0:row1])
            exact, mag = L.ref_dot(va, vb)
            tr.others = float(exact - mine)
            da, db = ctx.upload(va[row0:row1]), ctx.upload(vb[row0:row1])
            with tr.checked():
                got = d.dot(da, db)
            assert abs(np.longdouble(got) - exact) <= (nl / 2 + 512) * L.U * mag, (tag, got, float(exact))
            da.free()
            db.free()
        assert tr.log[-2:] == [1, 1], tr.log
        x_ext.free()
        y.free()
        d.free()


@pytest.mark.parametrize("name", L.CASES)
def test_irregular_partition(ctx, name):
    run_case(ctx, name)


@pytest.mark.parametrize("name", ["all_to_all", "untidy", "long"])
def test_irregular_partition_rp64(ctx, name):
    """The RP = int64_t instances of the plan, diagonal and diagonal-block kernels (block_fill_kernel's RPO included)."""
    with OptionScope(ctx, force_rp64=1):
        run_case(ctx, name, rp64=True)


@pytest.mark.parametrize("name", ["ties", "all_boundary"])
def test_irregular_partition_host_plan(ctx, name):
    with OptionScope(ctx, dist_host_plan=1):
        run_case(ctx, name)


# ---- diagonal status word -------------------------------------------------------------------------------------------------

def diag_rows(n, row0, edits, seed=3):
    """A row block of n rows at global row row0: three entries per row, the diagonal in the middle; edits[r] replaces
    row r's (columns, values)."""
    rng = np.random.default_rng(seed)
    rows = [[(row0 + r + 7) % (row0 + n + 50), row0 + r, (r * 5) % row0] for r in range(n)]
    vals = [list(rng.uniform(1, 2, 3)) for _ in range(n)]
    for r, (c, v) in edits.items():
        rows[r], vals[r] = c, v
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])])
    return L.CRS(n, rp, np.concatenate(rows), np.concatenate(vals), n_cols=row0 + n + 50)


def diag_error(ctx, Al, row0):
    from basic_iterative_solvers_amd import BisError
    dA = ctx.matrix(Al)
    with pytest.raises(BisError) as e:
        ctx.mat_diag(dA, row0)
    dA.free()
    return status_of(e.value)


def test_mat_diag_status(ctx, oracle):
    n, row0 = 700, 1000
    # no diagonal on two rows of different blocks: the lower GLOBAL index is named
    Al = diag_rows(n, row0, {300: ([5, 6], [1.0, 2.0]), 70: ([row0 + 71], [3.0])})
    assert L.ref_diag(Al, row0)[2] == ("none", row0 + 70)
    assert diag_error(ctx, Al, row0) == (NO_DIAG, f"No diagonal to extract at row index {row0 + 70}")
    # a zero diagonal
    Al = diag_rows(n, row0, {500: ([row0 + 500, 3], [0.0, 1.0])})
    assert diag_error(ctx, Al, row0) == (ZERO_DIAG, f"Zero detected on diagonal at row index {row0 + 500}")
    # duplicate diagonal entries: the last wins, in D and in 1/D
    Al = diag_rows(n, row0, {4: ([row0 + 4, 9, row0 + 4, row0 + 4], [2.0, 1.0, -8.0, 4.0]), 699: ([row0 + 699, row0 + 699], [3.0, 0.5])})
    D_ref, Dinv_ref, status = L.ref_diag(Al, row0)
    assert status is None and D_ref[4] == 4.0 and D_ref[699] == 0.5
    dA = ctx.matrix(Al)
    D, Dinv = ctx.mat_diag(dA, row0)
    assert L.same_bits(D.to_host(), D_ref) and L.same_bits(Dinv.to_host(), Dinv_ref)
    dA.free()
    # an earlier duplicate is zero, the last is not.  The reference's peel_diag_crs tests every diagonal entry where it
    # meets it and calls SanityChecker::zero_diag at the zero one, before the later entry is seen: "Zero detected", not
    # the last value.  The kernel does the same.
    r = 333
    Al = diag_rows(n, row0, {r: ([row0 + r, 2, row0 + r], [0.0, 1.0, 5.0])})
    blk = L.ref_diag_block(Al, row0)  # (the reference extracts from a square matrix: the block with local columns)
    blk.val.setflags(write=True)
    assert oracle.peel_diag(blk)[2] == 1 + r  # the oracle's restatement: zero diagonal at row r
    assert L.ref_diag(Al, row0)[2] == ("zero", row0 + r)
    assert diag_error(ctx, Al, row0) == (ZERO_DIAG, f"Zero detected on diagonal at row index {row0 + r}")


# ---- argument errors ------------------------------------------------------------------------------------------------------

def test_argument_errors_leave_the_context_usable(ctx):
    from basic_iterative_solvers_amd import BisError, Dist
    A, rs, _, _, plans, x, _ = case("all_to_all")
    P, p = len(rs) - 1, 1
    row0, row1 = int(rs[p]), int(rs[p + 1])
    nl = row1 - row0
    Al = L.local_rows(A, row0, row1)
    halo, recv, _ = plans[p]
    sc, scols = L.send_lists([(h, r) for h, r, _ in plans], p)

    def refused(fn):
        with pytest.raises(BisError) as e:
            fn()
        st, text = status_of(e.value)
        assert st == INVALID and text, (st, text)

    def plain_spmv(dA):  # the context still works: one SpMV of the rows with their global columns
        dx, dy = ctx.upload(x), ctx.upload(np.full(nl, np.nan))
        ctx.spmv(dA, dx, dy)
        L.check_spmv_rows(dy.to_host(), Al, x, "after a refused call")
        dx.free()
        dy.free()

    dA = ctx.matrix(Al)
    shifted = rs.copy()
    shifted[p + 1] -= 1
    refused(lambda: Dist(ctx, dA, p, P, shifted))  # the row range does not match the matrix
    plain_spmv(dA)
    longer = rs.copy()
    longer[-1] += 5
    refused(lambda: Dist(ctx, dA, p, P, longer))  # n_cols != row_starts[-1]
    plain_spmv(dA)

    def dist_spmv(d, tr):
        xe = np.full(d.n_ext, np.nan)
        xe[:nl] = x[row0:row1]
        x_ext, y = ctx.upload(xe), ctx.upload(np.full(nl, np.nan))
        try:
            with tr.checked():
                d.spmv(x_ext, y)
            assert tr.log[-1] == "x" and tr.sendbuf_exact[-1], "the exchange got other lists than the last good call set"
            L.check_spmv_rows(y.to_host(), L.ref_renumber(Al, halo, row0, row1), np.concatenate([x[row0:row1], x[halo]]), "dist")
        finally:
            x_ext.free()
            y.free()

    d = Dist(ctx, dA, p, P, rs)
    tr = L.KnownVectorTransport(x, sc, scols, halo, recv)
    x_ext, y = ctx.alloc(d.n_ext), ctx.alloc(nl)
    refused(lambda: d.spmv(x_ext, y))  # P > 1 and no transport yet
    x_ext.free()
    y.free()
    d.set_send_lists(sc, scols)
    d.set_comm(tr.ops)
    dist_spmv(d, tr)
    # a column this rank does not own, with counts that differ from the good ones: nothing of the handle may change
    bad_cols = scols.copy()
    bad_cols[-1] = row1
    bad_counts = sc[::-1].copy()
    assert int(bad_counts.sum()) == int(sc.sum()) and not np.array_equal(bad_counts, sc)
    refused(lambda: d.set_send_lists(bad_counts, bad_cols))
    assert d.stats()["send_entries"] == int(sc.sum())
    dist_spmv(d, tr)
    d.free()


# ---- distributed CG on the replicated world -----------------------------------------------------------------------------------

CG_TOL = 1e-12  # the stopping test: well above the rounding floor, so that the iteration count is the algorithm's
CG_WORLDS = {2: 300, 3: 301}  # P -> last boundary row of the low group: the interior run starts at 301 (odd) and 302


@functools.lru_cache(maxsize=None)
def cg_world(P):
    from basic_iterative_solvers_amd import halo_plan
    from oracle.pyoracle import Oracle
    nl = 2001
    A, A0, rs = L.replicated_world(P, nl, CG_WORLDS[P], seed=40 + P)
    plans = []
    for q in range(P):
        Aq = L.local_rows(A, q * nl, (q + 1) * nl)
        plans.append(halo_plan(nl, Aq.row_ptr, Aq.col, P, q, rs))
    halo, recv, interior = plans[0]
    a, b = int(interior[0]), int(interior[1])
    assert 0 < a < b < nl and a == CG_WORLDS[P] + 1 and len(halo) > 0  # three non-empty row views
    assert abs(A0.nnz / nl - 9) < 2  # about 8 entries per row of B, the diagonal, a few of C
    sc, scols = L.send_lists([(h, r) for h, r, _ in plans], 0)
    rng = np.random.default_rng(P)
    b_loc, x0_loc = rng.uniform(-1, 1, nl), rng.uniform(-1, 1, nl)
    rows = L.row_index(A)
    diag = np.zeros(P * nl)
    diag[rows[A.col == rows]] = A.val[A.col == rows]
    blocks = [L.ref_diag_block(L.local_rows(A, q * nl, (q + 1) * nl), q * nl) for q in range(P)]
    orc = Oracle()
    refs = {}
    for pc in ("none", "j", "sgs"):
        xr, hist = L.ref_pcg(A, np.tile(b_loc, P), np.tile(x0_loc, P), L.make_minv(pc, orc, blocks, diag, nl), CG_TOL, 200)
        assert len(hist) - 1 < 100 and hist[-1] < CG_TOL * hist[0], (pc, len(hist))  # converges in well under 200
        refs[pc] = (xr[:nl], hist)
    return A0, rs, halo, sc, scols, b_loc, x0_loc, refs


@pytest.mark.parametrize("rp64", [False, True], ids=["rp32", "rp64"])
@pytest.mark.parametrize("pc", ["none", "j", "sgs"])
@pytest.mark.parametrize("P", [2, 3])
def test_dist_cg_replicated_world(ctx, P, pc, rp64):
    """bis_dist_cg_* on rank 0 of a block-circulant world whose ranks all hold the same vectors, against the global numpy
    PCG (block-Jacobi for sgs); tolerances of tests/dist_worker.py."""
    from basic_iterative_solvers_amd import Dist
    A0, rs, halo, sc, scols, b_loc, x0_loc, refs = cg_world(P)
    x_ref, h_ref = refs[pc]
    nl = A0.n_rows
    with OptionScope(ctx, **({"force_rp64": 1} if rp64 else {})):
        dA2 = ctx.matrix(A0)
        d = Dist(ctx, ctx.matrix(A0), 0, P, rs)
        assert dA2.rp_width == (8 if rp64 else 4)
        assert np.array_equal(d.halo_info()[0], halo)
        d.set_send_lists(sc, scols)
        tr = L.ReplicatedWorldTransport(P, nl, halo, rs, scols)
        d.set_comm(tr.ops)
        bv, xv = ctx.upload(b_loc), ctx.upload(x0_loc)
        keep = []
        if pc == "j":
            D, Dinv = ctx.mat_diag(dA2, 0)
            keep += [D, Dinv]
            cg = d.cg(bv, xv, D)
        else:
            cg = d.cg(bv, xv)
        if pc == "sgs":  # SGS of the rank's diagonal block, set up as tests/dist_worker.py does
            dAb = ctx.diag_block(dA2, 0)
            assert dAb.rp_width == (8 if rp64 else 4)
            fLs, fUs, fD, fDinv = ctx.split_strict(dAb)
            ones = ctx.upload(np.ones(nl))
            keep += [dAb, fLs, fUs, fD, fDinv, ones]
            cg.set_preconditioner("sgs", Ls=fLs, Us=fUs, A_D=fD, A_D_inv=fDinv, L_D=ones, U_D=ones)
        n_it = len(h_ref) - 1 + 2
        with tr.checked():
            r0 = cg.init(CG_TOL)
            cg.iterate(n_it)
            iters, conv, hist = cg.status()
        x = xv.to_host()
        cg.free()
        for v in keep + [bv, xv, dA2]:
            v.free()
        d.free()
    m = min(len(hist), len(h_ref))
    dev = float(np.max(np.abs(hist[:m] - h_ref[:m])) / h_ref[0])
    print(f"P={P} {pc}: {iters} iterations (reference {len(h_ref) - 1}), history deviation {dev:.2e} r0, "
          f"max |x - x_ref| {np.max(np.abs(x - x_ref)):.2e}")
    assert abs(r0 - h_ref[0]) <= 1e-10 * h_ref[0]
    assert conv and dev <= 1e-10 and abs(iters - (len(h_ref) - 1)) <= 1, (conv, dev, iters, len(h_ref) - 1)
    assert np.max(np.abs(x - x_ref)) <= 1e-9
    # one exchange per SpMV; the all-reduces in the order bis_cg.hip issues them: (r,z) and (r,r) at init, then per
    # enqueued iteration (Ap,p) and the batched {(r,z), (r,r)}
    assert tr.log == ["x", 1, 1] + ["x", 1, 2] * n_it, tr.log[:12]
    assert all(tr.sendbuf_exact)
