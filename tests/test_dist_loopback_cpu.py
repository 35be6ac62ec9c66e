"""The irregular-partition table of dist_loopback.py against the host planner bis_halo_plan (no device needed), and a
self-test of the numpy references the GPU tests of the row-partitioned layer rely on (test_gpu_dist_loopback.py)."""
import numpy as np
import pytest

import dist_loopback as L


@pytest.mark.parametrize("name", L.CASES)
def test_host_halo_plan_on_irregular_partitions(name):
    """bis_halo_plan == the numpy plan on every rank of every case: halo columns, per-owner counts and the interior run
    itself (not only its length), the first of several longest runs and a rank without rows included."""
    from basic_iterative_solvers_amd import halo_plan
    A, rs, _, _ = L.make_case(name)
    plans = L.case_plans(A, rs)
    L.check_case_property(name, A, rs, plans)
    P = len(rs) - 1
    for p in range(P):
        Al = L.local_rows(A, int(rs[p]), int(rs[p + 1]))
        halo, recv, interior = halo_plan(Al.n_rows, Al.row_ptr, Al.col, P, p, rs)
        r_halo, r_recv, r_int = plans[p]
        assert np.array_equal(halo, r_halo) and halo.dtype == np.int32, (name, p)
        assert np.array_equal(recv, r_recv), (name, p, recv, r_recv)
        assert (int(interior[0]), int(interior[1])) == r_int, (name, p, interior, r_int)
        assert int(recv.sum()) == len(halo)
        # the send lists routed from these plans lie inside the owner's rows
        sc, cols = L.send_lists([(h, r) for h, r, _ in plans], p)
        assert np.all((cols >= rs[p]) & (cols < rs[p + 1])) and int(sc[p]) == 0


def test_reference_plan_on_a_hand_made_partition():
    """The numpy plan itself, on rows small enough to read: duplicates, an empty peer between two owners, tied runs."""
    #  rank 1 owns rows 4..11 of 16; rank 2 has no rows; rank 3 owns 12..15
    rows = [[4, 0], [5], [12, 12, 3], [7], [8], [15, 9], [10], [11]]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    Al = L.CRS(8, rp, np.concatenate(rows), np.ones(rp[-1]), n_cols=16)
    halo, recv, interior = L.ref_halo_plan(Al, [0, 4, 12, 12, 16], 1)
    assert halo.tolist() == [0, 3, 12, 15] and recv.tolist() == [2, 0, 0, 2]
    assert interior == (3, 5)  # runs [1,2), [3,5), [6,8): the first of the two longest
    assert L.interior_runs(Al, [0, 4, 12, 12, 16], 1).tolist() == [0, 1, 2, 2]
    ren = L.ref_renumber(Al, halo, 4, 12)
    assert ren.col.tolist() == [0, 8, 1, 10, 10, 9, 3, 4, 11, 5, 6, 7] and ren.n_cols == 12


def test_reference_diag_and_block_on_hand_made_rows():
    rows = [[10, 3, 10], [11, 12], [0], [13, 13]]  # row block at global row 10
    vals = [[2.0, 5.0, 4.0], [0.0, 1.0], [7.0], [0.0, 3.0]]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    Al = L.CRS(4, rp, np.concatenate(rows), np.concatenate(vals), n_cols=20)
    D, Dinv, status = L.ref_diag(Al, 10)
    assert D[0] == 4.0 and Dinv[0] == 0.25 and D[3] == 3.0  # the last entry wins
    assert status == ("zero", 11)  # row 11's zero comes before row 12's missing diagonal
    Bk = L.ref_diag_block(Al, 10)
    assert Bk.row_ptr.tolist() == [0, 2, 4, 4, 6] and Bk.col.tolist() == [0, 0, 1, 2, 3, 3]
    assert Bk.val.tolist() == [2.0, 4.0, 0.0, 1.0, 0.0, 3.0]


def test_reference_spmv_bound_catches_a_dropped_term():
    A, rs, _, _ = L.make_case("untidy")
    x = np.random.default_rng(1).uniform(-1, 1, A.n_cols)
    y = L.spmv64(A, x)
    L.check_spmv_rows(y, A, x, "numpy")
    r = int(np.argmax(np.diff(A.row_ptr)))
    k = int(A.row_ptr[r])
    y[r] -= A.val[k] * x[A.col[k]]
    with pytest.raises(AssertionError):
        L.check_spmv_rows(y, A, x, "dropped")


@pytest.mark.parametrize("P", [2, 3])
def test_reference_pcg_on_the_replicated_world_solves_the_system(P, oracle):
    """The numpy PCG (none, Jacobi, block-Jacobi SGS) against a direct dense solve on a small replicated world, and the
    world's premises: A symmetric, every rank's rows the same up to the cyclic shift."""
    nl = 120
    A, A0, rs = L.replicated_world(P, nl, 80, seed=P)
    n = P * nl
    dense = np.zeros((n, n))
    np.add.at(dense, (L.row_index(A), A.col), A.val)
    assert np.array_equal(dense, dense.T)
    for p in range(1, P):  # block-circulant: rank p's rows are rank 0's, columns shifted by p blocks
        assert np.array_equal(np.roll(dense[p * nl:(p + 1) * nl], -p * nl, axis=1), dense[:nl])
    b = np.tile(np.random.default_rng(5).uniform(-1, 1, nl), P)
    x0 = np.tile(np.random.default_rng(6).uniform(-1, 1, nl), P)
    exact = np.linalg.solve(dense, b)
    diag = np.diag(dense).copy()
    blocks = [L.ref_diag_block(L.local_rows(A, p * nl, (p + 1) * nl), p * nl) for p in range(P)]
    for pc in ("none", "j", "sgs"):
        x, hist = L.ref_pcg(A, b, x0, L.make_minv(pc, oracle, blocks, diag, nl), 1e-13, 200)
        assert len(hist) - 1 < 200 and hist[-1] < 1e-13 * hist[0], (pc, len(hist))
        assert np.max(np.abs(x - exact)) <= 1e-11, pc
        assert same_on_every_rank(x, P)


def same_on_every_rank(v, P):
    parts = v.reshape(P, -1)
    return bool(np.all(np.abs(parts - parts[0]) <= 1e-12 * np.max(np.abs(v))))
