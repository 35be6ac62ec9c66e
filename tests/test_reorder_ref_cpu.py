"""The references of reorder_ref.py checked by independent means, and the conditions the cases of test_gpu_reorder.py rely
on: the device code refuses more than 64 colours and more than 64 connected components, so every case meant to pass is
pinned here with its colour and component count -- a change of seed cannot turn a passing case into a refused one (or a
refused one into a passing one) unnoticed."""
import numpy as np
import pytest

import reorder_ref as R

N1 = 65836    # 257 blocks of 256 rows + 44: the second trip of the single-workgroup scans
N2 = 524588   # 2049 blocks + 44: past every grid cap


def _rows(A):
    return np.repeat(np.arange(A.n_rows, dtype=np.int64), np.diff(A.row_ptr))


def _proper(A, colour):
    """No stored entry couples two rows of one colour."""
    rows = _rows(A)
    off = rows != A.col
    return not np.any(colour[rows[off]] == colour[A.col[off]])


def _structurally_symmetric(A):
    M = A.to_scipy().copy()  # (to_scipy shares A's arrays; sum_duplicates sorts in place)
    M.data[:] = 1.0
    M.sum_duplicates()
    M.data[:] = 1.0
    return (M != M.T).nnz == 0


def test_queue_order_equals_scipy_bfs():
    from scipy.sparse.csgraph import breadth_first_order
    A = R.grid2d(257)
    assert A.n_rows == 66049
    want = breadth_first_order(A.to_scipy(), 0, directed=False, return_predecessors=False)
    assert np.array_equal(R.queue_order(A, False), want)


def test_queue_order_rcm_small_by_hand():
    # 0 - 1 - 2 and 3 - 4, vertex 5 alone: degrees 1 2 1 1 1 0.  Starts by (degree, index): 5, then 0 (-> 1 -> 2), then 3 (-> 4)
    A = R._from_rows([[0, 1], [0, 1, 2], [1, 2], [3, 4], [3, 4], []], [[1.0] * k for k in (2, 3, 2, 2, 2, 0)])
    assert R.queue_order(A, True).tolist() == [5, 0, 1, 2, 3, 4][::-1]
    assert R.queue_order(A, False).tolist() == [0, 1, 2, 3, 4, 5]
    assert R.n_components(A) == 3
    # a star 0 - {1, 2, 3, 4} with 1 - 2: RCM starts at 3 (degree 1), pops 0, whose children go by (degree, index): 4, 1, 2
    S = R._from_rows([[1, 2, 3, 4], [0, 2], [0, 1], [0], [0]], [[1.0] * k for k in (4, 2, 2, 1, 1)])
    assert R.queue_order(S, True).tolist() == [3, 0, 4, 1, 2][::-1]
    assert R.queue_order(S, False).tolist() == [0, 1, 2, 3, 4]


def _first_fit_brute(A):
    n = A.n_rows
    colour = np.full(n, -1)
    for r in range(n):
        used = {colour[c] for c in A.col[A.row_ptr[r]:A.row_ptr[r + 1]] if c < r}
        c = 0
        while c in used:
            c += 1
        colour[r] = c
    return colour


@pytest.mark.parametrize("build", [lambda: R.banded_sym(200, 2, 40), lambda: R.ragged_lower(200), lambda: R.unsym(200),
                                   lambda: R.clique_at(200, 60, 64)], ids=["banded", "ragged", "unsym", "clique"])
def test_greedy_colours_equals_brute_force_first_fit(build):
    A = build()
    assert A.n_rows == 200
    assert np.array_equal(R.greedy_colours(A), _first_fit_brute(A))


# (case, builder, colours needed, connected components or None where no BFS case uses it)
CASES = [
    ("banded_N1", lambda: R.banded_sym(N1, 2, 40), 6, None),
    ("banded_N2", lambda: R.banded_sym(N2, 2, 40), 6, None),
    ("path_N1", lambda: R.path(N1), 2, 1),
    ("ragged", lambda: R.ragged_lower(5000), 17, None),
    ("ragged_bfs", lambda: R.symmetric_part(R.ragged_lower(5000, empty_every=173)), None, 54),
    ("clique64", lambda: R.clique_at(1000, 224, 64), 64, 1),
    ("grid257", lambda: R.grid2d(257), 2, 1),
    ("grid513_tail", lambda: R.with_tail(R.grid2d(513), 3), 2, 2),
    ("hub", lambda: R.hub(20000, 6000), None, 1),
    ("grid_63_isolated", lambda: R.with_isolated(R.grid2d(20), 63), 2, 64),
]


@pytest.mark.parametrize("name,build,colours,components", CASES, ids=[c[0] for c in CASES])
def test_case_conditions(name, build, colours, components):
    A = build()
    colour = R.greedy_colours(A)
    assert _proper(A, colour), "greedy_colours is not a proper colouring on a symmetric pattern"
    assert colour.min() == 0 and len(np.unique(colour)) == colour.max() + 1
    assert colour.max() + 1 <= 64
    if colours is not None:
        assert colour.max() + 1 == colours
    if components is not None:
        from scipy.sparse.csgraph import connected_components
        M = A.to_scipy().copy()
        M.data[:] = 1.0
        assert connected_components(M, directed=False)[0] == R.n_components(A) == components
        assert components <= 64
        assert _structurally_symmetric(A)
        assert not any(len(set(c)) < len(c) for c in R._rows_of(A)[0]), "a repeated column: the BFS refuses the pattern"


def test_refused_cases_need_65():
    A = R.clique_at(1000, 224, 65)
    assert R.greedy_colours(A).max() + 1 == 65
    assert R.n_components(R.with_isolated(R.grid2d(20), 64)) == 65


def test_with_isolated_has_both_kinds():
    A = R.with_isolated(R.grid2d(20), 63)
    lens = np.diff(A.row_ptr)[400:]
    assert np.count_nonzero(lens == 0) == 31 and np.count_nonzero(lens == 1) == 32
    assert np.array_equal(A.col[A.row_ptr[400]:], 400 + 2 * np.arange(32))


def test_ragged_lower_is_what_it_says():
    A = R.ragged_lower(5000)
    rows, _ = R._rows_of(A)
    lower = [sum(1 for c in cs if c < r) for r, cs in enumerate(rows)]
    seen = set()
    have = [set(c) for c in rows]
    for r in range(200, 5000):  # (past the first 120 rows every row finds the candidates it asks for)
        if r % 53 == 0:
            assert rows[r] == [] and not any(r in h for h in have[max(0, r - 130):r + 130])
        elif r % 211 == 0:
            assert rows[r] == [r]
        else:
            want = R.RAGGED_COUNTS[r % 8]
            dup = 1 if (want and r % 11 == 0) else 0
            assert lower[r] == want + dup
            assert len(rows[r]) - len(have[r]) == dup
            assert (r in have[r]) == (r % 37 != 0)
            seen.add(want)
            assert all(r in have[c] for c in rows[r])  # every entry has its mirror
    assert seen == set(R.RAGGED_COUNTS)
    assert any(cs != sorted(cs) for cs in rows), "columns are meant to be unsorted"
    S = R.symmetric_part(A)
    assert _structurally_symmetric(S) and S.nnz == A.nnz - sum(len(c) - len(set(c)) for c in rows)
    srows, _ = R._rows_of(S)
    assert any(cs != sorted(cs) for cs in srows)
    assert any(cs == [] for cs in srows) and any(cs == [r] for r, cs in enumerate(srows))


def test_unsym_reference_colouring_couples_equal_colours():
    """On the unsymmetric pattern the colouring (lower entries only) gives two coupled rows the same colour somewhere;
    otherwise the GPU case on it would test nothing beyond the symmetric ones."""
    A = R.unsym(5000)
    assert not _structurally_symmetric(A)
    colour = R.greedy_colours(A)
    rows = _rows(A)
    off = rows != A.col
    assert np.count_nonzero(colour[rows[off]] == colour[A.col[off]]) >= 1
    full = R.banded_sym(5000, 2, 40)
    lower_full = np.count_nonzero(full.col < _rows(full))
    assert np.count_nonzero(A.col < rows) == lower_full - lower_full // 3
    assert np.count_nonzero(A.col >= rows) == np.count_nonzero(full.col >= _rows(full))


def test_scale_ref_by_hand():
    # row 0: diagonal stored twice (4 then 16: the later one wins); row 1: no diagonal; row 2: negative diagonal
    A = R._from_rows([[0, 1, 0], [0, 2], [2, 1]], [[4.0, 3.0, 16.0], [5.0, 7.0], [-0.25, 2.0]])
    s, val, bad = R.scale_ref(A, 0.5)
    assert bad == -1
    assert s.tolist() == [0.25, 0.5, 2.0]
    assert val.tolist() == [4.0 * 0.0625, 3.0 * 0.125, 16.0 * 0.0625, 5.0 * 0.125, 7.0 * 1.0, -0.25 * 4.0, 2.0 * 1.0]
    s0, val0, _ = R.scale_ref(A, 0.0)
    assert s0.tolist() == [0.25, 0.0, 2.0] and val0[1] == 0.0 and val0[3] == 0.0
    B = R._from_rows([[0], [1], [2], [3]], [[1e-16], [9.9e-17], [2.0], [-9.9e-17]])
    s, _, bad = R.scale_ref(B, 0.0)
    assert bad == 1 and s[0] == 1e8


def test_builders_are_seeded():
    a, b = R.banded_sym(3000, 2, 40), R.banded_sym(3000, 2, 40)
    assert np.array_equal(a.col, b.col) and np.array_equal(a.val, b.val)
    a, b = R.ragged_lower(600), R.ragged_lower(600)
    assert np.array_equal(a.col, b.col) and np.array_equal(a.val, b.val)
    assert not np.array_equal(R.banded_sym(3000, 2, 40, seed=2).col, R.banded_sym(3000, 2, 40).col)
