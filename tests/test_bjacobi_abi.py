"""CPU: the library exports the block-Jacobi entry points (bis_bj_*), those that take a context refuse a null one -- no CPU
path -- and leave their out-parameters alone, the header declares them with the preconditioner type
BIS_PC_BLOCK_JACOBI = 11, and the Python layer carries the type, Context.bjacobi and the BJ class.

The numpy restatement of the header's definitions (tests/bjacobi_ref.py, which the GPU test compares the device with bit for
bit) is checked here against numpy.linalg.inv: on random blocks of every size 1..32, half of them with a strengthened
diagonal, the residual ||R B - I||_inf of the restated Gauss-Jordan inverse was at most 3.2 times numpy's on this project's
CPU run (20 seeds a size; docs/EXPERIMENTS.md section 28); the test allows 8 times, numpy's residual taken as at least
m 2^-52 so that an exact numpy inverse does not make the bound zero."""
import ctypes
import os
import re

import numpy as np
import pytest

import bjacobi_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["bis_bj_create", "bis_bj_destroy", "bis_bj_apply", "bis_bj_mapply", "bis_bj_operand", "bis_bj_info", "bis_bj_blocks"]
FACTOR = 8.0


@pytest.fixture(scope="module")
def lib():
    from basic_iterative_solvers_amd import build
    return ctypes.CDLL(build.build())


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "bis_hip.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_exported(lib, name):
    assert hasattr(lib, name)


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_declared(header, name):
    assert re.search(r"BIS_API\s+[\w\s\*]*\b" + name + r"\s*\(", header), name


def test_type_eleven_is_declared(header):
    assert re.search(r"\bBIS_PC_BLOCK_JACOBI\s*=\s*11\b", header)
    assert re.search(r"typedef\s+struct\s*\{[^}]*block_size[^}]*block_ptr[^}]*n_blocks[^}]*symmetrize[^}]*\}\s*bis_bj_params\s*;", header)


def test_null_context_is_refused(lib):
    out = ctypes.c_void_p()
    assert lib.bis_bj_create(None, None, None, ctypes.byref(out)) == 1  # BIS_ERR_NO_DEVICE
    assert not out
    assert lib.bis_bj_apply(None, None, None, None) == 1
    assert lib.bis_bj_mapply(None, None, None, None, 2) == 1
    assert lib.bis_bj_destroy(None, None) == 1
    vals = (ctypes.c_double * 2)(-7.0, -7.0)
    offs = (ctypes.c_int64 * 2)(-7, -7)
    assert lib.bis_bj_blocks(None, None, vals, offs) == 1 and list(vals) == [-7.0, -7.0] and list(offs) == [-7, -7]
    lib.bis_bj_operand.restype = ctypes.c_void_p
    assert lib.bis_bj_operand(None) is None
    nb = ctypes.c_int64(-7)
    assert lib.bis_bj_info(None, ctypes.byref(nb), None, None) == 2 and nb.value == -7  # BIS_ERR_INVALID


def test_python_layer_has_bj():
    import basic_iterative_solvers_amd as bis
    assert bis.PC["bj"] == 11
    assert callable(bis.Context.bjacobi)
    for name in ("apply", "mapply", "info", "blocks", "free"):
        assert callable(getattr(bis.BJ, name)), name
    assert [f[0] for f in bis.BJParams._fields_] == ["block_size", "block_ptr", "n_blocks", "symmetrize"]


def residual(R, B):
    return float(np.abs(R @ B - np.eye(len(B))).sum(axis=1).max())


@pytest.mark.parametrize("m", range(1, 33))
def test_restated_inverse_against_numpy(m):
    worst = 0.0
    for seed in range(20):
        rng = np.random.default_rng(1000 * m + seed)
        B = rng.uniform(-1, 1, (m, m))
        if seed % 2:
            B += np.diag(rng.uniform(1, 2, m)) * m ** 0.5
        R = ref.invert(B)
        assert R is not None
        mine, theirs = residual(R, B), max(residual(np.linalg.inv(B), B), m * 2.0 ** -52)
        worst = max(worst, mine / theirs)
        assert mine <= FACTOR * theirs, (m, seed, mine, theirs)
    print(f"m = {m}: worst residual ratio over numpy.linalg.inv {worst:.2f}")


def test_permutation_and_a_swap_at_every_step():
    P = np.array([[0.0, 1.0], [1.0, 0.0]])
    assert np.array_equal(ref.invert(P), P)
    m = 6
    B = 1e-3 * np.random.default_rng(1).uniform(-1, 1, (m, m))
    for i in range(m):
        B[i, (i + 1) % m] = i + 2.0  # the largest entry of column k sits below row k at every step but the last
    swaps = 0
    T = B.copy()
    for k in range(m - 1):  # (plain elimination, to count the swaps the input forces)
        p = k + int(np.argmax(np.abs(T[k:, k])))
        swaps += p != k
        T[[k, p]] = T[[p, k]]
        T[k + 1:] -= np.outer(T[k + 1:, k] / T[k, k], T[k])
    assert swaps == m - 1
    R = ref.invert(B)
    assert residual(R, B) <= FACTOR * max(residual(np.linalg.inv(B), B), m * 2.0 ** -52)


def test_singular_blocks_are_reported():
    assert ref.invert(np.array([[1.0, 2.0], [2.0, 4.0]])) is None
    assert ref.invert(np.zeros((1, 1))) is None
    assert ref.invert(np.array([[np.nan]])) is None
    B = np.random.default_rng(2).uniform(-1, 1, (5, 5))
    B[3] = B[1] * 2.0  # an exact multiple: the elimination leaves a zero row
    assert ref.invert(B) is None


def test_extraction_sums_repeated_entries_in_storage_order_and_ignores_the_rest():
    from oracle.pyoracle import CRS
    # rows 0..2, blocks {0, 1}, {2}: row 0 holds column 1 three times, and column 2 outside its block
    rp = np.array([0, 5, 6, 8], dtype=np.int64)
    col = np.array([1, 0, 1, 2, 1, 1, 0, 2], dtype=np.int32)
    val = np.array([1e16, 3.0, 1.0, 99.0, -1e16, 2.0, 98.0, 5.0])
    blocks = ref.extract(CRS(3, rp, col, val), np.array([0, 2, 3]))
    assert np.array_equal(blocks[0], np.array([[3.0, ((0.0 + 1e16) + 1.0) + -1e16], [0.0, 2.0]]))
    assert np.array_equal(blocks[1], np.array([[5.0]]))


def test_restated_apply_rounds_every_product_and_sum():
    from oracle.pyoracle import CRS
    B = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, 0.25], [0.5, 0.25, 2.0]])
    rp = np.array([0, 3, 6, 9], dtype=np.int64)
    A = CRS(3, rp, np.tile(np.arange(3, dtype=np.int32), 3), B.ravel())
    bj = ref.BlockJacobi(A, block_size=3, symmetrize=True)
    R = bj.blocks[0]
    assert np.array_equal(R, R.T)
    x = np.array([0.1, -0.7, 1e-3])
    want = np.array([(R[i, 0] * x[0] + R[i, 1] * x[1]) + R[i, 2] * x[2] for i in range(3)])
    assert np.array_equal(bj.apply(x), want)
    X = np.stack([x, 3.0 * x], axis=1)
    out = bj.apply(X)
    assert np.array_equal(out[:, 0], want) and np.array_equal(out[:, 1], bj.apply(3.0 * x))
