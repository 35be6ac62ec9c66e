"""CPU: the library exports the ILU(k) entry points, the header declares them, those that take a context refuse a null one
and leave their out-parameters alone, bis_iluk_limits answers without a device, and the Python layer carries the calls.

The two restatements of the symbolic phase in tests/iluk_ref.py -- the textbook sum rule and the two breadth-first searches
the device runs (fill-path theorem, Hysom & Pothen) -- are compared on seeded random patterns, structurally symmetric and
not, for k = 0, 1, 2, 3, 5; the GPU test compares the device with the second."""
import ctypes
import os
import re

import numpy as np
import pytest

import iluk_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["bis_mat_iluk_symbolic", "bis_mat_iluk", "bis_mat_iluk_kernel", "bis_iluk_limits"]


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


def test_limits_need_no_device(lib):
    ml, mv = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.bis_iluk_limits(ctypes.byref(ml), ctypes.byref(mv)) == 0
    assert ml.value == 16 and mv.value >= 4096  # levels fit a byte; the issue's floor for the table
    assert lib.bis_iluk_limits(None, None) == 0


def test_null_context_is_refused(lib):
    out, out2 = ctypes.c_void_p(), ctypes.c_void_p()
    nf = ctypes.c_int64(-7)
    assert lib.bis_mat_iluk_symbolic(None, None, 1, ctypes.byref(out), ctypes.byref(nf)) == 1  # BIS_ERR_NO_DEVICE
    assert not out and nf.value == -7
    for level in (0, 1):
        assert lib.bis_mat_iluk(None, None, level, ctypes.c_double(1e-8), ctypes.c_double(1e-4), ctypes.byref(out),
                                ctypes.byref(out2), None, None, ctypes.byref(nf)) == 1
        assert not out and not out2 and nf.value == -7
    lib.bis_mat_iluk_kernel.restype = ctypes.c_char_p
    assert lib.bis_mat_iluk_kernel(None) == b""


def test_python_layer_has_iluk():
    import basic_iterative_solvers_amd as bis
    assert callable(bis.Context.iluk) and callable(bis.Context.iluk_symbolic) and callable(bis.Mat.iluk_kernel)
    assert bis.iluk_limits() == (16, 4096)


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("seed", range(6))
def test_the_two_formulations_agree(seed, symmetric):
    A = ref.random_pattern(40, 0.06, symmetric, 5200 + seed)
    for k in (0, 1, 2, 3, 5):
        assert ref.symbolic_sum_rule(A, k) == ref.symbolic_two_search(A, k), (seed, symmetric, k)


def test_level_zero_is_the_pattern_and_levels_nest():
    A = ref.random_pattern(40, 0.06, False, 77)
    rp = A.row_ptr
    lev0 = ref.symbolic_two_search(A, 0)
    assert [sorted(r) for r in lev0] == [sorted(int(c) for c in A.col[rp[i]:rp[i + 1]]) for i in range(40)]
    prev = lev0
    for k in (1, 2, 3):
        cur = ref.symbolic_two_search(A, k)
        for a, b in zip(prev, cur):
            assert all(b[j] == l for j, l in a.items())  # a level, once found, does not change with k
        prev = cur
    full = ref.symbolic_two_search(A, 40)
    P, n_fill = ref.padded(A, full)
    Ls, L_D, Us, U_D = ref.numeric(P)
    n = 40
    L = np.eye(n)
    U = np.diag(U_D)
    for M, F in ((L, Ls), (U, Us)):
        for i in range(n):
            M[i, F.col[F.row_ptr[i]:F.row_ptr[i + 1]]] = F.val[F.row_ptr[i]:F.row_ptr[i + 1]]
    D = np.zeros((n, n))
    for i in range(n):
        D[i, A.col[rp[i]:rp[i + 1]]] = A.val[rp[i]:rp[i + 1]]
    assert np.abs(L @ U - D).max() <= 1e-13 * np.abs(D).max() * n  # every level kept: the complete factorisation


def test_exact_fma_rounds_once():
    a, b, c = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -1.0
    assert ref.fma(a, b, c) == 2.0 ** -29 + 2.0 ** -60 and a * b + c == 2.0 ** -29
