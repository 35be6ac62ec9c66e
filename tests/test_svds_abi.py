"""CPU: the library exports the singular-value entry points (bis_svds_*), the header declares them with its enums, they
refuse a null context like every other entry point -- no CPU path -- and leave their out-parameters alone, and the Python
layer carries the class."""
import ctypes
import os
import re

import pytest

SYMBOLS = ["bis_svds_create", "bis_svds_set_start", "bis_svds_init", "bis_svds_iterate", "bis_svds_op_begin", "bis_svds_op_end",
           "bis_svds_status", "bis_svds_vectors", "bis_svds_destroy"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bis_hip.h")


@pytest.fixture(scope="module")
def lib():
    from basic_iterative_solvers_amd import build
    return ctypes.CDLL(build.build())


@pytest.fixture(scope="module")
def header():
    with open(HEADER) as f:
        return f.read()


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_declared_and_exported(lib, header, name):
    assert re.search(r"BIS_API\s+bis_status\s+" + name + r"\s*\(", header)
    assert hasattr(lib, name)


def test_enums(header):
    assert "enum { BIS_SVDS_LM = 0, BIS_SVDS_SM = 1 };" in header
    assert ("enum { BIS_SVDS_LIVE = 0, BIS_SVDS_CONVERGED = 1, BIS_SVDS_INVARIANT = 2, BIS_SVDS_JACOBI = 3, BIS_SVDS_BAD_START = 4 };"
            in header)


def test_null_context_is_refused(lib):
    h = ctypes.c_void_p()
    assert lib.bis_svds_create(None, None, None, ctypes.c_int64(8), ctypes.c_int64(6), ctypes.c_int(2), ctypes.c_int(0),
                               ctypes.c_int(0), ctypes.byref(h)) == 1 and not h  # BIS_ERR_NO_DEVICE
    assert lib.bis_svds_set_start(None, None, None) == 1
    assert lib.bis_svds_init(None, None, ctypes.c_double(1e-10)) == 1
    assert lib.bis_svds_iterate(None, None, ctypes.c_int(1)) == 1
    inp, out, tr = ctypes.c_void_p(7), ctypes.c_void_p(7), ctypes.c_int(-7)
    assert lib.bis_svds_op_begin(None, None, ctypes.byref(inp), ctypes.byref(out), ctypes.byref(tr)) == 1
    assert (inp.value, out.value, tr.value) == (7, 7, -7)
    assert lib.bis_svds_op_end(None, None) == 1
    ints = [ctypes.c_int(-7) for _ in range(6)]
    sref = ctypes.c_double(-7.0)
    arrays = [(ctypes.c_double * 4)(*([-7.0] * 4)) for _ in range(4)]
    assert lib.bis_svds_status(None, None, *[ctypes.byref(i) for i in ints], ctypes.byref(sref), *arrays, ctypes.c_int(4)) == 1
    assert [i.value for i in ints] == [-7] * 6 and sref.value == -7.0 and all(list(a) == [-7.0] * 4 for a in arrays)
    assert lib.bis_svds_vectors(None, None, None, ctypes.c_int64(8), None, ctypes.c_int64(6)) == 1
    assert lib.bis_svds_destroy(None, None) == 1
    assert not h


def test_python_layer_has_svds():
    import basic_iterative_solvers_amd as bis
    assert callable(bis.Context.svds)
    assert bis.SVDS._sym == "svds" and issubclass(bis.SVDS, bis._Solver)
    for name in ("init", "iterate", "status", "vectors", "op_begin", "op_end", "solve", "set_start", "free"):
        assert callable(getattr(bis.SVDS, name))
    assert bis.SVDS.WHICH == {"LM": 0, "SM": 1}
