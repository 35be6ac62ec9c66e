"""CPU: the library declares and exports the IDR(s) entry points (bis_idr_*), they refuse a null context like every other
entry point -- no CPU path -- and leave their out-parameters alone, and the Python layer carries the class."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["bis_idr_create", "bis_idr_set_preconditioner", "bis_idr_set_shadow", "bis_idr_init", "bis_idr_iterate",
           "bis_idr_status", "bis_idr_destroy"]


@pytest.fixture(scope="module")
def lib():
    from basic_iterative_solvers_amd import build
    return ctypes.CDLL(build.build())


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_declared_and_exported(lib, name):
    header = open(os.path.join(ROOT, "include", "bis_hip.h")).read()
    assert re.search(r"BIS_API\s+bis_status\s+" + name + r"\s*\(", header), name
    assert hasattr(lib, name)


def test_null_context_is_refused(lib):
    h = ctypes.c_void_p()
    for s in (0, 4, 9):
        assert lib.bis_idr_create(None, None, None, None, ctypes.c_int(s), ctypes.byref(h)) == 1 and not h  # BIS_ERR_NO_DEVICE
    for pc in (0, 1, 7, 10, 11, 12):
        assert lib.bis_idr_set_preconditioner(None, None, ctypes.c_int(pc), None, None, None, None, None, None,
                                              ctypes.c_int(1), ctypes.c_int(0)) == 1
    P = (ctypes.c_double * 4)(*([-7.0] * 4))
    assert lib.bis_idr_set_shadow(None, None, P) == 1 and list(P) == [-7.0] * 4
    r0 = ctypes.c_double(-7.0)
    assert lib.bis_idr_init(None, None, ctypes.c_double(1e-8), ctypes.byref(r0)) == 1
    assert r0.value == -7.0
    assert lib.bis_idr_iterate(None, None, ctypes.c_int(1)) == 1
    iters, conv = ctypes.c_int(-7), ctypes.c_int(-7)
    hist = (ctypes.c_double * 4)(*([-7.0] * 4))
    assert lib.bis_idr_status(None, None, ctypes.byref(iters), ctypes.byref(conv), hist, ctypes.c_int(4)) == 1
    assert (iters.value, conv.value) == (-7, -7) and list(hist) == [-7.0] * 4
    assert lib.bis_idr_destroy(None, None) == 1
    assert not h


def test_python_layer_has_idr():
    import basic_iterative_solvers_amd as bis
    assert callable(bis.Context.idr)
    assert bis.IDR._sym == "idr" and issubclass(bis.IDR, bis._Solver)
    for name in ("set_preconditioner", "set_shadow", "init", "iterate", "status", "free"):
        assert callable(getattr(bis.IDR, name))
