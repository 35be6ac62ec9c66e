"""CPU: the library exports the flexible GMRES entry points (bis_fgmres_*), they refuse a null context like every other
entry point -- no CPU path -- and leave their out-parameters alone, and the Python layer carries the class."""
import ctypes

import pytest

SYMBOLS = ["bis_fgmres_create", "bis_fgmres_set_preconditioner", "bis_fgmres_init", "bis_fgmres_iterate", "bis_fgmres_solution",
           "bis_fgmres_status", "bis_fgmres_destroy"]


@pytest.fixture(scope="module")
def lib():
    from basic_iterative_solvers_amd import build
    return ctypes.CDLL(build.build())


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_exported(lib, name):
    assert hasattr(lib, name)


def test_null_context_is_refused(lib):
    h = ctypes.c_void_p()
    assert lib.bis_fgmres_create(None, None, None, None, ctypes.c_int(10), ctypes.byref(h)) == 1 and not h  # BIS_ERR_NO_DEVICE
    for pc in (4, 5, 10):  # also the types the lock-step handle refuses
        assert lib.bis_fgmres_set_preconditioner(None, None, ctypes.c_int(pc), None, None, None, None, None, None,
                                                 ctypes.c_int(1), ctypes.c_int(0)) == 1
    r0 = ctypes.c_double(-7.0)
    assert lib.bis_fgmres_init(None, None, ctypes.c_double(1e-8), ctypes.byref(r0)) == 1
    assert r0.value == -7.0
    assert lib.bis_fgmres_iterate(None, None, ctypes.c_int(1)) == 1
    assert lib.bis_fgmres_solution(None, None, None) == 1
    iters, conv, n_hist = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    hist = (ctypes.c_double * 4)(*([-7.0] * 4))
    assert lib.bis_fgmres_status(None, None, ctypes.byref(iters), ctypes.byref(conv), ctypes.byref(n_hist), hist,
                                 ctypes.c_int(4)) == 1
    assert (iters.value, conv.value, n_hist.value) == (-7, -7, -7) and list(hist) == [-7.0] * 4
    assert lib.bis_fgmres_destroy(None, None) == 1
    assert not h


def test_python_layer_has_the_flexible_gmres():
    import basic_iterative_solvers_amd as bis
    assert callable(bis.Context.fgmres)
    for name in ("set_preconditioner", "init", "iterate", "status", "solution", "free"):
        assert callable(getattr(bis.FGMRES, name))
