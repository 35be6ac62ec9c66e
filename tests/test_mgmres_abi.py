"""CPU: the library exports the lock-step GMRES entry points (bis_mgmres_*), they refuse a null context like every other
entry point -- no CPU path -- and leave their out-parameters alone, and the Python layer carries the class."""
import ctypes

import pytest

SYMBOLS = ["bis_mgmres_create", "bis_mgmres_set_preconditioner", "bis_mgmres_init", "bis_mgmres_iterate", "bis_mgmres_solution",
           "bis_mgmres_status", "bis_mgmres_destroy"]


@pytest.fixture(scope="module")
def lib():
    from basic_iterative_solvers_amd import build
    return ctypes.CDLL(build.build())


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_exported(lib, name):
    assert hasattr(lib, name)


def test_null_context_is_refused(lib):
    h = ctypes.c_void_p()
    assert lib.bis_mgmres_create(None, None, None, None, ctypes.c_int(4), ctypes.c_int(10), ctypes.byref(h)) == 1 and not h  # BIS_ERR_NO_DEVICE
    assert lib.bis_mgmres_set_preconditioner(None, None, ctypes.c_int(4), None, None, None, None, None, None,
                                             ctypes.c_int(1), ctypes.c_int(0)) == 1
    r0 = (ctypes.c_double * 8)(*([-7.0] * 8))
    assert lib.bis_mgmres_init(None, None, ctypes.c_double(1e-8), r0) == 1
    assert list(r0) == [-7.0] * 8
    assert lib.bis_mgmres_iterate(None, None, ctypes.c_int(1)) == 1
    assert lib.bis_mgmres_solution(None, None, None) == 1
    iters, conv, n_hist = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    hist = (ctypes.c_double * 4)(*([-7.0] * 4))
    assert lib.bis_mgmres_status(None, None, ctypes.c_int(0), ctypes.byref(iters), ctypes.byref(conv), ctypes.byref(n_hist), hist,
                                 ctypes.c_int(4)) == 1
    assert (iters.value, conv.value, n_hist.value) == (-7, -7, -7) and list(hist) == [-7.0] * 4
    assert lib.bis_mgmres_destroy(None, None) == 1
    assert not h


def test_python_layer_has_the_lock_step_gmres():
    import basic_iterative_solvers_amd as bis
    assert callable(bis.Context.mgmres)
    for name in ("set_preconditioner", "init", "iterate", "status", "solution", "free"):
        assert callable(getattr(bis.MGMRES, name))
