"""CPU: the library exports the lock-step BiCGSTAB entry points (bis_mbicgstab_*), they refuse a null context like every
other entry point -- no CPU path -- and the Python layer carries the class."""
import ctypes

import pytest

SYMBOLS = ["bis_mbicgstab_create", "bis_mbicgstab_set_preconditioner", "bis_mbicgstab_init", "bis_mbicgstab_iterate",
           "bis_mbicgstab_status", "bis_mbicgstab_destroy"]


@pytest.fixture(scope="module")
def lib():
    from basic_iterative_solvers_amd import build
    return ctypes.CDLL(build.build())


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_exported(lib, name):
    assert hasattr(lib, name)


def test_null_context_is_refused(lib):
    h = ctypes.c_void_p()
    assert lib.bis_mbicgstab_create(None, None, None, None, ctypes.c_int(4), ctypes.byref(h)) == 1 and not h  # BIS_ERR_NO_DEVICE
    assert lib.bis_mbicgstab_set_preconditioner(None, None, ctypes.c_int(4), None, None, None, None, None, None,
                                                ctypes.c_int(1), ctypes.c_int(0)) == 1
    assert lib.bis_mbicgstab_init(None, None, ctypes.c_double(1e-8), None) == 1
    assert lib.bis_mbicgstab_iterate(None, None, ctypes.c_int(1)) == 1
    iters, conv = ctypes.c_int(-7), ctypes.c_int(-7)
    assert lib.bis_mbicgstab_status(None, None, ctypes.c_int(0), ctypes.byref(iters), ctypes.byref(conv), None, ctypes.c_int(0)) == 1
    assert (iters.value, conv.value) == (-7, -7)
    assert lib.bis_mbicgstab_destroy(None, None) == 1
    assert not h


def test_python_layer_has_the_lock_step_bicgstab():
    import basic_iterative_solvers_amd as bis
    assert callable(bis.Context.mbicgstab)
    for name in ("set_preconditioner", "init", "iterate", "status", "free"):
        assert callable(getattr(bis.MBiCGSTAB, name))
