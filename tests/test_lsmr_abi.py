"""CPU: the library exports the LSMR entry points (bis_lsmr_*, bis_mat_row_norms), they refuse a null context like every
other entry point -- no CPU path -- and leave their out-parameters alone, and the Python layer carries the class."""
import ctypes

import pytest

SYMBOLS = ["bis_lsmr_create", "bis_lsmr_set_damping", "bis_lsmr_set_col_scaling", "bis_lsmr_init", "bis_lsmr_iterate",
           "bis_lsmr_status", "bis_lsmr_destroy", "bis_mat_row_norms"]


@pytest.fixture(scope="module")
def lib():
    from basic_iterative_solvers_amd import build
    return ctypes.CDLL(build.build())


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_exported(lib, name):
    assert hasattr(lib, name)


def test_null_context_is_refused(lib):
    h = ctypes.c_void_p()
    assert lib.bis_lsmr_create(None, None, None, None, None, ctypes.byref(h)) == 1 and not h  # BIS_ERR_NO_DEVICE
    assert lib.bis_lsmr_set_damping(None, None, ctypes.c_double(0.5)) == 1
    assert lib.bis_lsmr_set_col_scaling(None, None, None) == 1
    r0, ar0 = ctypes.c_double(-7.0), ctypes.c_double(-7.0)
    assert lib.bis_lsmr_init(None, None, ctypes.c_double(1e-8), ctypes.c_double(1e-8), ctypes.byref(r0), ctypes.byref(ar0)) == 1
    assert (r0.value, ar0.value) == (-7.0, -7.0)
    assert lib.bis_lsmr_iterate(None, None, ctypes.c_int(1)) == 1
    iters, conv, reason = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    hist = (ctypes.c_double * 4)(*([-7.0] * 4))
    hist_r = (ctypes.c_double * 4)(*([-7.0] * 4))
    assert lib.bis_lsmr_status(None, None, ctypes.byref(iters), ctypes.byref(conv), ctypes.byref(reason), hist, hist_r,
                               ctypes.c_int(4)) == 1
    assert (iters.value, conv.value, reason.value) == (-7, -7, -7) and list(hist) == [-7.0] * 4 and list(hist_r) == [-7.0] * 4
    assert lib.bis_lsmr_destroy(None, None) == 1
    assert lib.bis_mat_row_norms(None, None, None) == 1
    assert lib.bis_lsmr_scaling_from_norms(None, None, ctypes.c_int64(4), None) == 1
    assert not h


def test_python_layer_has_lsmr():
    import basic_iterative_solvers_amd as bis
    assert callable(bis.Context.lsmr) and callable(bis.Mat.row_norms)
    assert bis.LSMR._sym == "lsmr" and issubclass(bis.LSMR, bis._Solver)
    for name in ("init", "iterate", "status", "free", "set_damping", "set_col_scaling"):
        assert callable(getattr(bis.LSMR, name))
