"""CPU: the library exports the multi-vector sweep / preconditioner entry points (bis_sptrsm, bis_bsptrsm, bis_mitrsv,
bis_mvec_*_diag, bis_mapply_preconditioner, bis_mcg_set_preconditioner) and they refuse a null context like every other
entry point -- no CPU path."""
import ctypes

import pytest

NEW = ["bis_sptrsm", "bis_bsptrsm", "bis_mat_sweepm_kernel", "bis_mitrsv", "bis_mvec_div_diag", "bis_mvec_mul_diag",
       "bis_mapply_preconditioner", "bis_mcg_set_preconditioner"]


@pytest.fixture(scope="module")
def lib():
    from basic_iterative_solvers_amd import build
    return ctypes.CDLL(build.build())


@pytest.mark.parametrize("name", NEW)
def test_symbol_is_exported(lib, name):
    assert hasattr(lib, name)


def test_null_context_is_refused(lib):
    i, i64 = ctypes.c_int, ctypes.c_int64
    assert lib.bis_sptrsm(None, None, None, None, None, i(4)) == 1  # BIS_ERR_NO_DEVICE
    assert lib.bis_bsptrsm(None, None, None, None, None, i(4)) == 1
    assert lib.bis_mitrsv(None, None, None, None, None, None, i(2), i(4)) == 1
    assert lib.bis_mvec_div_diag(None, None, None, None, i64(0), i(2)) == 1
    assert lib.bis_mvec_mul_diag(None, None, None, None, i64(0), i(2)) == 1
    assert lib.bis_mapply_preconditioner(None, i(7), i64(0), i(4), None, None, None, None, None, None, None, None, None, None,
                                         i(1), i(0)) == 1
    assert lib.bis_mcg_set_preconditioner(None, None, i(7), None, None, None, None, None, None, i(1), i(0)) == 1
    lib.bis_mat_sweepm_kernel.restype = ctypes.c_char_p
    assert lib.bis_mat_sweepm_kernel(None, i(0)) == b""
    assert lib.bis_mat_sweepm_kernel(None, i(1)) == b""


def test_python_layer_has_the_multi_vector_sweep_surface():
    import basic_iterative_solvers_amd as bis
    for name in ("sptrsm", "bsptrsm", "mitrsv", "mvec_div_diag", "mvec_mul_diag", "mapply_preconditioner"):
        assert callable(getattr(bis.Context, name))
    assert callable(bis.Mat.sweepm_kernel)
    assert callable(bis.MCG.set_preconditioner)
