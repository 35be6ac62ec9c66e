"""CPU: the library exports the sparse matrix-matrix product, the transpose and the smoothed-aggregation entry points, the
header declares them, they refuse a null context (BIS_ERR_NO_DEVICE) and leave their out-parameters alone, the limits are
the stated constants, and the Python layer carries Context.spgemm, Mat.transpose, spgemm_limits and the smoothed MG."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATUS = ["bis_spgemm", "bis_mat_transpose", "bis_spgemm_limits", "bis_mg_create_smoothed", "bis_mg_level_prolong_omega"]
POINTER = {"bis_spgemm_kernel": r"const\s+char\s*\*", "bis_mg_level_prolongator": r"const\s+bis_mat\s*\*",
           "bis_mg_level_restrictor": r"const\s+bis_mat\s*\*"}


@pytest.fixture(scope="module")
def lib():
    from basic_iterative_solvers_amd import build
    return ctypes.CDLL(build.build())


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "bis_hip.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", STATUS + list(POINTER))
def test_symbol_is_exported(lib, name):
    assert hasattr(lib, name)


@pytest.mark.parametrize("name", STATUS + list(POINTER))
def test_symbol_is_declared(header, name):
    ret = POINTER.get(name, r"bis_status\s+")
    assert re.search(r"BIS_API\s+" + ret + name + r"\s*\(", header), name


def test_without_a_device_they_return_no_device(lib):
    out = ctypes.c_void_p()
    fake = ctypes.c_void_p(0)
    assert lib.bis_spgemm(None, fake, fake, ctypes.byref(out)) == 1 and not out  # BIS_ERR_NO_DEVICE
    assert lib.bis_mat_transpose(None, fake, ctypes.byref(out)) == 1 and not out
    assert lib.bis_mg_create_smoothed(None, fake, None, ctypes.c_double(0.0), ctypes.byref(out)) == 1 and not out
    assert lib.bis_mg_create_smoothed(None, fake, None, ctypes.c_double(5.0), ctypes.byref(out)) == 1 and not out


def test_null_handles_and_limits(lib):
    lib.bis_spgemm_kernel.restype = ctypes.c_char_p
    lib.bis_mg_level_prolongator.restype = ctypes.c_void_p
    lib.bis_mg_level_restrictor.restype = ctypes.c_void_p
    assert lib.bis_spgemm_kernel(None) == b""
    assert lib.bis_mg_level_prolongator(None, ctypes.c_int(0)) is None and lib.bis_mg_level_restrictor(None, ctypes.c_int(0)) is None
    w = ctypes.c_double(-7.0)
    assert lib.bis_mg_level_prolong_omega(None, ctypes.c_int(0), ctypes.byref(w)) == 2 and w.value == -7.0  # BIS_ERR_INVALID
    wave, cap, cap_max, batch = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    assert lib.bis_spgemm_limits(ctypes.byref(wave), ctypes.byref(cap), ctypes.byref(cap_max), ctypes.byref(batch)) == 0
    assert (wave.value, cap.value, cap_max.value, batch.value) == (256, 4096, 4096, 1 << 26)
    assert lib.bis_spgemm_limits(None, None, None, None) == 0
    # the row path's LDS: 4 bytes per candidate column at the largest cap, far inside the CU's 160 KiB at full occupancy
    assert 8 * (4 * cap_max.value + 4 * 256) <= 160 * 1024
    for name in ("spgemm_row_cap", "spgemm_batch"):
        assert lib.bis_set_option(name.encode(), ctypes.c_int(-1)) == 0


def test_python_layer():
    import basic_iterative_solvers_amd as bis
    assert list(inspect.signature(bis.Context.spgemm).parameters) == ["self", "A", "B"]
    assert callable(bis.Mat.transpose) and callable(bis.Mat.spgemm_kernel)
    assert bis.spgemm_limits() == dict(wave_cap=256, row_cap=4096, row_cap_max=4096, batch=1 << 26)
    params = inspect.signature(bis.Context.mg).parameters
    assert params["smooth"].default is False and params["prolong_omega"].default == 0.0
    for name in ("prolongator", "restrictor", "prolong_omega"):
        assert callable(getattr(bis.MG, name))
    assert [f[0] for f in bis.MGParams._fields_] == ["max_levels", "coarse_limit", "coarsening", "nu", "coarse_sweeps", "omega",
                                                      "coarse_scale"]
    assert ctypes.sizeof(bis.MGParams) == 48
