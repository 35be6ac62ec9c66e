"""CPU: the library exports the multigrid cycle entry points (bis_mg_set_cycle, bis_mg_cycle), the header declares them and
the four cycle values, they refuse a null context / a null hierarchy and leave their out-parameters alone, the Python layer
carries MG.set_cycle, MG.cycle and the Context.mg keywords, and bis_mg_params is still the seven pinned fields."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["bis_mg_set_cycle", "bis_mg_cycle"]


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
    assert re.search(r"BIS_API\s+bis_status\s+" + name + r"\s*\(", header), name


@pytest.mark.parametrize("name,value", [("BIS_MG_CYCLE_V", 0), ("BIS_MG_CYCLE_W", 1), ("BIS_MG_CYCLE_K", 2), ("BIS_MG_CYCLE_K_GCR", 3)])
def test_cycle_values_are_declared(header, name, value):
    assert re.search(r"\b" + name + r"\s*=\s*" + str(value) + r"\b", header), name


def test_null_arguments_are_refused(lib):
    assert lib.bis_mg_set_cycle(None, None, ctypes.c_int(2), ctypes.c_int(0)) == 1  # BIS_ERR_NO_DEVICE
    cycle, levels = ctypes.c_int(-7), ctypes.c_int(-7)
    assert lib.bis_mg_cycle(None, ctypes.byref(cycle), ctypes.byref(levels)) == 2  # BIS_ERR_INVALID
    assert cycle.value == -7 and levels.value == -7
    assert lib.bis_mg_cycle(None, None, None) == 2


def test_python_layer_has_the_cycle():
    import basic_iterative_solvers_amd as bis
    assert callable(bis.MG.set_cycle)
    assert list(inspect.signature(bis.MG.set_cycle).parameters) == ["self", "cycle", "levels"]
    assert inspect.signature(bis.MG.set_cycle).parameters["levels"].default == 0
    assert isinstance(inspect.getattr_static(bis.MG, "cycle"), property)
    assert bis.MG.CYCLE == dict(v=0, w=1, k=2, kgcr=3)
    params = inspect.signature(bis.Context.mg).parameters
    assert "cycle" in params and "cycle_levels" in params and params["cycle_levels"].default == 0
    assert [f[0] for f in bis.MGParams._fields_] == ["max_levels", "coarse_limit", "coarsening", "nu", "coarse_sweeps", "omega",
                                                      "coarse_scale"]
    assert ctypes.sizeof(bis.MGParams) == 48
