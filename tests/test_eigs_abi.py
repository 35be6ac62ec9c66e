"""CPU: the library exports the eigensolver entry points (bis_eigs_*), they refuse a null context like every other entry
point -- no CPU path -- and leave their out-parameters alone, and the Python layer carries the class."""
import ctypes

import pytest

SYMBOLS = ["bis_eigs_create", "bis_eigs_set_start", "bis_eigs_init", "bis_eigs_iterate", "bis_eigs_op_begin", "bis_eigs_op_end",
           "bis_eigs_status", "bis_eigs_vectors", "bis_eigs_destroy"]


@pytest.fixture(scope="module")
def lib():
    from basic_iterative_solvers_amd import build
    return ctypes.CDLL(build.build())


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_exported(lib, name):
    assert hasattr(lib, name)


def test_null_context_is_refused(lib):
    h = ctypes.c_void_p()
    assert lib.bis_eigs_create(None, None, ctypes.c_int64(8), ctypes.c_int(2), ctypes.c_int(0), ctypes.c_int(0),
                               ctypes.byref(h)) == 1 and not h  # BIS_ERR_NO_DEVICE
    assert lib.bis_eigs_set_start(None, None, None) == 1
    assert lib.bis_eigs_init(None, None, ctypes.c_double(1e-10)) == 1
    assert lib.bis_eigs_iterate(None, None, ctypes.c_int(1)) == 1
    inp, out = ctypes.c_void_p(7), ctypes.c_void_p(7)
    assert lib.bis_eigs_op_begin(None, None, ctypes.byref(inp), ctypes.byref(out)) == 1
    assert (inp.value, out.value) == (7, 7)
    assert lib.bis_eigs_op_end(None, None) == 1
    ints = [ctypes.c_int(-7) for _ in range(6)]
    arrays = [(ctypes.c_double * 4)(*([-7.0] * 4)) for _ in range(4)]
    assert lib.bis_eigs_status(None, None, *[ctypes.byref(i) for i in ints], *arrays, ctypes.c_int(4)) == 1
    assert [i.value for i in ints] == [-7] * 6 and all(list(a) == [-7.0] * 4 for a in arrays)
    assert lib.bis_eigs_vectors(None, None, None, ctypes.c_int64(8)) == 1
    assert lib.bis_eigs_destroy(None, None) == 1
    assert not h


def test_python_layer_has_eigs():
    import basic_iterative_solvers_amd as bis
    assert callable(bis.Context.eigs)
    assert bis.Eigs._sym == "eigs" and issubclass(bis.Eigs, bis._Solver)
    for name in ("init", "iterate", "status", "vectors", "op_begin", "op_end", "solve", "set_start", "free"):
        assert callable(getattr(bis.Eigs, name))
    assert bis.Eigs.WHICH == {"SA": 0, "LA": 1, "LM": 2}
