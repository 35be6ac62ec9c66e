"""CPU: the library exports bis_mat_round_f32 and the header declares it, it refuses a null context like every other entry
point -- no CPU path -- and leaves its out-parameter alone, the option spmv_win4 is in the options table, the Python layer
carries Mat.round_f32, and the host CLI rejects a bad -pprec before it touches a device."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "basic_iterative_solvers_amd", "host", "basic_iterative_solvers")


@pytest.fixture(scope="module")
def lib():
    from basic_iterative_solvers_amd import build
    return ctypes.CDLL(build.build())


def test_symbol_is_exported_and_declared(lib):
    assert hasattr(lib, "bis_mat_round_f32")
    with open(os.path.join(ROOT, "include", "bis_hip.h")) as f:
        header = f.read()
    assert re.search(r"BIS_API\s+bis_status\s+bis_mat_round_f32\s*\(\s*bis_ctx \*ctx,\s*bis_mat \*A,\s*double \*max_rel_change\s*\)", header)


def test_null_context_is_refused(lib):
    m = ctypes.c_double(-7.0)
    assert lib.bis_mat_round_f32(None, None, ctypes.byref(m)) == 1  # BIS_ERR_NO_DEVICE
    assert m.value == -7.0


def test_option_is_in_the_table(lib):
    assert lib.bis_set_option(b"spmv_win4", 0) == 0
    buf = ctypes.create_string_buffer(4096)
    lib.bis_options_describe(buf, 4096)
    assert b'"spmv_win4": 0' in buf.value or b'"spmv_win4":0' in buf.value, buf.value
    assert lib.bis_set_option(b"spmv_win4", -1) == 0
    lib.bis_options_describe(buf, 4096)
    assert b"spmv_win4" not in buf.value


def test_python_layer_has_round_f32():
    import basic_iterative_solvers_amd as bis
    assert callable(bis.Mat.round_f32)


@pytest.mark.parametrize("args,text", [
    (("hpcg:8", "-cg", "-p", "ilu0", "-pprec", "32"), "ERROR: -pprec 32 needs a preconditioner that is applied by SpMV"),
    (("hpcg:8", "-cg", "-pprec", "32"), "ERROR: -pprec 32 needs a preconditioner that is applied by SpMV"),
    (("hpcg:8", "-cg", "-p", "fsai", "-pprec", "16"), "ERROR: -pprec 32|64")])
def test_cli_rejects_a_bad_pprec_before_any_device_work(args, text):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(BIN)])
    out = subprocess.run([BIN] + list(args), capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and text in out.stderr, out.stdout[-500:] + out.stderr[-500:]
