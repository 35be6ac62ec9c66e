"""GPU: the host CLI's `-pprec 32|64` -- the factors that -p fsai and -p ilu0it apply by SpMV are rounded to fp32 after the
factorisation (bis_mat_round_f32); the solve converges in the same number of iterations (+-1) as without the flag, the
rounding is reported in one line, and the flag is an error with a preconditioner that runs exact sweeps."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "basic_iterative_solvers_amd", "host", "basic_iterative_solvers")
LINE = re.compile(r"^preconditioner values rounded to fp32: max relative change (\S+)$", re.M)


def cli(*args):
    assert os.path.exists(BIN), "host binary not built (make -C basic_iterative_solvers_amd/host)"
    return subprocess.run([BIN] + list(args), capture_output=True, text=True, timeout=300)


def solve(*args):
    out = cli(*args)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"(converged in: |did not converge after )(\d+) iterations", out.stdout)
    assert m, out.stdout[-1500:]
    return dict(iters=int(m.group(2)), converged=m.group(1).startswith("converged"), stdout=out.stdout)


@pytest.mark.parametrize("args", [("fem:8,8,8", "-cg", "-p", "fsai"), ("fem:8,8,8", "-bi", "-p", "ilu0it", "-inner", "3")],
                         ids=["cg-fsai", "bicgstab-ilu0it"])
def test_pprec_32_converges_like_64(args):
    plain = solve(*args)
    r64 = solve(*args, "-pprec", "64")
    r32 = solve(*args, "-pprec", "32")
    print(f"{' '.join(args)}: {plain['iters']} iterations, -pprec 32: {r32['iters']}")
    assert plain["converged"] and r32["converged"]
    assert not LINE.search(plain["stdout"]) and not LINE.search(r64["stdout"])  # without the flag: what it printed before
    assert r64["iters"] == plain["iters"]
    m = LINE.findall(r32["stdout"])
    assert len(m) == 1 and 0.0 < float(m[0]) <= 2.0 ** -24, m
    assert abs(r32["iters"] - plain["iters"]) <= 1


@pytest.mark.parametrize("extra", [("-p", "ilu0"), ("-p", "sgs"), ()], ids=["ilu0", "sgs", "none"])
def test_pprec_32_needs_a_preconditioner_applied_by_spmv(extra):
    out = cli("hpcg:8", "-cg", *extra, "-pprec", "32")
    assert out.returncode != 0
    assert "ERROR: -pprec 32 needs a preconditioner that is applied by SpMV" in out.stderr
    assert "converged" not in out.stdout


def test_pprec_takes_32_or_64():
    out = cli("hpcg:8", "-cg", "-p", "fsai", "-pprec", "16")
    assert out.returncode != 0 and "ERROR: -pprec 32|64" in out.stderr
