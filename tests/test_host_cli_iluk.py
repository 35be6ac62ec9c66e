"""GPU: the host CLI's `-fill K` -- ILU(K) with level-of-fill (bis_mat_iluk) behind -p ilu0 and -p ilu0it: a command line
without the flag prints what it printed, K >= 1 adds the fill line and lowers the iteration count, -perm and -pprec 32
compose, and the flag is refused with any other preconditioner."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "basic_iterative_solvers_amd", "host", "basic_iterative_solvers")
LINE = re.compile(r"^ILU\((\d+)\): (\d+) fill entries, L\+U\+D entries = (\d+) \(([0-9.e+-]+) x A\)$", re.M)


def cli(*args):
    assert os.path.exists(BIN), "host binary not built (make -C basic_iterative_solvers_amd/host)"
    return subprocess.run([BIN] + list(args), capture_output=True, text=True, timeout=300)


def solve(*args):
    out = cli(*args)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"(converged in: |did not converge after )(\d+) iterations", out.stdout)
    assert m, out.stdout[-1500:]
    return dict(iters=int(m.group(2)), converged=m.group(1).startswith("converged"), stdout=out.stdout)


def untimed(stdout):
    """The output without the lines that carry wall-clock times."""
    return [l for l in stdout.splitlines() if "[s]" not in l and "time" not in l.lower()]


def test_without_the_flag_nothing_changes_and_level_one_needs_fewer_iterations():
    plain = solve("hpcg:12", "-cg", "-p", "ilu0")
    zero = solve("hpcg:12", "-cg", "-p", "ilu0", "-fill", "0")
    one = solve("hpcg:12", "-cg", "-p", "ilu0", "-fill", "1")
    assert not LINE.search(plain["stdout"]) and "incomplete LU(0)" in plain["stdout"] and "ILU(" not in plain["stdout"]
    assert untimed(zero["stdout"]) == untimed(plain["stdout"])
    level, fill, entries, ratio = LINE.findall(one["stdout"])[0]
    n, nnz = 12 ** 3, (3 * 12 - 2) ** 3
    print(f"hpcg:12 -cg -p ilu0: {plain['iters']} iterations, -fill 1: {one['iters']}; {fill} fill entries, {entries} stored ({ratio} x A)")
    assert int(level) == 1 and int(fill) > 0 and int(entries) == nnz + int(fill) and abs(float(ratio) - int(entries) / nnz) < 1e-3
    assert n < int(fill)
    assert "incomplete LU(1)" in one["stdout"] and "incomplete LU(0)" not in one["stdout"]
    assert plain["converged"] and one["converged"] and one["iters"] < plain["iters"]


def test_perm_and_rounded_iterative_solves_compose():
    run = solve("hpcg:12", "-cg", "-p", "ilu0it", "-fill", "2", "-inner", "6", "-pprec", "32", "-perm", "rcm")
    assert run["converged"] and LINE.findall(run["stdout"])[0][0] == "2"
    assert "incomplete LU(2), iterative solves (6)" in run["stdout"]
    assert "preconditioner values rounded to fp32" in run["stdout"] and "reverse Cuthill-McKee" in run["stdout"]
    # rounding follows the factorisation
    assert run["stdout"].index("ILU(2):") < run["stdout"].index("preconditioner values rounded")


def test_refusals():
    out = cli("hpcg:12", "-cg", "-p", "sgs", "-fill", "1")
    assert out.returncode != 0 and "-fill K" in out.stderr and "converged" not in out.stdout
    out = cli("hpcg:12", "-cg", "-fill", "1")
    assert out.returncode != 0 and "-fill K" in out.stderr
    for k in ("17", "-1", "x"):
        out = cli("hpcg:12", "-cg", "-p", "ilu0", "-fill", k)
        assert out.returncode != 0 and "-fill K" in out.stderr and "converged" not in out.stdout, k
