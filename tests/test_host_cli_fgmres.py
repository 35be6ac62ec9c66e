"""GPU, through the host CLI: the method -fgm (flexible GMRES on the device schedule bis_fgmres_*, methods/fgmres.hpp).
Without a preconditioner it prints -gm's table, name apart; with one it stands on the right, so the table is the true
residual's, and it takes the K-cycles of -p mg that -gm still refuses.  The iteration counts of the preconditioned runs are
printed, not asserted."""
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import gen_from_cli_arg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "basic_iterative_solvers_amd", "host", "basic_iterative_solvers")
RES = re.compile(r"\|\|A\*x_(\d+) - b\|\|_2 = (\S+)")


def cli(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)


def solve(*args):
    out = cli(*args)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    table = RES.findall(out.stdout)
    m = re.search(r"Solver: (\S+)\((\d+)\).*?(converged in: |did not converge after )(\d+) iterations", out.stdout)
    assert m, out.stdout[-1500:]
    stop = float(re.search(r"tol \* \|\|Ax_0 - b\|\|_2\" is: (\S+)", out.stdout).group(1))
    final = float(re.search(r"\|\|A\*x_star - b\|\|_2 = ([^\s]+?)\.\n", out.stdout).group(1))
    return dict(labels=[int(k) for k, _ in table], hist=np.array([float(v) for _, v in table]), solver=m.group(1), rl=int(m.group(2)),
                converged=m.group(3).startswith("converged"), iters=int(m.group(4)), stop=stop, final=final, stdout=out.stdout)


def test_without_a_preconditioner_the_table_is_gmres_s():
    f, g = solve("hpcg:16", "-fgm"), solve("hpcg:16", "-gm")
    r0 = g["hist"][0]
    n = min(len(f["hist"]), len(g["hist"]))
    dev = np.max(np.abs(f["hist"][:n] - g["hist"][:n])) / r0
    print(f"hpcg:16: -fgm {f['iters']} iterations, {len(f['hist'])} table lines, -gm {g['iters']} iterations, {len(g['hist'])} lines, "
          f"tables apart {dev:.3e} r0")
    assert (f["solver"], g["solver"]) == ("fgmres", "gmres") and f["rl"] == g["rl"] == 10
    assert dev <= 1e-10
    assert f["iters"] == g["iters"] and len(f["hist"]) == len(g["hist"]) and f["labels"] == g["labels"]
    assert f["converged"] and g["converged"]
    assert f["stop"] == g["stop"]


def test_restart_length_flag():
    f, g = solve("hpcg:8", "-fgm", "-rl", "4"), solve("hpcg:8", "-gm", "-rl", "4")
    assert f["rl"] == 4 and "Solver: fgmres(4)" in f["stdout"]
    n = min(len(f["hist"]), len(g["hist"]))
    assert np.max(np.abs(f["hist"][:n] - g["hist"][:n])) <= 1e-10 * g["hist"][0]
    # the summary's count includes the restarts, as for -gm: one table line per iteration and per restart
    assert f["iters"] == len(f["hist"]) - 1


CONVERGED = [("hpcg:32", ["-p", "mg", "-mg", "limit=64,cycle=k"]),
             ("unstr:8,8,8", ["-p", "mg", "-mg", "cycle=kgcr,limit=8"]),
             ("anderson:14,shift=9", ["-p", "gs", "-rl", "5"])]


@pytest.mark.parametrize("matrix,flags", CONVERGED, ids=[c[0] for c in CONVERGED])
def test_preconditioned_runs_converge(tmp_path, oracle, matrix, flags):
    xfile = str(tmp_path / "x.txt")
    r = solve(matrix, "-fgm", *flags, "-dump-x", xfile)
    r0 = r["hist"][0]
    print(f"{matrix} -fgm {' '.join(flags)}: {r['iters']} iterations (restarts included), {len(r['hist'])} table lines, final "
          f"{r['final']:.6e}, stopping criterion {r['stop']:.6e}, r0 {r0:.6e}")
    assert r["converged"] and r["solver"] == "fgmres"
    assert r["final"] <= r["stop"] + 1e-10 * r0
    assert r["final"] == r["hist"][-1]
    A = gen_from_cli_arg(oracle, matrix)
    x = np.loadtxt(xfile)
    assert x.shape == (A.n_rows,)
    res = float(np.linalg.norm(np.ones(A.n_rows) - oracle.spmv(A, x)))  # b = 1 (B_VAL)
    print(f"{matrix}: || b - A x* || recomputed by the oracle {res:.6e}, apart {abs(res - r['final']) / r0:.3e} r0")
    assert abs(res - r["final"]) <= 1e-10 * r0
    assert res <= r["stop"] + 1e-10 * r0


def test_gmres_still_refuses_the_k_cycle():
    out = cli("hpcg:32", "-gm", "-p", "mg", "-mg", "limit=64,cycle=k")
    assert out.returncode != 0
    assert ("ERROR: -mg cycle=k|kgcr is not a fixed preconditioner, which -gm (left-preconditioned GMRES, not flexible) assumes: "
            "use -cg or -bi, or cycle=v|w") in out.stderr


@pytest.mark.parametrize("flag", ["-unfused", "-hostscalars"])
def test_there_is_no_call_by_call_form(flag):
    out = cli("hpcg:8", "-fgm", flag)
    assert out.returncode != 0
    assert "no call-by-call form" in out.stderr and "ERROR: -fgm" in out.stderr


def test_a_stationary_method_still_cannot_take_mg():
    out = cli("hpcg:8", "-j", "-p", "mg")
    assert out.returncode != 0
    assert "ERROR: -p mg needs a Krylov method: -cg, -gm or -bi" in out.stderr
