"""GPU, through the host CLI: the method -mr (MINRES on the device schedule bis_minres_*, methods/minres.hpp).  The table is
phibar, the residual norm (in the M^-1 norm with a preconditioner); the CLI solves with b = 1, x0 = 0.1, tol 1e-14."""
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import gen_from_cli_arg, hist_dev
from test_gpu_minres import Cache, run_ref

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
    m = re.search(r"Solver: (\S+).*?(converged in: |did not converge after )(\d+) iterations", out.stdout)
    assert m, out.stdout[-1500:]
    return dict(hist=np.array([float(v) for _, v in table]), solver=m.group(1), converged=m.group(2).startswith("converged"),
                iters=int(m.group(3)), stdout=out.stdout)


def test_on_an_spd_matrix_it_does_what_cg_does():
    m, c = solve("anderson:12,shift=7", "-mr"), solve("anderson:12,shift=7", "-cg")
    print(f"anderson:12,shift=7: -mr {m['iters']} iterations, -cg {c['iters']}; largest rise of the -mr table "
          f"{np.max(np.diff(m['hist'])) / m['hist'][0]:.3e} r0")
    assert m["solver"] == "minres" and m["converged"] and c["converged"]
    assert abs(m["iters"] - c["iters"]) <= 2
    assert m["hist"][0] == c["hist"][0]
    assert np.all(np.diff(m["hist"]) <= 0.0)
    assert "res3 => iter_count:" in m["stdout"] and "res6 => iter_count:" in m["stdout"]  # the milestones, as for -cg


def test_an_indefinite_matrix(tmp_path, oracle):
    from basic_iterative_solvers_amd import Context
    xfile = str(tmp_path / "x.txt")
    r = solve("anderson:10,shift=6.5", "-mr", "-dump-x", xfile)
    r0 = r["hist"][0]
    assert r["converged"] and np.all(np.diff(r["hist"]) <= 0.0)
    # the reference loop of tests/test_gpu_minres.py with the CLI's system: b = 1, x0 = 0.1, tol 1e-14
    ctx = Context()
    e = Cache(ctx).system("and10")
    ref = run_ref(ctx, e, (None, None, None, 0), iters=1000, b=np.ones(e["n"]), x0=np.full(e["n"], 0.1), tol=1e-14)
    ctx.close()
    dev = hist_dev(r["hist"][:41], ref["hist"][:41])
    print(f"anderson:10,shift=6.5 -mr: {r['iters']} iterations, reference loop {ref['iters']}, first 40 entries apart {dev:.3e} r0")
    assert ref["conv"] and abs(r["iters"] - ref["iters"]) <= 2
    assert dev <= 1e-10
    A = gen_from_cli_arg(oracle, "anderson:10,shift=6.5")
    x = np.loadtxt(xfile)
    assert x.shape == (A.n_rows,)
    res = float(np.linalg.norm(np.ones(A.n_rows) - oracle.spmv(A, x)))
    print(f"|| b - A x* || recomputed by the oracle {res:.6e} = {res / r0:.3e} r0, last table entry {r['hist'][-1] / r0:.3e} r0")
    assert abs(res - r["hist"][-1]) <= 1e-10 * r0


@pytest.mark.parametrize("matrix,flags", [("anderson:10,shift=6.5", ["-p", "j"]), ("hpcg:16", ["-p", "mg"]),
                                          ("hpcg:16", ["-p", "sgs", "-perm", "rcm"])], ids=["anderson-j", "hpcg-mg", "hpcg-sgs-rcm"])
def test_preconditioned_runs_converge(matrix, flags):
    r = solve(matrix, "-mr", *flags)
    print(f"{matrix} -mr {' '.join(flags)}: {r['iters']} iterations")
    assert r["converged"] and r["solver"] == "minres" and "with preconditioner" in r["stdout"]
    assert np.all(np.diff(r["hist"]) <= 0.0)


def test_the_k_cycle_is_refused():
    out = cli("hpcg:16", "-mr", "-p", "mg", "-mg", "cycle=k")
    assert out.returncode != 0
    assert "ERROR: -mg cycle=k|kgcr is not a fixed preconditioner, which -mr (MINRES) assumes: use -fgm, or cycle=v|w" in out.stderr


@pytest.mark.parametrize("flag", ["-unfused", "-hostscalars"])
def test_there_is_no_call_by_call_form(flag):
    out = cli("hpcg:8", "-mr", flag)
    assert out.returncode != 0
    assert "no call-by-call form" in out.stderr and "ERROR: -mr" in out.stderr


def test_cg_prints_what_it_printed(oracle):
    r = solve("hpcg:16", "-cg")
    ref = oracle.solve(oracle.gen_hpcg(16), "cg", "none")
    assert r["solver"] == "conjugate-gradient" and "minres" not in r["stdout"]
    assert hist_dev(r["hist"], ref["hist"]) <= 1e-10 and r["converged"] and abs(r["iters"] - ref["iters"]) <= 1
