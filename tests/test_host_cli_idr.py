"""GPU, through the host CLI: the method -idr [-ids S] (IDR(s) on the device schedule bis_idr_*, methods/idr.hpp).  The table
is the recurrence of the true residual norm; the CLI solves with b = 1, x0 = 0.1, tol 1e-14."""
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import gen_from_cli_arg
from test_gpu_idr import Cache, host_spmv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "basic_iterative_solvers_amd", "host", "basic_iterative_solvers")
RES = re.compile(r"\|\|A\*x_(\d+) - b\|\|_2 = (\S+)")
MATRIX = "unstr:8,8,8"


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


@pytest.fixture(scope="module")
def bicgstab():
    return solve(MATRIX, "-bi")


@pytest.mark.parametrize("flags,pc,s", [([], "none", 4), (["-p", "ilu0", "-ids", "2"], "ilu0", 2)], ids=["idr4", "idr2-ilu0"])
def test_it_converges_and_x_solves_the_system(tmp_path, oracle, bicgstab, flags, pc, s):
    from basic_iterative_solvers_amd import Context
    xfile = str(tmp_path / "x.txt")
    r = solve(MATRIX, "-idr", *flags, "-dump-x", xfile)
    assert r["converged"] and r["solver"] == f"idr({s})"
    assert ("with preconditioner" in r["stdout"]) == (pc != "none")
    assert r["hist"][0] == bicgstab["hist"][0]  # || b - A x0 ||, the same kernels
    A = gen_from_cli_arg(oracle, MATRIX)
    n = A.n_rows
    x = np.loadtxt(xfile)
    assert x.shape == (n,)
    res = float(np.linalg.norm(np.ones(n) - oracle.spmv(A, x)))
    # the restatement of tests/idr_ref.py on the CLI's system: b = 1, x0 = 0.1, tol 1e-14
    ctx = Context()
    cache = Cache(ctx)
    e = cache.system("unstr8")
    assert e["n"] == n and np.array_equal(e["A"].col, A.col) and np.array_equal(e["A"].val, A.val)
    g = cache.ref("unstr8", pc, s, tag="cli", b=np.ones(n), x0=np.full(n, 0.1), tol=1e-14, iters=1000)
    res_g = float(np.linalg.norm(np.ones(n) - host_spmv(e["A"], g["x"])))
    ctx.close()
    r0 = r["hist"][0]
    print(f"{MATRIX} -idr {' '.join(flags)}: {r['iters']} iterations (restatement {g['iters']}, -bi {bicgstab['iters']}); || b - A x* || "
          f"recomputed by the oracle {res:.3e} = {res / r0:.3e} r0, the restatement's {res_g:.3e} = {res_g / r0:.3e} r0")
    assert g["conv"] and abs(r["iters"] - g["iters"]) <= 3
    assert res <= 10.0 * res_g


@pytest.mark.parametrize("args,message", [
    (["-idr", "-ids", "9"], "ERROR: -ids S: the dimension of the shadow space of -idr, 1 <= S <= 8"),
    (["-bi", "-ids", "2"], "ERROR: -ids S is the dimension of the shadow space of IDR(s): it needs the method -idr"),
    (["-idr", "-unfused"], "ERROR: -idr is a device schedule (bis_idr_*) and has no call-by-call form: -unfused and -hostscalars do not apply"),
    (["-idr", "-p", "mg", "-mg", "cycle=k"], "ERROR: -mg cycle=k|kgcr is not a fixed preconditioner, which -idr (IDR(s)) assumes: use -fgm, or cycle=v|w"),
], ids=["ids9", "ids-without-idr", "unfused", "k-cycle"])
def test_refusals(args, message):
    out = cli(MATRIX, *args)
    assert out.returncode != 0
    assert message in out.stderr


def test_bicgstab_prints_what_it_printed(bicgstab):
    assert bicgstab["solver"] == "bicgstab" and "idr" not in bicgstab["stdout"]
