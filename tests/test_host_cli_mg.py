"""GPU: the host CLI's `-p mg` -- one V-cycle of the aggregation multigrid hierarchy (bis_mg_create) as the preconditioner
of -cg, -gm and -bi: the hierarchy line after preprocessing, fewer CG iterations than without it, `-mg key=value,...`,
`-perm` (the permuted matrix has no grid hint: MIS aggregates), and the refusals."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "basic_iterative_solvers_amd", "host", "basic_iterative_solvers")
LINE = re.compile(r"^multigrid: (\d+) levels, rows ([\d /]+), operator complexity (\S+), aggregates ([a-z /]+)$", re.M)


def cli(*args):
    assert os.path.exists(BIN), "host binary not built (make -C basic_iterative_solvers_amd/host)"
    return subprocess.run([BIN] + list(args), capture_output=True, text=True, timeout=300)


def solve(*args):
    out = cli(*args)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"(converged in: |did not converge after )(\d+) iterations", out.stdout)
    assert m, out.stdout[-1500:]
    return dict(iters=int(m.group(2)), converged=m.group(1).startswith("converged"), stdout=out.stdout)


def hierarchy(stdout):
    m = LINE.findall(stdout)
    assert len(m) == 1, stdout[-1500:]
    levels, rows, complexity, kinds = m[0]
    rows = [int(r) for r in rows.split(" / ")]
    assert int(levels) == len(rows) and float(complexity) >= 1.0
    return rows, float(complexity), kinds.split(" / ")


def test_cg_with_mg_needs_fewer_iterations_and_prints_the_hierarchy():
    plain = solve("hpcg:16", "-cg")
    mg = solve("hpcg:16", "-cg", "-p", "mg")
    rows, complexity, kinds = hierarchy(mg["stdout"])
    print(f"hpcg:16 -cg: {plain['iters']} iterations, -p mg: {mg['iters']}; rows {rows}, operator complexity {complexity}, {kinds}")
    assert plain["converged"] and mg["converged"] and mg["iters"] < plain["iters"]
    assert rows == [4096, 512, 64] and kinds == ["grid", "grid"]
    assert not LINE.search(plain["stdout"])


@pytest.mark.parametrize("args,first_kind", [(("fem:8,8,8", "-bi", "-p", "mg"), "grid"), (("unstr:8,8,8", "-gm", "-p", "mg"), "mis"),
                                             (("hpcg:16", "-cg", "-p", "mg", "-perm", "rcm"), "mis"),
                                             (("hpcg:16", "-cg", "-p", "mg", "-mg", "nu=2,scale=1.5"), "grid"),
                                             (("hpcg:16", "-cg", "-p", "mg", "-unfused"), "grid"),
                                             (("hpcg:16", "-gm", "-p", "mg", "-hostscalars", "-mg", "coarsening=mis,limit=100,cs=2"), "mis")],
                         ids=["bicgstab-fem", "gmres-unstr", "cg-rcm", "cg-nu2-scale1.5", "cg-unfused", "gmres-hostscalars-mis"])
def test_converges(args, first_kind):
    run = solve(*args)
    rows, complexity, kinds = hierarchy(run["stdout"])
    print(f"{' '.join(args)}: {run['iters']} iterations; rows {rows}, operator complexity {complexity}, {kinds}")
    assert run["converged"] and len(rows) >= 2 and kinds[0] == first_kind


def test_refusals():
    out = cli("hpcg:8", "-cg", "-p", "mg", "-pprec", "32")
    assert out.returncode != 0 and "ERROR: -pprec 32 needs a preconditioner that is applied by SpMV" in out.stderr
    out = cli("hpcg:8", "-cg", "-p", "mg", "-mg", "nu=0")
    assert out.returncode != 0 and "bad parameters" in out.stderr and "converged" not in out.stdout
    out = cli("hpcg:8", "-cg", "-p", "mg", "-mg", "sweeps=3")
    assert out.returncode != 0 and "cannot read" in out.stderr
    out = cli("hpcg:8", "-gs", "-p", "mg")
    assert out.returncode != 0 and "-p mg needs a Krylov method" in out.stderr
