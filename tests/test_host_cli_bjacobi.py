"""GPU: the host CLI's `-p bj [-bs N]` -- block Jacobi (bis_bj_create) as the preconditioner of -cg, -gm, -fgm, -mr and -bi:
the block line after preprocessing, the block size from the grid hint's dof or from -bs, -perm, and the refusals."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "basic_iterative_solvers_amd", "host", "basic_iterative_solvers")
LINE = re.compile(r"^block Jacobi: (\d+) blocks of (\d+) rows \(last (\d+)\), (\d+) stored values(.*)$", re.M)


def cli(*args):
    assert os.path.exists(BIN), "host binary not built (make -C basic_iterative_solvers_amd/host)"
    return subprocess.run([BIN] + list(args), capture_output=True, text=True, timeout=300)


def solve(*args):
    out = cli(*args)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"(converged in: |did not converge after )(\d+) iterations", out.stdout)
    assert m, out.stdout[-1500:]
    return dict(iters=int(m.group(2)), converged=m.group(1).startswith("converged"), stdout=out.stdout)


def block_line(stdout):
    m = LINE.findall(stdout)
    assert len(m) == 1, stdout[-1500:]
    blocks, rows, last, values, rest = m[0]
    return int(blocks), int(rows), int(last), int(values), rest


def test_cg_on_fem_takes_the_block_size_from_the_grid_hint():
    plain = solve("fem:8,8,8", "-cg", "-p", "j")
    run = solve("fem:8,8,8", "-cg", "-p", "bj")
    blocks, rows, last, values, rest = block_line(run["stdout"])
    print(f"fem:8,8,8 -cg: -p j {plain['iters']} iterations, -p bj {run['iters']}; {blocks} blocks of {rows} rows (last {last}), {values} values")
    assert run["converged"] and (blocks, rows, last, values, rest) == (512, 3, 3, 4608, "")
    assert "with preconditioner: block jacobi" in run["stdout"]
    assert not LINE.search(plain["stdout"])


def test_without_a_dof_the_block_size_must_be_given():
    out = cli("hpcg:16", "-cg", "-p", "bj")
    assert out.returncode != 0 and "-bs" in out.stderr and "converged" not in out.stdout
    run = solve("hpcg:16", "-cg", "-p", "bj", "-bs", "16")
    assert run["converged"] and block_line(run["stdout"]) == (256, 16, 16, 65536, "")
    run = solve("hpcg:16", "-cg", "-p", "bj", "-bs", "7")  # 4096 = 7 * 585 + 1
    assert run["converged"] and block_line(run["stdout"]) == (586, 7, 1, 585 * 49 + 1, "")


@pytest.mark.parametrize("method", ["-bi", "-gm", "-fgm", "-mr", "-cg"])
def test_krylov_methods_on_unstr(method):
    run = solve("unstr:8,8,8", method, "-p", "bj", "-bs", "3")
    blocks, rows, last, values, rest = block_line(run["stdout"])
    print(f"unstr:8,8,8 {method} -p bj -bs 3: {run['iters']} iterations")
    assert run["converged"] and (blocks, rows, last, values, rest) == (512, 3, 3, 4608, "")


@pytest.mark.parametrize("args", [("fem:8,8,8", "-cg", "-p", "bj", "-unfused"), ("fem:8,8,8", "-gm", "-p", "bj", "-hostscalars"),
                                  ("fem:8,8,8", "-bi", "-p", "bj", "-hostscalars")], ids=["cg-unfused", "gmres-hostscalars", "bicgstab-hostscalars"])
def test_call_by_call_forms(args):
    run = solve(*args)
    assert run["converged"] and block_line(run["stdout"])[:2] == (512, 3)


def test_perm_blocks_are_consecutive_rows_of_the_permuted_matrix():
    run = solve("fem:8,8,8", "-cg", "-p", "bj", "-bs", "3", "-perm", "rcm")
    blocks, rows, last, values, rest = block_line(run["stdout"])
    assert run["converged"] and (blocks, rows, last, values) == (512, 3, 3, 4608) and "permuted" in rest


def test_refusals():
    for method in ("-j", "-gs", "-sgs"):
        out = cli("fem:8,8,8", method, "-p", "bj")
        assert out.returncode != 0 and "-p bj needs a Krylov method" in out.stderr, method
    out = cli("fem:8,8,8", "-cg", "-p", "bj", "-pprec", "32")
    assert out.returncode != 0 and "ERROR: -pprec 32 needs a preconditioner that is applied by SpMV" in out.stderr
    for bs in ("0", "33", "-4", "x"):
        out = cli("fem:8,8,8", "-cg", "-p", "bj", "-bs", bs)
        assert out.returncode != 0 and "-bs N" in out.stderr and "converged" not in out.stdout, bs
