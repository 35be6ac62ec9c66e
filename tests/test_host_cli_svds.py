"""GPU, through the host CLI: the method -svd K [-which lm|sm] [-ncv M] (thick-restart Lanczos bidiagonalisation on the device
schedule bis_svds_*, methods/svds.hpp) on a rectangular .mtx the test writes.  The table is the restart history, the summary
names the solver and adds the number of products, one line per triplet and max ||A v - sigma u||_2 + ||A^T u - sigma v||_2
computed from the returned vectors; the CLI solves with tol 1e-10."""
import os
import re
import subprocess

import numpy as np
import pytest

import svds_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "basic_iterative_solvers_amd", "host", "basic_iterative_solvers")
RES = re.compile(r"\|\|A\*x_(\d+) - b\|\|_2 = (\S+)")
TRIPLET = re.compile(r"sigma_(\d+) = (\S+) residual estimate = (\S+)")
TOL = 1e-10


def cli(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)


def write_mtx(path, A):
    rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
    with open(path, "w") as f:
        f.write(f"%%MatrixMarket matrix coordinate real general\n{A.n_rows} {A.n_cols} {A.nnz}\n")
        f.writelines(f"{r + 1} {c + 1} {v:.17g}\n" for r, c, v in zip(rows, A.col, A.val))


@pytest.fixture(scope="module")
def T_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("svds") / "T.mtx")
    write_mtx(path, S.table_matrix("T"))  # 1301 x 700
    return path


@pytest.mark.parametrize("flags,which,ncv", [([], "LM", None), (["-which", "sm", "-ncv", "24"], "SM", 24)], ids=["default", "sm24"])
def test_values_are_the_python_handle_s(T_file, flags, which, ncv):
    from basic_iterative_solvers_amd import Context
    out = cli(T_file, "-svd", "4", *flags)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    ctx = Context()
    dA = ctx.matrix(S.table_matrix("T"))
    s = ctx.svds(dA, k=4, which=which, ncv=ncv, tol=TOL)
    want = s.solve(max_cycles=400)
    s.free()
    ctx.close()
    triplets = TRIPLET.findall(out.stdout)
    table = np.array([float(v) for _, v in RES.findall(out.stdout)])
    m = re.search(r"Solver: lanczos-svd\((\d+), ncv=(\d+), (\w+)\) converged in: (\d+) iterations", out.stdout)
    prod = re.search(r"Operator products: (\d+), restarts: (\d+)", out.stdout)
    res = re.search(r"max \|\|A v - sigma u\|\|_2 \+ \|\|A\^T u - sigma v\|\|_2 = (\S+)", out.stdout)
    assert m and prod and res and len(triplets) == 4, out.stdout[-2000:]
    print(f"T -svd 4 {' '.join(flags)}: {m.group(0)}; products {prod.group(1)}; values {[t[1] for t in triplets]}; "
          f"handle {want['values']}; residual line {res.group(1)}")
    assert (int(m.group(1)), int(m.group(2)), m.group(3)) == (4, 20 if ncv is None else ncv, which.lower())
    assert int(m.group(4)) == want["restarts"] and int(prod.group(1)) == want["products"] and int(prod.group(2)) == want["restarts"]
    # to the digits printed: the same handle on the same matrix gives the same bits
    for (i, val, est), wv, we in zip(triplets, want["values"], want["est"]):
        assert val == f"{wv:.16e}" and est == f"{we:.16e}", (i, val, wv)
    assert len(table) >= want["restarts"] and np.array_equal(table[:want["restarts"]], want["hist"])
    # the true residuals of converged triplets: estimate-sized, at most 4 tol sigma_max
    assert 0.0 < float(res.group(1)) <= 4 * TOL * want["sigma_ref"]
    assert want["converged"]


@pytest.mark.parametrize("flags,needle", [(["-p", "j"], "ERROR: -p does not apply to -svd K"), (["-perm", "rcm"], "ERROR: -perm does not apply to -svd K"),
                                          (["-scale", "1"], "ERROR: -scale does not apply to -svd K"),
                                          (["-unfused"], "ERROR: -unfused does not apply to -svd K"),
                                          (["-hostscalars"], "ERROR: -hostscalars does not apply to -svd K"),
                                          (["-ncv", "4"], "ERROR: -ncv M: the basis size of -svd K must exceed K"),
                                          (["-ncv", "65"], "ERROR: -ncv M: the basis size of -svd K"),
                                          (["-which", "sa"], "ERROR: -which lm|sm"), (["-which", "la"], "ERROR: -which lm|sm")])
def test_flags_that_do_not_apply_are_refused(T_file, flags, needle):
    out = cli(T_file, "-svd", "4", *flags)
    assert out.returncode != 0 and needle in out.stderr


def test_svd_needs_its_count(T_file):
    for args in (["-svd"], ["-svd", "x"], ["-svd", "0"], ["-svd", "64"]):
        out = cli(T_file, *args)
        assert out.returncode != 0 and "ERROR: -svd K" in out.stderr


def test_other_methods_still_need_a_square_matrix(T_file):
    out = cli(T_file, "-cg")
    assert out.returncode != 0 and "Matrix must be square." in out.stderr
    out = cli(T_file, "-eig", "2")
    assert out.returncode != 0 and "Matrix must be square." in out.stderr


def test_usage_names_the_method():
    out = cli("hpcg:8", "-nosuchmethod")
    assert out.returncode != 0 and "-svd K (thick-restart Lanczos bidiagonalisation" in out.stdout
