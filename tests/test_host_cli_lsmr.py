"""GPU, through the host CLI: the method -lsmr [-damp L] [-colscale] (LSMR on the device schedule bis_lsmr_*,
methods/lsmr.hpp), the one method that takes a rectangular .mtx.  The table is the `r` column of the handle, the summary
adds the last `ar` entry; the CLI solves with b = 1 (as many entries as rows), x0 = 0.1 (as many as columns), tol 1e-14
for both tests."""
import os
import re
import subprocess

import numpy as np
import pytest

import lsmr_ref as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "basic_iterative_solvers_amd", "host", "basic_iterative_solvers")
RES = re.compile(r"\|\|A\*x_(\d+) - b\|\|_2 = (\S+)")
TOL = 1e-14
MAX_ITERS = 1000


def cli(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)


def solve(*args):
    out = cli(*args)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    table = RES.findall(out.stdout)
    m = re.search(r"Solver: (\S+).*?(converged in: |did not converge after )(\d+) iterations", out.stdout)
    ar = re.search(r"\|\|A\^T\(A\*x - b\)\|\|_2 estimate = (\S+)", out.stdout)
    assert m and ar, out.stdout[-1500:]
    return dict(hist=np.array([float(v) for _, v in table]), solver=m.group(1), converged=m.group(2).startswith("converged"),
                iters=int(m.group(3)), ar=float(ar.group(1)), stdout=out.stdout)


def write_mtx(path, A, symmetry="general"):
    rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
    with open(path, "w") as f:
        f.write(f"%%MatrixMarket matrix coordinate real {symmetry}\n{A.n_rows} {A.n_cols} {A.nnz}\n")
        f.writelines(f"{r + 1} {c + 1} {v:.17g}\n" for r, c, v in zip(rows, A.col, A.val))


@pytest.fixture(scope="module")
def T_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lsmr") / "T.mtx")
    write_mtx(path, L.table_matrix("T"))
    return path


def handle_solve(dA, damp=0.0, col_scaling=None):
    """The Python handle on the CLI's system."""
    ctx = dA.ctx
    db, dx = ctx.upload(np.ones(dA.n_rows)), ctx.upload(np.full(dA.n_cols, 0.1))
    s = ctx.lsmr(dA, db, dx, damp=damp, col_scaling=col_scaling)
    s.init(TOL)
    s.iterate(MAX_ITERS)
    out = s.status()
    out["x"] = dx.to_host()
    s.free()
    return out


@pytest.mark.parametrize("flags", [[], ["-damp", "0.5"], ["-colscale"]], ids=["plain", "damp", "colscale"])
def test_rectangular_file_against_the_python_handle(T_file, tmp_path, flags):
    from basic_iterative_solvers_amd import Context
    xfile = str(tmp_path / "x.txt")
    r = solve(T_file, "-lsmr", *flags, "-dump-x", xfile)
    ctx = Context()
    want = handle_solve(ctx.matrix(L.table_matrix("T")), damp=0.5 if "-damp" in flags else 0.0, col_scaling="norm" if "-colscale" in flags else None)
    ctx.close()
    r0 = want["hist_r"][0]
    k = min(21, len(want["hist_r"]), len(r["hist"]))
    dev = np.max(np.abs(r["hist"][:k] - want["hist_r"][:k])) / r0
    x = np.loadtxt(xfile)
    xerr = np.linalg.norm(x - want["x"]) / np.linalg.norm(want["x"])
    print(f"T {' '.join(flags)}: CLI {r['iters']} iterations, handle {want['iters']} (reason {want['reason']}); first {k} table entries "
          f"apart {dev:.2e} r0; x apart {xerr:.2e}; ar estimate {r['ar']:.3e} / {want['hist'][-1]:.3e}")
    assert r["solver"] == "lsmr" and "with preconditioner" not in r["stdout"]
    assert k == 21 and dev <= 1e-10
    assert x.shape == (700,) and xerr <= 1e-12
    assert r["iters"] == want["iters"] and r["converged"] == want["converged"] and len(r["hist"]) == want["iters"] + 1
    assert abs(r["ar"] - want["hist"][-1]) <= 1e-3 * want["hist"][-1]  # the summary prints four digits
    # an inconsistent system: the residual stays, the normal equations' residual is what converged
    assert r["converged"] and want["reason"] == 2 and r["hist"][-1] > 0.1 * r0 and r["ar"] < TOL * want["hist"][0]
    assert ("(damped)" in r["stdout"]) == ("-damp" in flags) and ("(in the scaled variable)" in r["stdout"]) == ("-colscale" in flags)
    if not flags:
        A = L.table_matrix("T")
        err = np.linalg.norm(x - L.lstsq_damped(A, np.ones(A.n_rows))) / np.linalg.norm(x)
        print(f"  x against lstsq: {err:.2e}")
        assert err <= 1e-10


def test_square_generator_input(tmp_path):
    from basic_iterative_solvers_amd import Context
    xfile = str(tmp_path / "x.txt")
    r = solve("unstr:8,8,8", "-lsmr", "-dump-x", xfile)
    ctx = Context()
    want = handle_solve(ctx.gen_unstr(8, 8, 8))
    ctx.close()
    r0 = want["hist_r"][0]
    k = min(21, len(want["hist_r"]), len(r["hist"]))
    dev = np.max(np.abs(r["hist"][:k] - want["hist_r"][:k])) / r0
    x = np.loadtxt(xfile)
    xerr = np.linalg.norm(x - want["x"]) / np.linalg.norm(want["x"])
    print(f"unstr:8,8,8: CLI {r['iters']} iterations, handle {want['iters']} (reason {want['reason']}, converged {want['converged']}); first {k} "
          f"table entries apart {dev:.2e} r0; x apart {xerr:.2e}; last table entry {r['hist'][-1] / r0:.2e} r0")
    # (a consistent, well-conditioned system: the solve may end before 20 entries exist; then every entry is compared)
    assert r["solver"] == "lsmr" and k == min(21, want["iters"] + 1) and dev <= 1e-10 and xerr <= 1e-12
    assert r["iters"] == want["iters"] and r["converged"] == want["converged"] and len(r["hist"]) == want["iters"] + 1
    assert np.all(np.diff(want["hist"]) <= 0)
    assert "res3 => iter_count:" in r["stdout"]  # the milestones, as for -mr


@pytest.mark.parametrize("flags,needle", [(["-p", "j"], "ERROR: -p does not apply to -lsmr"), (["-perm", "rcm"], "ERROR: -perm does not apply to -lsmr"),
                                          (["-unfused"], "ERROR: -unfused does not apply to -lsmr"),
                                          (["-hostscalars"], "ERROR: -hostscalars does not apply to -lsmr"),
                                          (["-scale", "1"], "ERROR: -scale 1 does not apply to -lsmr"),
                                          (["-damp", "-1"], "ERROR: -damp L"), (["-damp", "x"], "ERROR: -damp L")])
def test_flags_that_do_not_apply_are_refused(flags, needle):
    out = cli("hpcg:8", "-lsmr", *flags)
    assert out.returncode != 0 and needle in out.stderr


@pytest.mark.parametrize("method", ["-cg", "-mr", "-gm"])
@pytest.mark.parametrize("flags,needle", [(["-damp", "0.5"], "ERROR: -damp L is an option of LSMR: it needs the method -lsmr"),
                                          (["-colscale"], "ERROR: -colscale is an option of LSMR: it needs the method -lsmr")])
def test_lsmr_options_need_the_method(method, flags, needle):
    out = cli("hpcg:8", method, *flags)
    assert out.returncode != 0 and needle in out.stderr


@pytest.mark.parametrize("method", ["-cg", "-mr", "-idr", "-j"])
def test_other_methods_still_need_a_square_matrix(T_file, method):
    out = cli(T_file, method)
    assert out.returncode != 0 and "Matrix must be square." in out.stderr


def test_symmetric_banner_on_a_rectangular_matrix_is_an_error(tmp_path):
    path = str(tmp_path / "bad.mtx")
    write_mtx(path, L.banded(5, 3, 2, 4), symmetry="symmetric")
    out = cli(path, "-lsmr")
    assert out.returncode != 0 and "symmetric Matrix Market banner needs a square matrix" in out.stderr
    assert "Matrix must be square." in cli(path, "-cg").stderr


def test_usage_names_the_method():
    out = cli("hpcg:8", "-nosuchmethod")
    assert out.returncode != 0 and "-lsmr (LSMR" in out.stdout
