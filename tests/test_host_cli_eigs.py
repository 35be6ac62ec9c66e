"""GPU, through the host CLI: the method -eig K [-which sa|la|lm] [-ncv M] (thick-restart Lanczos on the device schedule
bis_eigs_*, methods/eigs.hpp).  The table is the restart history, the summary names the solver and adds the number of
products, one line per pair and max ||A x - lambda x||_2 computed from the returned vectors; the CLI solves with tol 1e-10."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "basic_iterative_solvers_amd", "host", "basic_iterative_solvers")
RES = re.compile(r"\|\|A\*x_(\d+) - b\|\|_2 = (\S+)")
PAIR = re.compile(r"lambda_(\d+) = (\S+) residual estimate = (\S+)")
TOL = 1e-10


def cli(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("flags,which,ncv", [([], "SA", None), (["-which", "la", "-ncv", "24"], "LA", 24)], ids=["default", "la24"])
def test_values_are_the_python_handle_s(flags, which, ncv):
    from basic_iterative_solvers_amd import Context
    out = cli("anderson:8", "-eig", "4", *flags)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    ctx = Context()
    dA = ctx.gen_anderson(8)
    s = ctx.eigs(dA, k=4, which=which, ncv=ncv, tol=TOL)
    want = s.solve(max_cycles=400)
    s.free()
    ctx.close()
    pairs = PAIR.findall(out.stdout)
    table = np.array([float(v) for _, v in RES.findall(out.stdout)])
    m = re.search(r"Solver: lanczos\((\d+), ncv=(\d+), (\w+)\) converged in: (\d+) iterations", out.stdout)
    prod = re.search(r"Operator products: (\d+), restarts: (\d+)", out.stdout)
    res = re.search(r"max \|\|A x - lambda x\|\|_2 = (\S+)", out.stdout)
    assert m and prod and res and len(pairs) == 4, out.stdout[-2000:]
    print(f"anderson:8 -eig 4 {' '.join(flags)}: {m.group(0)}; products {prod.group(1)}; values {[p[1] for p in pairs]}; "
          f"handle {want['values']}; residual line {res.group(1)}")
    assert (int(m.group(1)), int(m.group(2)), m.group(3)) == (4, 20 if ncv is None else ncv, which.lower())
    assert int(m.group(4)) == want["restarts"] and int(prod.group(1)) == want["products"] and int(prod.group(2)) == want["restarts"]
    # to the digits printed: the same handle on the same matrix gives the same bits
    for (i, val, est), wv, we in zip(pairs, want["values"], want["est"]):
        assert val == f"{wv:.16e}" and est == f"{we:.16e}", (i, val, wv)
    assert len(table) >= want["restarts"] and np.array_equal(table[:want["restarts"]], want["hist"])
    # the true residuals of converged pairs: estimate-sized, far below 1e-8 ||A||
    assert 0.0 < float(res.group(1)) <= 1e-8
    assert want["converged"]


@pytest.mark.parametrize("flags,needle", [(["-p", "j"], "ERROR: -p does not apply to -eig K"), (["-perm", "rcm"], "ERROR: -perm does not apply to -eig K"),
                                          (["-scale", "1"], "ERROR: -scale does not apply to -eig K"),
                                          (["-unfused"], "ERROR: -unfused does not apply to -eig K"),
                                          (["-hostscalars"], "ERROR: -hostscalars does not apply to -eig K"),
                                          (["-ncv", "4"], "ERROR: -ncv M"), (["-which", "xx"], "ERROR: -which sa|la|lm")])
def test_flags_that_do_not_apply_are_refused(flags, needle):
    out = cli("anderson:8", "-eig", "4", *flags)
    assert out.returncode != 0 and needle in out.stderr


def test_eig_needs_its_count():
    for args in (["-eig"], ["-eig", "x"], ["-eig", "0"]):
        out = cli("anderson:8", *args)
        assert out.returncode != 0 and "ERROR: -eig K" in out.stderr


@pytest.mark.parametrize("method", ["-cg", "-mr"])
@pytest.mark.parametrize("flags,needle", [(["-which", "la"], "ERROR: -which is an option of the eigensolver: it needs the method -eig K"),
                                          (["-ncv", "24"], "ERROR: -ncv M is an option of the eigensolver: it needs the method -eig K")])
def test_eig_options_need_the_method(method, flags, needle):
    out = cli("anderson:8", method, *flags)
    assert out.returncode != 0 and needle in out.stderr


def test_a_command_line_without_eig_prints_what_it_printed_before():
    """-mr on the same generator: the table is the MINRES handle's history to the digits printed, and no line of the
    eigensolver's appears."""
    from basic_iterative_solvers_amd import Context
    out = cli("anderson:8,shift=0.3", "-mr")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    ctx = Context()
    dA = ctx.gen_anderson(8, shift=0.3)
    n = dA.n_rows
    b, x = ctx.upload(np.ones(n)), ctx.upload(np.full(n, 0.1))
    mr = ctx.minres(dA, b, x)
    mr.init(1e-14)
    mr.iterate(1000)
    iters, conv, hist = mr.status()
    mr.free()
    ctx.close()
    table = [v for _, v in RES.findall(out.stdout)]
    m = re.search(r"Solver: minres (converged in: |did not converge after )(\d+) iterations", out.stdout)
    assert m and int(m.group(2)) == iters and m.group(1).startswith("converged") == conv
    assert table[:iters + 1] == [f"{h:.16e}" for h in hist]
    for word in ("lanczos", "lambda_", "Operator products", "max ||A x - lambda x||"):
        assert word not in out.stdout
    out = cli("anderson:8", "-nosuchmethod")
    assert out.returncode != 0 and "-eig K (thick-restart Lanczos" in out.stdout and "-lsmr (LSMR" in out.stdout
