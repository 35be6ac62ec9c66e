"""GPU: the host CLI's `-mg cycle=v|w|k|kgcr,klev=N` -- the W- and K-cycles of `-p mg` (bis_mg_set_cycle): the hierarchy
line stays as it was, a second line names the cycle when it is not V, CG needs strictly fewer iterations with K than with W
than with V (fused and -unfused), BiCGSTAB takes the GCR K-cycle, GMRES refuses a K-cycle and takes W, and what cannot be
read is refused."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "basic_iterative_solvers_amd", "host", "basic_iterative_solvers")
LINE = re.compile(r"^multigrid: .*$", re.M)
CYCLE_LINE = re.compile(r"^multigrid cycle: (.*), transitions (.*)$", re.M)


def cli(*args):
    assert os.path.exists(BIN), "host binary not built (make -C basic_iterative_solvers_amd/host)"
    return subprocess.run([BIN] + list(args), capture_output=True, text=True, timeout=300)


def solve(*args):
    out = cli(*args)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"(converged in: |did not converge after )(\d+) iterations", out.stdout)
    assert m, out.stdout[-1500:]
    return dict(iters=int(m.group(2)), converged=m.group(1).startswith("converged"), stdout=out.stdout)


@pytest.mark.parametrize("extra", [(), ("-unfused",)], ids=["fused", "unfused"])
def test_cg_iterations_fall_from_v_to_w_to_k(extra):
    base = ("hpcg:32", "-cg", "-p", "mg") + extra
    v = solve(*base, "-mg", "limit=64")
    w = solve(*base, "-mg", "limit=64,cycle=w")
    k = solve(*base, "-mg", "limit=64,cycle=k")
    first = [LINE.findall(r["stdout"]) for r in (v, w, k)]
    print(f"hpcg:32 -cg -p mg {' '.join(extra)}: V {v['iters']}, W {w['iters']}, K {k['iters']} iterations; {first[0]}")
    assert len(first[0]) == 1 and first[0][0].startswith("multigrid: 4 levels, rows 32768 / 4096 / 512 / 64, ")
    assert first[1] == first[0] and first[2] == first[0]
    assert not CYCLE_LINE.search(v["stdout"]) and "multigrid cycle" not in v["stdout"]
    assert CYCLE_LINE.findall(w["stdout"]) == [("W", "0..1")] and CYCLE_LINE.findall(k["stdout"]) == [("K (conjugate)", "0..1")]
    for r in (w, k):  # the cycle line follows the hierarchy line
        assert re.search(r"^multigrid: .*\nmultigrid cycle: ", r["stdout"], re.M)
    assert v["converged"] and w["converged"] and k["converged"]
    assert k["iters"] < w["iters"] < v["iters"]
    explicit = solve(*base, "-mg", "limit=64,cycle=v")  # V named: what a command line without cycle= prints and computes
    assert not CYCLE_LINE.search(explicit["stdout"]) and explicit["iters"] == v["iters"]


def test_klev_limits_the_transitions():
    run = solve("hpcg:32", "-cg", "-p", "mg", "-mg", "limit=64,cycle=k,klev=1")
    assert CYCLE_LINE.findall(run["stdout"]) == [("K (conjugate)", "0..0")] and run["converged"]
    run = solve("hpcg:32", "-cg", "-p", "mg", "-mg", "limit=64,cycle=w,klev=7")
    assert CYCLE_LINE.findall(run["stdout"]) == [("W", "0..1")]


def test_bicgstab_with_the_gcr_k_cycle_converges():
    run = solve("unstr:8,8,8", "-bi", "-p", "mg", "-mg", "cycle=kgcr")
    print(f"unstr:8,8,8 -bi -p mg -mg cycle=kgcr: {run['iters']} iterations; {LINE.findall(run['stdout'])}")
    assert run["converged"]
    assert len(CYCLE_LINE.findall(run["stdout"])) == 1 and CYCLE_LINE.findall(run["stdout"])[0][0] == "K (GCR)"
    deep = solve("unstr:8,8,8", "-bi", "-p", "mg", "-mg", "cycle=kgcr,limit=8")  # (enough levels for the cycle to act)
    print(f"... limit=8: {deep['iters']} iterations; {LINE.findall(deep['stdout'])}")
    assert deep["converged"]


def test_gmres_refuses_a_k_cycle_and_takes_w():
    for cycle in ("k", "kgcr"):
        out = cli("hpcg:16", "-gm", "-p", "mg", "-mg", "cycle=" + cycle)
        assert out.returncode != 0 and "not a fixed preconditioner" in out.stderr and "-gm" in out.stderr
        assert "converged" not in out.stdout
    run = solve("hpcg:16", "-gm", "-p", "mg", "-mg", "cycle=w,limit=8")
    assert run["converged"] and CYCLE_LINE.findall(run["stdout"]) == [("W", "0..1")]


def test_what_cannot_be_read_is_refused():
    for bad in ("cycle=x", "klev=-1", "cycle=", "klev=two"):
        out = cli("hpcg:8", "-cg", "-p", "mg", "-mg", bad)
        assert out.returncode != 0 and "cannot read" in out.stderr and bad in out.stderr, bad
