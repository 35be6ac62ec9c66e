"""GPU: the host CLI's `-mg smooth=1[,pomega=X]` -- smoothed aggregation behind `-p mg` (bis_mg_create_smoothed): CG needs
fewer iterations than with the unsmoothed hierarchy of the same command line, the hierarchy line names the smoothed
prolongators and is otherwise worded as before, the reordered input beats the unpreconditioned count, GMRES takes the fixed
operator, and what cannot be read is refused."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "basic_iterative_solvers_amd", "host", "basic_iterative_solvers")
LINE = re.compile(r"^multigrid: .*$", re.M)
# the hierarchy line as it has been worded since -p mg exists
PLAIN = re.compile(r"^multigrid: (\d+) levels, rows \d+( / \d+)*, operator complexity [0-9.]+, aggregates( none| (grid|mis)( / (grid|mis))*)$")


def cli(*args):
    assert os.path.exists(BIN), "host binary not built (make -C basic_iterative_solvers_amd/host)"
    return subprocess.run([BIN] + list(args), capture_output=True, text=True, timeout=300)


def solve(*args):
    out = cli(*args)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"(converged in: |did not converge after )(\d+) iterations", out.stdout)
    assert m, out.stdout[-1500:]
    return dict(iters=int(m.group(2)), converged=m.group(1).startswith("converged"), stdout=out.stdout)


def test_cg_needs_fewer_iterations_and_the_line_says_so():
    plain = solve("hpcg:16", "-cg", "-p", "mg")
    smooth = solve("hpcg:16", "-cg", "-p", "mg", "-mg", "smooth=1")
    lp, ls = LINE.findall(plain["stdout"]), LINE.findall(smooth["stdout"])
    print(f"hpcg:16 -cg -p mg: {plain['iters']} iterations, {lp}; -mg smooth=1: {smooth['iters']} iterations, {ls}")
    assert plain["converged"] and smooth["converged"] and smooth["iters"] < plain["iters"]
    assert len(lp) == 1 and PLAIN.match(lp[0]), lp
    assert lp[0] == "multigrid: 3 levels, rows 4096 / 512 / 64, operator complexity 1.11967, aggregates grid / grid"  # the line as it has always read
    assert "smoothed" not in plain["stdout"]
    suffix = ", smoothed prolongators (omega 1.33333)"
    assert len(ls) == 1 and ls[0].endswith(suffix) and PLAIN.match(ls[0][:-len(suffix)]), ls
    explicit = solve("hpcg:16", "-cg", "-p", "mg", "-mg", "smooth=0")  # named: what a command line without smooth= prints and computes
    assert LINE.findall(explicit["stdout"]) == lp and explicit["iters"] == plain["iters"]
    half = solve("hpcg:16", "-cg", "-p", "mg", "-mg", "smooth=1,pomega=0.5")
    assert half["converged"] and LINE.findall(half["stdout"])[0].endswith(", smoothed prolongators (omega 0.5)")


def test_the_reordered_input_beats_the_unpreconditioned_count():
    none = solve("hpcg:16", "-cg", "-perm", "rcm")
    smooth = solve("hpcg:16", "-cg", "-perm", "rcm", "-p", "mg", "-mg", "smooth=1")
    print(f"hpcg:16 -cg -perm rcm: {none['iters']} iterations unpreconditioned, {smooth['iters']} with -p mg -mg smooth=1; "
          f"{LINE.findall(smooth['stdout'])}")
    assert none["converged"] and smooth["converged"] and smooth["iters"] < none["iters"]
    assert "aggregates mis" in LINE.findall(smooth["stdout"])[0]


def test_gmres_takes_the_smoothed_hierarchy():
    run = solve("hpcg:16", "-gm", "-p", "mg", "-mg", "smooth=1")
    assert run["converged"] and LINE.findall(run["stdout"])[0].endswith("(omega 1.33333)")


def test_what_cannot_be_read_is_refused():
    for bad, args in (("pomega=2", "smooth=1,pomega=2"), ("pomega=1", "pomega=1"), ("pomega=0", "smooth=1,pomega=0"), ("smooth=2", "smooth=2"),
                      ("pomega=1", "limit=64,pomega=1,smooth=0")):
        out = cli("hpcg:8", "-cg", "-p", "mg", "-mg", args)
        assert out.returncode != 0 and "cannot read" in out.stderr and bad in out.stderr, (args, out.stderr)
        assert "converged" not in out.stdout
