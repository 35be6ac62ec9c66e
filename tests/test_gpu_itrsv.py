"""GPU: the iterative triangular solve (bis_itrsv), the ILU(0) apply built on it (preconditioner type 8, `-p ilu0it`) and
the CLI's `-inner K`.

bis_itrsv is defined step by step (include/bis_hip.h): x_0 = D_inv * b, x_{k+1} = (b - T x_k) * D_inv with T x_k exactly
bis_spmv's value and the subtraction and multiplication rounded separately -- so every check of the primitive here is bit
for bit, against bis_spmv on the device followed by that arithmetic in numpy."""
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import HIST_TOL, OptionScope, hist_dev, random_spmv_case
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

KTOL = 1e-13  # kernel-level relative tolerance, SURVEY.md 8d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "basic_iterative_solvers_amd", "host", "basic_iterative_solvers")
RES = re.compile(r"\|\|A\*x_(\d+) - b\|\|_2 = (\S+)")

FUSED = "itrsv_fused_rowblock"


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    info = c.device_info()
    assert info["arch"].startswith("gfx950")
    yield c
    c.close()


def strict_triangles(A):
    """Host CRS of the strict lower and strict upper part of the square part of A (entries keep their order)."""
    n = A.n_rows
    rows = np.repeat(np.arange(n), np.diff(A.row_ptr))
    out = []
    for keep in (A.col < rows, (A.col > rows) & (A.col < n)):
        rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int64)
        out.append(CRS(n, rp, A.col[keep].astype(np.int32), A.val[keep]))
    return out


def identity_cases(ctx):
    """(tag, device triangle, D_inv as numpy) -- built under the options in effect when called.  Generator matrices
    (split on the device), three random SpMV cases made strictly triangular, a triangle with runs of empty rows, n = 1."""
    rng = np.random.default_rng(77)
    for tag, gen in (("hpcg 16x12x10", lambda: ctx.gen_hpcg(16, 12, 10)), ("anderson 14", lambda: ctx.gen_anderson(14, shift=9.0)),
                     ("fem 6x5x4", lambda: ctx.gen_fem(6, 5, 4))):
        dA = gen()
        L, U, D, Dinv = ctx.split_strict(dA)
        dinv = Dinv.to_host()
        yield tag + " L", L, dinv
        yield tag + " U", U, dinv
        D.free(); Dinv.free(); dA.free()
    for seed in (3, 7, 11):
        A, _, _, info = random_spmv_case(seed)
        L, U = strict_triangles(A)
        dinv = 1.0 / rng.uniform(1.0, 4.0, A.n_rows)
        yield f"random{seed} L {info}", ctx.matrix(L), dinv
        yield f"random{seed} U {info}", ctx.matrix(U), dinv
    n = 3000  # empty rows: the first five, every third, a run in the middle
    lens = rng.integers(1, 9, n)
    lens[:5] = 0
    lens[::3] = 0
    lens[1500:1600] = 0
    lens = np.minimum(lens, np.arange(n))
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(r, int(lens[r]), replace=False)) for r in range(n)]).astype(np.int32)
    yield "empty rows L", ctx.matrix(CRS(n, rp, col, rng.uniform(-1, 1, rp[-1]))), 1.0 / rng.uniform(1.0, 4.0, n)
    yield "n = 1", ctx.matrix(CRS(1, np.array([0, 0], dtype=np.int64), np.zeros(0, np.int32), np.zeros(0))), np.array([0.37])


def check_step_identity(ctx, tag, T, dinv):
    """bis_itrsv(n_sweeps = 0 .. 4) against the step-by-step composition; returns the path's name."""
    n = T.n_rows
    rng = np.random.default_rng(n)
    b = rng.uniform(-1, 1, n)
    db, dd = ctx.upload(b), ctx.upload(dinv)
    xk, tmp, x, work = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
    assert T.itrsv_kernel() == ""
    ref = [dinv * b]
    for k in range(4):
        xk.set(ref[-1])
        ctx.spmv(T, xk, tmp)
        ref.append((b - tmp.to_host()) * dinv)
    spmv_kernel, form = T.spmv_kernel(), T.spmv_stream_info()[3]
    for k in range(5):
        x.set(np.full(n, np.nan)); work.set(np.full(n, np.nan))
        ctx.itrsv(T, dd, db, x, work, k)
        got = x.to_host()
        assert np.array_equal(got, ref[k]), (tag, k, T.itrsv_kernel(), int(np.sum(got != ref[k])))
        assert np.array_equal(db.to_host(), b) and np.array_equal(dd.to_host(), dinv), (tag, k)
    name = T.itrsv_kernel()
    want = FUSED if spmv_kernel.startswith("spmv_rowblock_kernel") else f"itrsv spmv+epilogue form={form}"
    print(f"{tag}: n = {n}, SpMV {spmv_kernel} (form {form}) -> {name}")
    assert name == want, (tag, spmv_kernel, form, name)
    for v in (db, dd, xk, tmp, x, work):
        v.free()
    T.free()
    return name


def test_step_identity_both_paths(ctx):
    """Check 1: bit for bit, n_sweeps 0 .. 4, under the default options (the dictionary matrices take the SpMV + epilogue
    path) and with the dictionary and win8 forms off (everything takes the fused row-block step)."""
    default = {tag: check_step_identity(ctx, tag, T, dinv) for tag, T, dinv in identity_cases(ctx)}
    assert any(v.startswith("itrsv spmv+epilogue form=") for v in default.values()), default
    for tag in ("hpcg 16x12x10 L", "anderson 14 U"):  # value dictionaries: never the CRS-value kernel
        assert default[tag] != FUSED, default
    with OptionScope(ctx, spmv_win8=0, spmv_valdict=0):
        plain = {tag: check_step_identity(ctx, tag, T, dinv) for tag, T, dinv in identity_cases(ctx)}
    assert set(plain.values()) == {FUSED}, plain


def test_nilpotency_on_multicolour_order(ctx):
    """Check 2: the triangles of a multi-colour order have one dependency level per colour, so n_colours steps ARE the
    solve: agreement with bis_sptrsv / bis_bsptrsv to the kernel gate 1e-13 |x|_inf; one step is not."""
    dB, _, n_col = ctx.multicolour(ctx.gen_hpcg(8))
    assert n_col == 8
    n = dB.n_rows
    L, U, D, Dinv = ctx.split_strict(dB)
    b = np.random.default_rng(5).uniform(-1, 1, n)
    db, x, work, xe = ctx.upload(b), ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
    for T, sweep in ((L, ctx.sptrsv), (U, ctx.bsptrsv)):
        sweep(T, xe, D, db)
        exact = xe.to_host()
        scale = np.max(np.abs(exact))
        ctx.itrsv(T, Dinv, db, x, work, n_col)
        err = np.max(np.abs(x.to_host() - exact)) / scale
        ctx.itrsv(T, Dinv, db, x, work, 1)
        err1 = np.max(np.abs(x.to_host() - exact)) / scale
        print(f"{T.itrsv_kernel()}: |x_{n_col} - x| = {err:.3e} |x|_inf, |x_1 - x| = {err1:.3e} |x|_inf")
        assert err <= KTOL
        assert err1 > 1e-6


@pytest.mark.parametrize("inner", [0, 1, 3])
def test_type8_is_two_itrsv_calls(ctx, inner):
    """Check 3: BIS_PC_ILU0_ITER = tmp <- itrsv(L, L_D, input), output <- itrsv(U, 1 / U_D, tmp), bit for bit, also with
    output aliasing input; input is left alone otherwise; tmp / work that alias an operand are refused."""
    from basic_iterative_solvers_amd import BisError, PC
    assert PC["ilu0it"] == 8
    dA = ctx.gen_fem(7, 6, 5)
    n = dA.n_rows
    Ls, L_D, Us, U_D = ctx.ilu0(dA)
    assert np.array_equal(L_D.to_host(), np.ones(n))
    Uinv = ctx.alloc(n)
    ctx.elemwise_div_vectors(Uinv, L_D, U_D)
    y = np.random.default_rng(9).uniform(-1, 1, n)
    inp, out, tmp, work, t2, w2, want = (ctx.upload(y), ctx.alloc(n), ctx.alloc(n), ctx.alloc(n), ctx.alloc(n), ctx.alloc(n),
                                         ctx.alloc(n))
    ctx.itrsv(Ls, L_D, inp, t2, w2, inner)
    ctx.itrsv(Us, Uinv, t2, want, w2, inner)
    ref = want.to_host()
    ctx.apply_preconditioner("ilu0it", n, Ls, Us, None, Uinv, L_D, None, out, inp, tmp, work, inner=inner)
    assert np.array_equal(out.to_host(), ref)
    assert np.array_equal(inp.to_host(), y)
    ctx.apply_preconditioner("ilu0it", n, Ls, Us, None, Uinv, L_D, None, inp, inp, tmp, work, inner=inner)  # in place
    assert np.array_equal(inp.to_host(), ref)
    if inner == 3:  # against the exact ILU(0) apply: three steps are a preconditioner, not the solve
        inp.set(y)
        ctx.apply_preconditioner("ilu0", n, Ls, Us, None, None, L_D, U_D, out, inp, tmp, work)
        gap = np.max(np.abs(out.to_host() - ref)) / np.max(np.abs(ref))
        print(f"fem 7x6x5: |ilu0it(3) - ilu0| = {gap:.3e} |z|_inf")
        assert 0.0 < gap < 1.0
        for bad in (dict(tmp=work), dict(tmp=inp), dict(work=out)):
            kw = dict(tmp=tmp, work=work)
            kw.update(bad)
            with pytest.raises(BisError):
                ctx.apply_preconditioner("ilu0it", n, Ls, Us, None, Uinv, L_D, None, out, inp, kw["tmp"], kw["work"], inner=inner)


def test_type8_through_the_fused_cg(ctx):
    """bis_cg_set_preconditioner reaches type 8 through bis_apply_preconditioner (as does the block-Jacobi use of the
    distributed CG): on the multi-colour order with inner = n_colours the history is the exact ILU(0) run's."""
    dB, _, n_col = ctx.multicolour(ctx.gen_hpcg(8))
    n = dB.n_rows
    Ls, L_D, Us, U_D = ctx.ilu0(dB)
    Uinv = ctx.alloc(n)
    ctx.elemwise_div_vectors(Uinv, L_D, U_D)
    hists = {}
    for pc, inner in (("ilu0", 0), ("ilu0it", n_col)):
        b, x = ctx.upload(np.full(n, 1.0)), ctx.upload(np.full(n, 0.1))
        cg = ctx.cg(dB, b, x)
        cg.set_preconditioner(pc, Ls=Ls, Us=Us, A_D=L_D, A_D_inv=Uinv, L_D=L_D, U_D=U_D, inner=inner)
        cg.init(1e-14)
        cg.iterate(200)
        iters, conv, hist = cg.status()
        assert conv
        hists[pc] = (iters, hist)
        cg.free()
    print({k: v[0] for k, v in hists.items()}, hist_dev(hists["ilu0it"][1], hists["ilu0"][1]))
    assert abs(hists["ilu0it"][0] - hists["ilu0"][0]) <= 2
    assert hist_dev(hists["ilu0it"][1], hists["ilu0"][1]) <= HIST_TOL["cg"]


def cli(*args):
    assert os.path.exists(BIN), "host binary not built (make -C basic_iterative_solvers_amd/host)"
    out = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"(converged in: |did not converge after )(\d+) iterations", out.stdout)
    assert m, out.stdout[-1500:]
    return dict(hist=np.array([float(v) for _, v in RES.findall(out.stdout)]), iters=int(m.group(2)),
                converged=m.group(1).startswith("converged"), stdout=out.stdout)


def test_cli_exact_limit_matches_ilu0():
    """Check 4: hpcg:16 -perm mc -cg: with -inner <n_colours> the iterative solves are exact, and the residual history is
    that of -p ilu0 on the same command within HIST_TOL["cg"], the stopping iterations within 2."""
    base = ["hpcg:16", "-cg", "-perm", "mc"]
    exact = cli(*base, "-p", "ilu0")
    n_col = int(re.search(r"multi-colour reordering: (\d+) colours", exact["stdout"]).group(1))
    assert n_col == 8
    it = cli(*base, "-p", "ilu0it", "-inner", str(n_col))
    assert f"with preconditioner: incomplete LU(0), iterative solves ({n_col})" in it["stdout"]
    dev = hist_dev(it["hist"], exact["hist"])
    print(f"ilu0 {exact['iters']} iterations, ilu0it -inner {n_col} {it['iters']}; max |dr| / r0 = {dev:.3e}")
    assert exact["converged"] and it["converged"]
    assert dev <= HIST_TOL["cg"]
    assert abs(it["iters"] - exact["iters"]) <= 2


def test_cli_truncated_solves_converge():
    """Check 5: fem:20,20,20 -bi -p ilu0it -inner 1 converges to the CLI's tolerance (1e-14 r0 within 1000 iterations).

    K = 1 comes from a CPU model, not from this run: the CLI's BiCGSTAB (host/methods/bicgstab.hpp) in numpy on the oracle's
    gen_fem(20, 20, 20) with the oracle's ILU(0) factors and both solves truncated to K steps.  The matrix is strongly
    diagonally dominant, so the model converges for every K: K = 0 (no step at all: z = U_D^-1 r) in 64 iterations,
    K = 1 in 37, K = 2 and 3 in 22, K = 4 in 21, K = 5 in 20, K = 6 and 8 in 21; exact solves need 21.  K = 1 is the
    smallest count that runs a step, and its 37 iterations leave a factor of 27 to the limit of 1000."""
    r = cli("fem:20,20,20", "-bi", "-p", "ilu0it", "-inner", "1")
    print(f"fem:20,20,20 -bi -p ilu0it -inner 1: {r['iters']} iterations, converged {r['converged']}")
    assert "with preconditioner: incomplete LU(0), iterative solves (1)" in r["stdout"]
    assert r["converged"]
    assert r["hist"][-1] < 1e-14 * r["hist"][0]


def test_cli_inner_flag_drives_two_stage():
    """-inner also sets the inner sweeps of 2st / s2st; without the flag they run the compile-time count (0) as before."""
    plain = cli("hpcg:8", "-cg", "-p", "s2st")
    zero = cli("hpcg:8", "-cg", "-p", "s2st", "-inner", "0")
    two = cli("hpcg:8", "-cg", "-p", "s2st", "-inner", "2")
    assert np.array_equal(plain["hist"], zero["hist"])
    assert two["converged"]
    m = min(len(two["hist"]), len(plain["hist"]))
    assert m > 2 and not np.array_equal(two["hist"][1:m], plain["hist"][1:m])  # another preconditioner: another history


def test_argument_checks(ctx):
    """Check 6: x == b, x == work, a negative sweep count -> BIS_ERR_INVALID (status 2), nothing computed."""
    from basic_iterative_solvers_amd import BisError
    dA = ctx.gen_hpcg(4)
    L, U, D, Dinv = ctx.split_strict(dA)
    n = dA.n_rows
    b, x, work = ctx.upload(np.ones(n)), ctx.upload(np.full(n, 7.0)), ctx.alloc(n)
    for args in ((L, Dinv, b, b, work, 2), (L, Dinv, b, x, x, 2), (L, Dinv, b, x, work, -1), (U, Dinv, b, Dinv, work, 1),
                 (U, Dinv, b, x, b, 1)):
        with pytest.raises(BisError, match="status 2"):
            ctx.itrsv(*args)
    assert np.array_equal(x.to_host(), np.full(n, 7.0)) and np.array_equal(b.to_host(), np.ones(n))
    ctx.itrsv(L, Dinv, b, x, None, 0)  # no step: work is not needed
    assert np.array_equal(x.to_host(), Dinv.to_host())
