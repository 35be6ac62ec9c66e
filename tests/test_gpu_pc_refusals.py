"""GPU: what the six solver handles' set_preconditioner refuses -- bis_cg_*, bis_mcg_*, bis_mbicgstab_*, bis_mgmres_*,
bis_fgmres_*, bis_minres_* -- pinned by status AND by the full text of bis_last_error, through one table of bad calls.  Every
case is a host-side argument check that returns before any launch; the only solves are one `init` per kind.

The order of the checks is part of what a caller sees, and it differs by family:
  lock-step (mcg, mbicgstab, mgmres): MG (6) before the null check of the handle; range; "call it before"; the two-stage types
      (6); outer_iters != 1 (6); the block-Jacobi operand; null triangle; triangle size; null diagonal.
  single (fgmres, minres): range; "call it before"; MG operand (2) then outer_iters != 1 (6); the same for block Jacobi; null
      triangle; triangle size; null diagonal (not when n == 0).
  cg: range; "call it before"; FSAI's factors; MG / block Jacobi operand (2) then distributed or outer_iters != 1 (6).  Null
      triangles and diagonals are NOT refused at set time.

System: the 27-point matrix on 3 x 3 x 3 (27 rows) with its triangles and diagonals, the same on 2 x 2 x 2 (8 rows) for the
"of another size" cases, a matrix without rows; one MG hierarchy and one block-Jacobi handle on each size; k = 2 columns,
restart 3."""
import ctypes as C

import numpy as np
import pytest

from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

KINDS = ("cg", "mcg", "mbicgstab", "mgmres", "fgmres", "minres")
LOCKSTEP = ("mcg", "mbicgstab", "mgmres")
K, RESTART = 2, 3

# the sentences after "bis_<kind>_set_preconditioner: "
BAD = "bad arguments"
BEFORE = "call it before bis_{kind}_init / bis_{kind}_iterate"
MG_MULTI = "the multigrid preconditioner has no multi-vector form"
TWO_MULTI = "the two-stage Gauss-Seidel types have no multi-vector form"
OUTER_MULTI = "outer_iters must be 1 on interleaved blocks"
MG_OPERAND = "MG needs the operand of a hierarchy of the solver's size in L_strict"
BJ_OPERAND = "block Jacobi needs the operand of a handle of the solver's size in L_strict"
MG_OUTER = "MG with outer_iters != 1 is not built"
BJ_OUTER = "block Jacobi with outer_iters != 1 is not built"
MG_OUTER_CG = "MG on a distributed handle, or with outer_iters != 1, is not built"
BJ_OUTER_CG = "block Jacobi on a distributed handle, or with outer_iters != 1, is not built"
FSAI_CG = "FSAI needs both factors, of the solver's size"
TRI_NULL = "the type needs a triangle that is null"
TRI_SIZE = "a triangle of another size"
DIAG_NULL = "the type needs a diagonal that is null"
OK = (0, None)

# what each type reads, as the lock-step and the single handles check it
NEEDS = {
    "gs": ("Ls", "A_D"),
    "bgs": ("Us", "A_D"),
    "sgs": ("Ls", "Us", "A_D"),
    "ilu0": ("Ls", "Us", "L_D", "U_D"),
    "ilu0it": ("Ls", "Us", "A_D_inv", "L_D"),
    "fsai": ("Ls", "Us"),
}
DIAGS = ("A_D", "A_D_inv", "L_D", "U_D")


def family(kind):
    return "cg" if kind == "cg" else "lockstep" if kind in LOCKSTEP else "single"


class System:
    def __init__(self, ctx, dA):
        self.ctx, self.dA, self.n = ctx, dA, dA.n_rows
        self.b, self.x = ctx.upload(np.ones(max(2, self.n * K))), ctx.upload(np.zeros(max(2, self.n * K)))
        if self.n:
            self.Ls, self.Us, self.D, self.Dinv = ctx.split_strict(dA)
            self.mg, self.bj = ctx.mg(dA), ctx.bjacobi(dA, block_size=3)
        else:  # the matrix without rows is its own triangle of the right size
            self.Ls = self.Us = dA

    def handle(self, kind):
        ctx, dA, b, x = self.ctx, self.dA, self.b, self.x
        return dict(cg=lambda: ctx.cg(dA, b, x), mcg=lambda: ctx.mcg(dA, b, x, K), mbicgstab=lambda: ctx.mbicgstab(dA, b, x, K),
                    mgmres=lambda: ctx.mgmres(dA, b, x, K, restart=RESTART), fgmres=lambda: ctx.fgmres(dA, b, x, restart=RESTART),
                    minres=lambda: ctx.minres(dA, b, x))[kind]()

    def operands(self, pc):
        """The accepted control call of `pc`: what the type needs, everything else null."""
        full = dict(Ls=self.Ls, Us=self.Us, A_D=self.D, A_D_inv=self.Dinv, L_D=self.D, U_D=self.D)
        return {name: full[name] for name in NEEDS[pc]}


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


@pytest.fixture(scope="module")
def systems(ctx):
    empty = ctx.matrix(CRS(0, np.zeros(1, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0)))
    return dict(s27=System(ctx, ctx.gen_hpcg(3, 3, 3)), s8=System(ctx, ctx.gen_hpcg(2, 2, 2)), s0=System(ctx, empty))


def set_pc(ctx, kind, h, pc, Ls=None, Us=None, A_D=None, A_D_inv=None, L_D=None, U_D=None, outer=1, inner=0):
    """(status, bis_last_error) of bis_<kind>_set_preconditioner on the raw handle h (None: a null handle)."""
    from basic_iterative_solvers_amd import PC

    def m(v):
        return v.h if v is not None else C.c_void_p()

    def p(v):
        return C.c_void_p(v.ptr) if v is not None else C.c_void_p()
    st = getattr(ctx.lib, f"bis_{kind}_set_preconditioner")(
        ctx.h, h, C.c_int(PC[pc] if isinstance(pc, str) else pc), m(Ls), m(Us), p(A_D), p(A_D_inv), p(L_D), p(U_D),
        C.c_int(outer), C.c_int(inner))
    return st, ctx.lib.bis_last_error(ctx.h).decode()


def check(ctx, kind, what, expect, h, pc, **args):
    status, sentence = expect
    got = set_pc(ctx, kind, h, pc, **args)
    print(f"{kind}: {what}: status {got[0]}" + (f", {got[1]!r}" if got[0] else ""))
    if status == 0:
        assert got[0] == 0, (what, got)
    else:
        assert got == (status, f"bis_{kind}_set_preconditioner: " + sentence.format(kind=kind)), what


@pytest.mark.parametrize("kind", KINDS)
def test_null_handle_and_range(ctx, systems, kind):
    s = systems["s27"]
    fam = family(kind)
    check(ctx, kind, "null handle, j", (2, BAD), None, "j", A_D=s.D)
    check(ctx, kind, "null handle, mg", (6, MG_MULTI) if fam == "lockstep" else (2, BAD), None, "mg", Ls=s.mg.operand)
    hd = s.handle(kind)
    check(ctx, kind, "type -1", (2, BAD), hd.h, -1)
    check(ctx, kind, "type 12", (2, BAD), hd.h, 12)
    check(ctx, kind, "outer 0", (2, BAD), hd.h, "j", A_D=s.D, outer=0)
    check(ctx, kind, "inner -1", (2, BAD), hd.h, "j", A_D=s.D, inner=-1)
    for two in ("2st", "s2st"):  # the range check wins over "no multi-vector form"
        check(ctx, kind, f"{two}, outer 0", (2, BAD), hd.h, two, Ls=s.Ls, Us=s.Us, A_D=s.D, A_D_inv=s.Dinv, outer=0)
    hd.free()


@pytest.mark.parametrize("kind", LOCKSTEP)
def test_lockstep_unsupported(ctx, systems, kind):
    s, s8 = systems["s27"], systems["s8"]
    hd = s.handle(kind)
    for two in ("2st", "s2st"):
        check(ctx, kind, two, (6, TWO_MULTI), hd.h, two, Ls=s.Ls, Us=s.Us, A_D=s.D, A_D_inv=s.Dinv)
    check(ctx, kind, "sgs, outer 2", (6, OUTER_MULTI), hd.h, "sgs", outer=2, **s.operands("sgs"))
    check(ctx, kind, "bj without operand, outer 2", (6, OUTER_MULTI), hd.h, "bj", outer=2)  # the outer check comes first
    check(ctx, kind, "bj of another size, outer 2", (6, OUTER_MULTI), hd.h, "bj", Ls=s8.bj.operand, outer=2)
    hd.free()


@pytest.mark.parametrize("kind", KINDS)
def test_mg_and_bj_operands(ctx, systems, kind):
    s, s8 = systems["s27"], systems["s8"]
    fam = family(kind)
    mg_operand = dict(lockstep=(6, MG_MULTI), single=(2, MG_OPERAND), cg=(2, MG_OPERAND))[fam]
    mg_outer = dict(lockstep=(6, MG_MULTI), single=(6, MG_OUTER), cg=(6, MG_OUTER_CG))[fam]
    bj_outer = dict(lockstep=(6, OUTER_MULTI), single=(6, BJ_OUTER), cg=(6, BJ_OUTER_CG))[fam]
    hd = s.handle(kind)
    check(ctx, kind, "mg, no operand", mg_operand, hd.h, "mg")
    check(ctx, kind, "mg, a matrix that is no operand", mg_operand, hd.h, "mg", Ls=s.Ls)
    check(ctx, kind, "mg, a block-Jacobi operand", mg_operand, hd.h, "mg", Ls=s.bj.operand)
    check(ctx, kind, "mg, operand of another size", mg_operand, hd.h, "mg", Ls=s8.mg.operand)
    check(ctx, kind, "mg, operand of another size, outer 2", mg_operand, hd.h, "mg", Ls=s8.mg.operand, outer=2)
    check(ctx, kind, "mg, outer 2", mg_outer, hd.h, "mg", Ls=s.mg.operand, outer=2)
    check(ctx, kind, "mg", (6, MG_MULTI) if fam == "lockstep" else OK, hd.h, "mg", Ls=s.mg.operand)
    check(ctx, kind, "bj, no operand", (2, BJ_OPERAND), hd.h, "bj")
    check(ctx, kind, "bj, a matrix that is no operand", (2, BJ_OPERAND), hd.h, "bj", Ls=s.Ls)
    check(ctx, kind, "bj, a hierarchy's operand", (2, BJ_OPERAND), hd.h, "bj", Ls=s.mg.operand)
    check(ctx, kind, "bj, operand of another size", (2, BJ_OPERAND), hd.h, "bj", Ls=s8.bj.operand)
    if fam != "lockstep":  # (lock-step: test_lockstep_unsupported)
        check(ctx, kind, "bj, operand of another size, outer 2", (2, BJ_OPERAND), hd.h, "bj", Ls=s8.bj.operand, outer=2)
    check(ctx, kind, "bj, outer 2", bj_outer, hd.h, "bj", Ls=s.bj.operand, outer=2)
    check(ctx, kind, "bj", OK, hd.h, "bj", Ls=s.bj.operand)
    check(ctx, kind, "the BJ object's operand, nothing else read", OK, hd.h, "bj", Ls=s.bj.operand, Us=s8.Us)
    hd.free()


@pytest.mark.parametrize("pc", sorted(NEEDS))
@pytest.mark.parametrize("kind", KINDS)
def test_triangles_and_diagonals(ctx, systems, kind, pc):
    s, s8 = systems["s27"], systems["s8"]
    cg = kind == "cg"
    hd = s.handle(kind)
    good = s.operands(pc)
    check(ctx, kind, f"{pc}: control", OK, hd.h, pc, **good)
    for tri in ("Ls", "Us"):
        needed = tri in NEEDS[pc]
        if cg:  # only FSAI's factors are looked at
            null = size = (2, FSAI_CG) if pc == "fsai" else OK
        else:
            null, size = ((2, TRI_NULL), (2, TRI_SIZE)) if needed else (OK, OK)
        check(ctx, kind, f"{pc}: {tri} null", null, hd.h, pc, **{**good, tri: None})
        check(ctx, kind, f"{pc}: {tri} of another size", size, hd.h, pc, **{**good, tri: getattr(s8, tri)})
    if not cg and len([t for t in ("Ls", "Us") if t in NEEDS[pc]]) == 2:  # the null check comes before the size check
        check(ctx, kind, f"{pc}: Ls of another size, Us null", (2, TRI_NULL), hd.h, pc, **{**good, "Ls": s8.Ls, "Us": None})
    for diag in DIAGS:
        if diag in NEEDS[pc]:
            check(ctx, kind, f"{pc}: {diag} null", OK if cg else (2, DIAG_NULL), hd.h, pc, **{**good, diag: None})
    if not cg and "A_D" in NEEDS[pc]:  # the triangle checks come before the diagonal check
        tri = "Ls" if "Ls" in NEEDS[pc] else "Us"
        check(ctx, kind, f"{pc}: {tri} of another size, A_D null", (2, TRI_SIZE), hd.h, pc,
              **{**good, tri: getattr(s8, tri), "A_D": None})
    hd.free()  # (cg: its last accepted call may lack a diagonal -- freed without init)


@pytest.mark.parametrize("kind", KINDS)
def test_jacobi_diagonal(ctx, systems, kind):
    s = systems["s27"]
    hd = s.handle(kind)
    check(ctx, kind, "j without A_D", OK if kind == "cg" else (2, DIAG_NULL), hd.h, "j")
    check(ctx, kind, "none", OK, hd.h, "none")
    hd.free()


@pytest.mark.parametrize("kind", KINDS)
def test_no_rows_need_no_diagonals(ctx, systems, kind):
    s0, s8 = systems["s0"], systems["s8"]
    hd = s0.handle(kind)
    check(ctx, kind, "n = 0: j without A_D", OK, hd.h, "j")
    for pc in sorted(NEEDS):
        tris = {t: s0.dA for t in ("Ls", "Us") if t in NEEDS[pc]}
        check(ctx, kind, f"n = 0: {pc} without diagonals", OK, hd.h, pc, **tris)
        if kind != "cg" or pc == "fsai":  # the triangles are still checked
            tri = sorted(tris)[0]
            check(ctx, kind, f"n = 0: {pc}, {tri} null", (2, FSAI_CG if kind == "cg" else TRI_NULL), hd.h, pc, **{**tris, tri: None})
            check(ctx, kind, f"n = 0: {pc}, {tri} of another size", (2, FSAI_CG if kind == "cg" else TRI_SIZE), hd.h, pc,
                  **{**tris, tri: getattr(s8, tri)})
    hd.free()


@pytest.mark.parametrize("kind", KINDS)
def test_after_init(ctx, systems, kind):
    s = systems["s27"]
    hd = s.handle(kind)
    check(ctx, kind, "j", OK, hd.h, "j", A_D=s.D)
    hd.init(1e-6)
    check(ctx, kind, "after init: j", (2, BEFORE), hd.h, "j", A_D=s.D)
    check(ctx, kind, "after init: none", (2, BEFORE), hd.h, "none")
    check(ctx, kind, "after init: type 12", (2, BAD), hd.h, 12)  # the range check comes first
    check(ctx, kind, "after init: mg", (6, MG_MULTI) if family(kind) == "lockstep" else (2, BEFORE), hd.h, "mg")
    if family(kind) == "lockstep":  # ... and "call it before" ahead of the unsupported types
        check(ctx, kind, "after init: 2st", (2, BEFORE), hd.h, "2st", Ls=s.Ls, A_D_inv=s.Dinv)
        check(ctx, kind, "after init: outer 2", (2, BEFORE), hd.h, "j", A_D=s.D, outer=2)
    hd.free()
