"""GPU: bis_idr_* (right-preconditioned IDR(s) as a device schedule) against the numpy restatement of tests/idr_ref.py, whose
preconditioner apply is the device's own bis_apply_preconditioner and whose products and sums are numpy's on the host: the
two differ in the rounding of every product, sum and update, not in the method.

The gate is the project's BiCGSTAB gate (tests/helpers.py): 1e-10 r0 over the first three history entries, 1e-4 r0 over the
whole history; iteration counts within 3.  Two differently rounded restatements on the host (fp64 dots against longdouble
dots, tests/test_idr_ref_cpu.py) stay within 2.9e-9 r0 and 5.9e-13 r0 on these inputs, so the reference alone holds the gate.
The true residual || b - A x || of the returned x is held within a factor 10 of the restatement's own.

Inputs: a nonsymmetric band under one wave with an odd n (37), one of 600 rows and 25 diagonals, the 7-point
convection-diffusion stencil on 10^3 nodes with convection 0.8, a band of 40001 rows (79 workgroups' partial sums, an odd
tail), the unstructured generator on 8^3 nodes for MG and ILU(0), n = 1 and n = 0."""
import numpy as np
import pytest

from helpers import HIST_TOL, hist_dev
from idr_ref import hashed_shadow, idr
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

TOL = 1e-10
ITERS = 400
SS = [1, 2, 4, 8]
# input -> the preconditioners its parity cases run with (every type meets every s on some input)
CASES = {"band37": ["none", "j", "gs", "bj"], "band600": ["none", "gs", "ilu0"], "cd10": ["none", "j", "ilu0", "bj"],
         "band40k": ["none", "j"], "unstr8": ["none", "gs", "ilu0", "bj", "mg"]}
PARITY = [(m, pc, s) for m, pcs in CASES.items() for pc in pcs for s in SS]


def host_spmv(A, x):
    rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
    return np.bincount(rows, weights=A.val * x[A.col], minlength=A.n_rows)


def ns_band(n, half, seed=1):
    """Random nonsymmetric, strictly diagonally dominant band: the sub- and super-diagonals are drawn independently."""
    rng = np.random.default_rng(seed)
    lo = {d: rng.uniform(-1, 1, n - d) for d in range(1, half + 1)}  # entry (r, r - d) at index r - d
    up = {d: rng.uniform(-1, 1, n - d) for d in range(1, half + 1)}  # entry (r, r + d) at index r
    absum = np.zeros(n)
    for d in range(1, half + 1):
        absum[d:] += np.abs(lo[d])
        absum[:n - d] += np.abs(up[d])
    diag = absum * rng.uniform(1.1, 1.5, n) + 1e-3
    rows, cols, vals = [], [], []
    for d in range(-half, half + 1):
        r = np.arange(max(0, -d), min(n, n - d))
        rows.append(r)
        cols.append(r + d)
        vals.append(diag if d == 0 else (lo[-d] if d < 0 else up[d]))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return CRS(n, rp, cols[order].astype(np.int32), vals[order])


def convdiff(m, conv):
    """The 7-point stencil of -Laplace(u) + conv grad(u) on m^3 nodes, x fastest: diagonal 6, -(1 + conv) towards the lower
    neighbour and -(1 - conv) towards the upper one in every direction."""
    n = m ** 3
    idx = np.arange(n)
    coord = [idx % m, (idx // m) % m, idx // (m * m)]
    rows, cols, vals = [idx], [idx], [np.full(n, 6.0)]
    for axis, stride in enumerate((1, m, m * m)):
        lower, upper = coord[axis] > 0, coord[axis] < m - 1
        rows += [idx[lower], idx[upper]]
        cols += [idx[lower] - stride, idx[upper] + stride]
        vals += [np.full(lower.sum(), -(1.0 + conv)), np.full(upper.sum(), -(1.0 - conv))]
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return CRS(n, rp, cols[order].astype(np.int32), vals[order])


def host_matrix(name):
    """The inputs that are built on the host (unstr8 comes from the device's generator)."""
    return {"band37": lambda: ns_band(37, 5), "band600": lambda: ns_band(600, 12), "cd10": lambda: convdiff(10, 0.8),
            "band40k": lambda: ns_band(40001, 3), "one": lambda: CRS(1, np.array([0, 1], dtype=np.int64), np.zeros(1, np.int32), np.array([2.5]))}[name]()


def right_hand_side(n, seed=7):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, n), 0.1 * rng.uniform(-1, 1, n)


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


class Cache:
    """Per input: the matrix, its preconditioner operands, b and x0, and every reference and device solve made so far --
    built once, never changed."""

    def __init__(self, ctx):
        self.ctx, self.sys, self.refs, self.devs = ctx, {}, {}, {}

    def system(self, name):
        if name not in self.sys:
            ctx = self.ctx
            dA = ctx.gen_unstr(8, 8, 8) if name == "unstr8" else ctx.matrix(host_matrix(name))
            n = dA.n_rows
            e = dict(dA=dA, n=n, A=CRS(n, *dA.download()))
            e["Ls"], e["Us"], e["D"], e["Dinv"] = ctx.split_strict(dA)
            e["b"], e["x0"] = right_hand_side(n)
            e["tmp"], e["work"], e["in"], e["out"] = (ctx.alloc(n) for _ in range(4))
            self.sys[name] = e
        return self.sys[name]

    def precond(self, name, pc):
        """keyword arguments of IDR.set_preconditioner / the operands of apply_preconditioner for this type"""
        e, ctx = self.system(name), self.ctx
        if pc == "none":
            return {}
        if pc in ("j", "gs"):
            return dict(Ls=e["Ls"], Us=e["Us"], A_D=e["D"], A_D_inv=e["Dinv"], L_D=e["D"], U_D=e["D"])
        if pc == "ilu0":
            if "ilu" not in e:
                e["ilu"] = ctx.ilu0(e["dA"])
            iLs, iLD, iUs, iUD = e["ilu"]
            return dict(Ls=iLs, Us=iUs, L_D=iLD, U_D=iUD)
        if pc == "bj":
            if "bj" not in e:
                e["bj"] = ctx.bjacobi(e["dA"], block_size=4)
            return dict(Ls=e["bj"].operand)
        if "mg" not in e:
            e["mg"] = ctx.mg(e["dA"])
        return dict(Ls=e["mg"].operand)

    def apply(self, name, pc):
        """v -> M^-1 v by the device's bis_apply_preconditioner (None without a preconditioner)"""
        if pc == "none":
            return None
        e, ctx, kw = self.system(name), self.ctx, self.precond(name, pc)
        ops = tuple(kw.get(k) for k in ("Ls", "Us", "A_D", "A_D_inv", "L_D", "U_D"))

        def fn(v):
            e["in"].set(v)
            ctx.apply_preconditioner(pc, e["n"], *ops, e["out"], e["in"], e["tmp"], e["work"])
            return e["out"].to_host()
        return fn

    def ref(self, name, pc, s, P=None, tag=None, b=None, x0=None, tol=TOL, iters=ITERS):
        """The restatement's solve; a call with P, b, x0, tol or iters of its own names itself by `tag`."""
        key = (name, pc, s, tag)
        if key not in self.refs:
            e = self.system(name)
            self.refs[key] = idr(lambda v: host_spmv(e["A"], v), e["b"] if b is None else b, e["x0"] if x0 is None else x0, s, tol,
                                 iters, apply=self.apply(name, pc), P=P)
        return self.refs[key]

    def solve(self, name, pc, s, steps=(ITERS,), P=None, reinit_after=None, b=None, x0=None):
        """One device solve: the state after each entry of `steps` further iterations."""
        e, ctx = self.system(name), self.ctx
        db, dx = ctx.upload(e["b"] if b is None else b), ctx.upload(e["x0"] if x0 is None else x0)
        h = ctx.idr(e["dA"], db, dx, s)
        if pc in ("mg", "bj"):  # the MG / BJ object itself stands for its type and operand
            self.precond(name, pc)
            h.set_preconditioner(e[pc])
        elif pc != "none":
            h.set_preconditioner(pc, **self.precond(name, pc))
        if P is not None:
            h.set_shadow(P)
        r0 = h.init(TOL)
        if reinit_after is not None:  # a solve abandoned inside a cycle, then init again on the start vector
            h.iterate(reinit_after)
            dx.set(e["x0"] if x0 is None else x0)
            assert h.init(TOL) == r0
        out = []
        for k in steps:
            h.iterate(k)
            it, conv, hist = h.status()
            out.append(dict(iters=it, conv=conv, hist=hist, x=dx.to_host(), r0=r0))
        h.free(); db.free(); dx.free()
        return out

    def dev(self, name, pc, s):
        key = (name, pc, s)
        if key not in self.devs:
            self.devs[key] = self.solve(name, pc, s)[0]
        return self.devs[key]


@pytest.fixture(scope="module")
def cache(ctx):
    return Cache(ctx)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_state(a, b):
    return a["iters"] == b["iters"] and a["conv"] == b["conv"] and same_bits(a["hist"], b["hist"]) and same_bits(a["x"], b["x"])


def true_residual(e, x):
    return float(np.linalg.norm(e["b"] - host_spmv(e["A"], x)))


def check_parity(d, g, tag):
    k = min(3, len(d["hist"]), len(g["hist"]))
    first, whole = hist_dev(d["hist"][:k], g["hist"][:k]), hist_dev(d["hist"], g["hist"])
    print(f"{tag}: device {d['iters']} iterations, restatement {g['iters']}; first three entries apart {first:.3e} r0, whole "
          f"history {whole:.3e} r0")
    assert d["conv"] and g["conv"]
    assert first <= 1e-10
    assert whole <= HIST_TOL["bi"]
    assert abs(d["iters"] - g["iters"]) <= 3


@pytest.mark.parametrize("name,pc,s", PARITY, ids=[f"{m}-{pc}-s{s}" for m, pc, s in PARITY])
def test_parity_with_the_restatement(cache, name, pc, s):
    d, g = cache.dev(name, pc, s), cache.ref(name, pc, s)
    assert d["hist"][0] == d["r0"] and len(d["hist"]) == d["iters"] + 1
    check_parity(d, g, f"{name} {pc} s={s}")


@pytest.mark.parametrize("name,pc,s", PARITY, ids=[f"{m}-{pc}-s{s}" for m, pc, s in PARITY])
def test_true_residual(cache, name, pc, s):
    e = cache.system(name)
    d, g = cache.dev(name, pc, s), cache.ref(name, pc, s)
    res_d, res_g = true_residual(e, d["x"]), true_residual(e, g["x"])
    print(f"{name} {pc} s={s}: || b - A x || device {res_d:.3e} = {res_d / d['r0']:.3e} r0 (last entry {d['hist'][-1] / d['r0']:.3e} r0), "
          f"restatement {res_g:.3e} = {res_g / d['r0']:.3e} r0")
    assert res_d <= 10.0 * res_g


@pytest.mark.parametrize("name,pc,s", [("band37", "none", 4), ("band40k", "j", 8), ("unstr8", "ilu0", 2), ("cd10", "bj", 4)])
def test_determinism_and_reuse(cache, name, pc, s):
    first = cache.dev(name, pc, s)
    again = cache.solve(name, pc, s)[0]
    assert same_state(first, again)  # two solves, the same bits
    split, whole = cache.solve(name, pc, s, steps=(5, 7))[1], cache.solve(name, pc, s, steps=(12,))[0]
    assert split["iters"] == min(12, first["iters"]) and same_state(split, whole)  # the position persists across calls
    mid = s // 2 + 1  # inside the first cycle for s >= 2, at its end for s = 1
    assert same_state(cache.solve(name, pc, s, reinit_after=mid)[0], first)  # init inside a cycle: a new handle
    after = cache.solve(name, pc, s, steps=(ITERS, 9, 1))
    assert after[0]["conv"] and same_state(after[0], after[1]) and same_state(after[0], after[2])  # nothing moves after the stop


def test_zero_right_hand_side(cache):
    e = cache.system("band600")
    d = cache.solve("band600", "none", 4, b=np.zeros(e["n"]), x0=np.zeros(e["n"]))[0]
    assert d["r0"] == 0.0 and d["iters"] == 1 and not d["conv"]
    assert d["hist"][0] == 0.0 and np.isnan(d["hist"][1])


@pytest.mark.parametrize("s", SS)
def test_identity_converges_at_iteration_one(ctx, s):
    n = 1001
    dA = ctx.matrix(CRS(n, np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), np.ones(n)))
    b, _ = right_hand_side(n)
    db, dx = ctx.upload(b), ctx.upload(np.zeros(n))
    h = ctx.idr(dA, db, dx, s)
    r0 = h.init(TOL)
    h.iterate(3)
    it, conv, hist = h.status()
    assert r0 > 0.0 and (it, conv) == (1, True) and hist[1] == 0.0
    assert same_bits(dx.to_host(), b)
    h.free(); db.free(); dx.free(); dA.free()


@pytest.mark.parametrize("s", SS)
def test_one_row(cache, s):
    e = cache.system("one")
    d = cache.solve("one", "none", s, b=np.array([5.0]), x0=np.array([0.0]))[0]
    print(f"n = 1, s = {s}: {d['iters']} iterations, x = {d['x'][0]!r}, history {d['hist']}")
    assert e["n"] == 1 and d["conv"] and d["iters"] <= 2
    assert abs(d["x"][0] - 2.0) <= 1e-14


def test_no_rows(ctx):
    dA = ctx.matrix(CRS(0, np.zeros(1, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0)))
    db, dx = ctx.alloc(2), ctx.alloc(2)
    h = ctx.idr(dA, db, dx, 4)
    h.set_preconditioner("j")
    assert h.init(TOL) == 0.0
    h.iterate(7)
    it, conv, hist = h.status()
    assert (it, conv) == (0, False)
    h.free()
    db.free(); dx.free(); dA.free()


def test_set_shadow(cache):
    from basic_iterative_solvers_amd import BisError
    ctx, name, s = cache.ctx, "band600", 4
    e = cache.system(name)
    # the hashed P passed explicitly: the default's bits
    assert same_state(cache.solve(name, "gs", s, P=hashed_shadow(e["n"], s))[0], cache.dev(name, "gs", s))
    # an orthonormal P: the restatement given that P
    Q, _ = np.linalg.qr(np.random.default_rng(3).standard_normal((e["n"], s)))
    d, g = cache.solve(name, "gs", s, P=Q)[0], cache.ref(name, "gs", s, P=Q, tag="orthonormal")
    check_parity(d, g, f"{name} gs s={s}, orthonormal P")
    assert not same_bits(d["hist"], cache.dev(name, "gs", s)["hist"])
    # after init it is refused
    db, dx = ctx.upload(e["b"]), ctx.upload(e["x0"])
    h = ctx.idr(e["dA"], db, dx, s)
    h.init(TOL)
    with pytest.raises(BisError, match="status 2"):
        h.set_shadow(Q)
    h.free(); db.free(); dx.free()


def test_error_table(cache):
    import ctypes as C

    from basic_iterative_solvers_amd import BisError
    ctx, e = cache.ctx, cache.system("unstr8")
    db, dx = ctx.upload(np.append(e["b"], [0.0, 0.0])), ctx.upload(np.append(e["x0"], [0.0, 0.0]))
    for s in (0, 9):
        with pytest.raises(BisError, match="status 2"):
            ctx.idr(e["dA"], db, dx, s)
    rect = ctx.matrix(CRS(2, np.array([0, 1, 2], dtype=np.int64), np.array([0, 2], np.int32), np.array([1.0, 1.0]), n_cols=3))
    h = C.c_void_p()
    assert ctx.lib.bis_idr_create(ctx.h, rect.h, C.c_void_p(db.ptr), C.c_void_p(dx.ptr), C.c_int(4), C.byref(h)) == 2 and not h
    rect.free()
    with pytest.raises(BisError, match="status 2"):  # b off a 16-byte boundary
        ctx.idr(e["dA"], db.offset(1), dx, 4)
    with pytest.raises(BisError, match="status 2"):
        ctx.idr(e["dA"], db, dx.offset(1), 4)
    h = ctx.idr(e["dA"], db, dx, 4)
    with pytest.raises(BisError, match="status 2"):  # iterate before init
        h.iterate(1)
    with pytest.raises(BisError, match="status 2"):  # a missing operand: refused here, not inside iterate
        h.set_preconditioner("gs", A_D=e["D"])
    with pytest.raises(BisError, match="status 2"):
        h.set_preconditioner("j")
    with pytest.raises(BisError, match="status 2"):  # type 12 is out of range
        h.set_preconditioner(12)
    other = ctx.gen_hpcg(8)
    mg_other = ctx.mg(other)
    with pytest.raises(BisError, match="status 2"):  # an MG operand of another size
        h.set_preconditioner("mg", Ls=mg_other.operand)
    with pytest.raises(BisError, match="status 6"):  # BIS_ERR_UNSUPPORTED, as bis_apply_preconditioner
        h.set_preconditioner("mg", Ls=cache.precond("unstr8", "mg")["Ls"], outer=2)
    h.set_preconditioner("gs", **cache.precond("unstr8", "gs"))
    h.init(TOL)
    with pytest.raises(BisError, match="status 2"):  # BIS_ERR_INVALID after bis_idr_init
        h.set_preconditioner("j", A_D=e["D"])
    h.iterate(ITERS)
    it, conv, hist = h.status()
    assert conv and same_bits(hist, cache.dev("unstr8", "gs", 4)["hist"])
    h.free(); mg_other.free(); other.free()
    db.free(); dx.free()
