"""GPU: bis_lsmr_* (LSMR for rectangular least-squares systems, a device schedule) against the numpy restatement of
include/bis_hip.h (tests/lsmr_ref.py) run on the device's own matrices, downloaded, and against a loop made of the
library's single-vector calls (spmv, compute_residual, dot, scale, subtract_vectors / sum_vectors, elemwise_mult_vectors)
with the scalar algebra in numpy (lsmr_ref.Scalars); the loop runs none of bis_lsmr_*.

Inputs (tests/lsmr_ref.py): T = banded(1301, 700, 5, 1), W = banded(700, 1301, 5, 2), S = banded(1025, 1025, 7, 3) with
damping 0 and 0.5, banded(515, 3, 2, 4), banded(3, 2, 2, 5), a 1 x 1 matrix; b uniform(-1, 1) from default_rng(3), x0 = 0,
tol 1e-10 for both tests.  The sizes are the edges of the passes: odd lengths (the single-lane tail), m != n, less than one
workgroup of pairs (3, 2, 1), more than two (1301, 1025).

Gate: the project's CG history gate, HIST_TOL["cg"] = 1e-10 of entry 0, on both history columns over the whole history;
`iters`, `converged` and `reason` equal; x at 1e-9 relative.  tests/test_lsmr_ref_cpu.py licenses it: the restatement moves
by at most 1.4e-16 of entry 0 between three orders of the sums.  Each test prints what it measured before it asserts."""
import ctypes as C

import numpy as np
import pytest

import lsmr_ref as L
from helpers import HIST_TOL
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

TOL = 1e-10
ITERS = 400
GATE = HIST_TOL["cg"]
X_GATE = 1e-9


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def relerr(x, want):
    nrm = np.linalg.norm(want)
    return np.linalg.norm(x - want) / (nrm if nrm else 1.0)


INPUTS = {"T": lambda: L.table_matrix("T"), "W": lambda: L.table_matrix("W"), "S": lambda: L.table_matrix("S"),
          "tall3": lambda: L.banded(515, 3, 2, 4), "tiny": lambda: L.banded(3, 2, 2, 5),
          "one": lambda: CRS(1, np.array([0, 1]), np.zeros(1, np.int32), np.array([2.5]), n_cols=1),
          "badT": L.badly_scaled_T}
# (input, damping): the issue's six rows and the three small inputs
ROWS = [(name, damp) for name in "TWS" for damp in L.DAMPS] + [("tall3", 0.0), ("tiny", 0.0), ("one", 0.0)]


class Cache:
    """Every system, reference and handle run once per module."""

    def __init__(self, ctx):
        self.ctx, self.sys, self.refs, self.runs = ctx, {}, {}, {}

    def system(self, name):
        if name not in self.sys:
            A = INPUTS[name]()
            dA = self.ctx.matrix(A)
            dAt = dA.transpose()
            b = L.rhs(A.n_rows)
            # what the device holds, downloaded: the reference's operands
            hA = CRS(dA.n_rows, *dA.download(), n_cols=dA.n_cols)
            hAt = CRS(dAt.n_rows, *dAt.download(), n_cols=dAt.n_cols)
            assert np.array_equal(hA.val, A.val) and np.array_equal(L.dense_of(hAt), L.dense_of(hA).T)
            self.sys[name] = dict(name=name, A=A, hA=hA, hAt=hAt, dA=dA, dAt=dAt, b=b, db=self.ctx.upload(b), m=A.n_rows, n=A.n_cols)
        return self.sys[name]

    def ref(self, name, damp, d=None, iters=ITERS):
        key = (name, damp, None if d is None else d.tobytes(), iters)
        if key not in self.refs:
            e = self.system(name)
            self.refs[key] = L.lsmr(e["hA"], e["hAt"], e["b"], damp=damp, d=d, tol_r=TOL, iters=iters)
        return self.refs[key]

    def run(self, name, damp):
        if (name, damp) not in self.runs:
            self.runs[(name, damp)] = run_handle(self.ctx, self.system(name), damp=damp)
        return self.runs[(name, damp)]


@pytest.fixture(scope="module")
def cache(ctx):
    return Cache(ctx)


def run_handle(ctx, e, damp=0.0, d=None, given_At=True, iters=ITERS, tol=TOL, x0=None, chunks=None):
    """One solve with the handle; d: None, "norm" or a numpy vector.  chunks: the iterate() calls to make instead of one."""
    dx = ctx.upload(np.zeros(e["n"]) if x0 is None else x0)
    dd = ctx.upload(d) if isinstance(d, np.ndarray) else d
    s = ctx.lsmr(e["dA"], e["db"], dx, At=e["dAt"] if given_At else None, damp=damp, col_scaling=dd)
    r0, ar0 = s.init(tol)
    for k in (chunks or [iters]):
        s.iterate(k)
    out = s.status()
    out.update(x=dx.to_host(), r0=r0, ar0=ar0)
    s.free()
    dx.free()
    if isinstance(d, np.ndarray):
        dd.free()
    return out


def run_loop(ctx, e, damp=0.0, d=None, iters=ITERS, tol=TOL):
    """The same iteration made of the library's single-vector calls; the scalars stay in numpy."""
    m, n, dA, dAt = e["m"], e["n"], e["dA"], e["dAt"]
    x, u, tm = ctx.upload(np.zeros(n)), ctx.alloc(m), ctx.alloc(m)
    v, h, hbar, tn, w = ctx.alloc(n), ctx.alloc(n), ctx.upload(np.zeros(n)), ctx.alloc(n), ctx.alloc(n)
    dd = ctx.upload(d) if d is not None else None
    ctx.compute_residual(dA, x, e["db"], u, tm)
    beta = np.sqrt(np.float64(ctx.dot(u, u, m)))
    ctx.spmv(dAt, u, tn)
    ctx.scale(tn, tn, float(L.div0(1.0, beta)), n)
    if dd is not None:
        ctx.elemwise_mult_vectors(tn, tn, dd, n=n)
    alpha = np.sqrt(np.float64(ctx.dot(tn, tn, n)))
    S = L.Scalars(beta, alpha, damp, tol)
    ctx.scale(v, tn, float(S.ia), n)
    ctx.copy_vector(h, v, n)
    while S.reason == 0 and S.iters < iters:
        if dd is not None:
            ctx.elemwise_mult_vectors(w, v, dd, n=n)
        ctx.spmv(dA, w if dd is not None else v, tm)
        ctx.subtract_vectors(u, tm, u, float(S.cu), m)                   # pass U
        S.set_beta(np.sqrt(np.float64(ctx.dot(u, u, m))))
        ctx.spmv(dAt, u, tn)
        ctx.scale(tn, tn, float(S.ib), n)                               # pass V
        if dd is not None:
            ctx.elemwise_mult_vectors(tn, tn, dd, n=n)
        ctx.subtract_vectors(tn, tn, v, float(S.beta), n)
        c_hbar, c_x, c_h = S.step(np.sqrt(np.float64(ctx.dot(tn, tn, n))))
        ctx.scale(v, tn, float(S.ia), n)                                # pass H
        ctx.subtract_vectors(hbar, h, hbar, float(c_hbar), n)
        if dd is not None:
            ctx.elemwise_mult_vectors(w, dd, hbar, n=n)
        ctx.sum_vectors(x, x, w if dd is not None else hbar, float(c_x), n)
        ctx.subtract_vectors(h, v, h, float(c_h), n)
    out = S.result(x.to_host())
    for vec in (x, u, tm, v, h, hbar, tn, w) + ((dd,) if dd is not None else ()):
        vec.free()
    return out


def compare(tag, got, want, gate=GATE, x_gate=X_GATE):
    """Prints the deviations, then asserts the gate."""
    k = min(len(got["hist"]), len(want["hist"]))
    dev = max(np.max(np.abs(got[c][:k] - want[c][:k])) / want[c][0] if want[c][0] else np.max(np.abs(got[c][:k])) for c in ("hist", "hist_r"))
    xerr = relerr(got["x"], want["x"])
    print(f"{tag}: {got['iters']} / {want['iters']} iterations, reason {L.REASONS[got['reason']]} / {L.REASONS[want['reason']]}, "
          f"histories deviate by {dev:.2e} of entry 0, x by {xerr:.2e}; bits equal: hist {same_bits(got['hist'], want['hist'])}, "
          f"x {same_bits(got['x'], want['x'])}")
    assert (got["iters"], got["converged"], got["reason"]) == (want["iters"], want["converged"], want["reason"])
    assert len(got["hist"]) == len(got["hist_r"]) == got["iters"] + 1
    assert dev <= gate
    assert xerr <= x_gate


# ---- (a) the history gate ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,damp", ROWS)
def test_history_gate_against_the_restatement(cache, name, damp):
    got, want = cache.run(name, damp), cache.ref(name, damp)
    compare(f"{name} damp {damp} vs numpy", got, want)
    assert got["converged"] and got["r0"] == got["hist_r"][0] and got["ar0"] == got["hist"][0]
    assert np.all(np.diff(got["hist"]) <= 0), "the ar history never increases"
    if name in L.TABLE:
        assert got["iters"] == L.TABLE[name][5][L.DAMPS.index(damp)]


@pytest.mark.parametrize("name,damp", ROWS)
def test_history_gate_against_the_library_loop(ctx, cache, name, damp):
    compare(f"{name} damp {damp} vs library loop", cache.run(name, damp), run_loop(ctx, cache.system(name), damp=damp))


def test_scaled_and_damped_against_both(ctx, cache):
    """The scaled kernels with a caller's d (not the norms), with damping: damping acts on y = x / d."""
    e = cache.system("T")
    d = np.random.default_rng(5).uniform(0.5, 2.0, e["n"])
    got = run_handle(ctx, e, damp=0.5, d=d)
    compare("T damp 0.5 d uniform(0.5, 2) vs numpy", got, cache.ref("T", 0.5, d))
    compare("T damp 0.5 d uniform(0.5, 2) vs library loop", got, run_loop(ctx, e, damp=0.5, d=d))
    # the problem it solves: min |A D y - b|^2 + damp^2 |y|^2, x = D y
    y = L.lstsq_damped(L.scale_columns(e["A"], d), e["b"], 0.5)
    print(f"  against lstsq on [A D; damp I]: {relerr(got['x'], d * y):.2e}")
    assert relerr(got["x"], d * y) <= 1e-8


# ---- (b) both ways of getting At ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,damp", [("T", 0.0), ("W", 0.5)])
def test_At_given_and_At_made_by_the_handle_agree_bit_for_bit(ctx, cache, name, damp):
    a, b = cache.run(name, damp), run_handle(ctx, cache.system(name), damp=damp, given_At=False)
    assert a["iters"] == b["iters"] and a["reason"] == b["reason"]
    assert same_bits(a["x"], b["x"]) and same_bits(a["hist"], b["hist"]) and same_bits(a["hist_r"], b["hist_r"])


# ---- (c) column scaling ------------------------------------------------------------------------------------------------
def test_column_scaling_by_the_norms(ctx, cache):
    e = cache.system("badT")
    want = cache.ref("badT", 0.0, 1.0 / L.col_norms(e["hA"]))
    for given in (True, False):
        got = run_handle(ctx, e, d="norm", given_At=given)
        err = relerr(got["x"], L.lstsq_damped(e["A"], e["b"]))
        print(f"badly scaled T, col_scaling='norm', At {'given' if given else 'made'}: {got['iters']} iterations (restatement "
              f"{want['iters']}), |x - lstsq| / |lstsq| = {err:.2e}")
        assert got["converged"] and abs(got["iters"] - want["iters"]) <= 2
        assert err <= 1e-7
    plain = cache.run("badT", 0.0)
    print(f"  without scaling: ar = {plain['hist'][-1] / plain['hist'][0]:.2e} ar0 after {plain['iters']} iterations")
    assert not plain["converged"] and plain["iters"] == ITERS and plain["reason"] == 0


def test_row_norms(ctx, cache):
    # sums of squares that are exact in any order: small integers; an empty row; more rows than one workgroup
    rng = np.random.default_rng(7)
    m, n = 777, 40
    rows = np.repeat(np.arange(m), 6)
    rows = rows[rows % 50 != 3]  # rows 3, 53, ... are empty
    A = L.from_triplets(m, n, rows, rng.integers(0, n, len(rows)), rng.integers(-9, 10, len(rows)).astype(np.float64))
    dA = ctx.matrix(A)
    got = dA.row_norms()
    sq = np.zeros(m)
    np.add.at(sq, np.repeat(np.arange(m), np.diff(A.row_ptr)), A.val * A.val)
    assert got.n == m and same_bits(got.to_host(), np.sqrt(sq)) and got.to_host()[3] == 0.0
    got.free()
    dA.free()
    e = cache.system("T")
    for dM, hM in ((e["dA"], e["hA"]), (e["dAt"], e["hAt"])):
        nrm = dM.row_norms()
        want = np.sqrt(np.array([np.sum(hM.val[a:b].astype(np.longdouble) ** 2) for a, b in zip(hM.row_ptr[:-1], hM.row_ptr[1:])]).astype(np.float64))
        dev = np.max(np.abs(nrm.to_host() - want) / want)
        print(f"row norms of a {hM.n_rows} x {hM.n_cols} matrix: {dev:.2e} relative")
        assert dev <= 1e-15
        nrm.free()
    # the scaling made of them: 1 where a norm is 0
    nz = ctx.upload(np.array([4.0, 0.0, 0.5, 0.0, 3.0]))
    ctx.check(ctx.lib.bis_lsmr_scaling_from_norms(ctx.h, C.c_void_p(nz.ptr), C.c_int64(5), C.c_void_p(nz.ptr)))
    assert same_bits(nz.to_host(), [0.25, 1.0, 2.0, 1.0, 1.0 / 3.0])
    nz.free()


# ---- (d) damping and refusals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["W", "S"])
def test_damped_solution_against_lstsq(cache, name):
    e, got = cache.system(name), cache.run(name, 0.5)
    err = relerr(got["x"], L.lstsq_damped(e["A"], e["b"], 0.5))
    print(f"{name} damp 0.5: |x - lstsq([A; 0.5 I])| / |.| = {err:.2e}")
    assert got["converged"] and err <= 1e-8


def test_refusals(ctx, cache):
    from basic_iterative_solvers_amd import BisError
    e = cache.system("T")
    dx, dd = ctx.upload(np.zeros(e["n"])), ctx.upload(np.ones(e["n"]))
    lib = ctx.lib
    s = ctx.lsmr(e["dA"], e["db"], dx, At=e["dAt"])
    assert lib.bis_lsmr_iterate(ctx.h, s.h, C.c_int(1)) == 2 and b"bis_lsmr_iterate" in lib.bis_last_error(ctx.h)
    for bad in (-0.5, float("nan"), float("inf")):
        assert lib.bis_lsmr_set_damping(ctx.h, s.h, C.c_double(bad)) == 2 and b"bis_lsmr_set_damping" in lib.bis_last_error(ctx.h)
    assert lib.bis_lsmr_set_col_scaling(ctx.h, s.h, C.c_void_p(dd.ptr + 8)) == 2  # off a 16-byte boundary
    with pytest.raises(BisError):
        s.set_col_scaling(ctx.upload(np.ones(e["n"] + 1)))
    s.set_col_scaling(dd)
    s.set_col_scaling(None)
    s.init(TOL)
    assert lib.bis_lsmr_set_damping(ctx.h, s.h, C.c_double(0.5)) == 2 and b"bis_lsmr_set_damping" in lib.bis_last_error(ctx.h)
    assert lib.bis_lsmr_set_col_scaling(ctx.h, s.h, C.c_void_p(dd.ptr)) == 2 and b"bis_lsmr_set_col_scaling" in lib.bis_last_error(ctx.h)
    s.free()
    h = C.c_void_p()
    for At in (e["dA"], cache.system("W")["dAt"]):  # m x n, and n x m of another matrix
        assert lib.bis_lsmr_create(ctx.h, e["dA"].h, At.h, C.c_void_p(e["db"].ptr), C.c_void_p(dx.ptr), C.byref(h)) == 2 and not h
        assert b"bis_lsmr_create" in lib.bis_last_error(ctx.h)
    big = ctx.alloc(e["m"] + 2)
    for pb, px in ((big.offset(1), dx), (e["db"], big.offset(1))):
        assert lib.bis_lsmr_create(ctx.h, e["dA"].h, e["dAt"].h, C.c_void_p(pb.ptr), C.c_void_p(px.ptr), C.byref(h)) == 2 and not h
    assert lib.bis_lsmr_create(ctx.h, None, None, C.c_void_p(e["db"].ptr), C.c_void_p(dx.ptr), C.byref(h)) == 2 and not h
    for call in (lambda: lib.bis_lsmr_init(ctx.h, None, C.c_double(TOL), C.c_double(TOL), None, None),
                 lambda: lib.bis_lsmr_iterate(ctx.h, None, C.c_int(1)),
                 lambda: lib.bis_lsmr_status(ctx.h, None, None, None, None, None, None, C.c_int(0)),
                 lambda: lib.bis_lsmr_set_damping(ctx.h, None, C.c_double(0.0)),
                 lambda: lib.bis_lsmr_set_col_scaling(ctx.h, None, None)):
        assert call() == 2
    with pytest.raises(BisError):
        ctx.lsmr(e["dA"], e["db"], dx, col_scaling="columns")
    for v in (dx, dd, big):
        v.free()


# ---- (e) breakdowns and edges ------------------------------------------------------------------------------------------
def solve_small(ctx, A, b, x0=None, tol=TOL, iters=10):
    dA = ctx.matrix(A)
    e = dict(dA=dA, dAt=None, db=ctx.upload(b), m=A.n_rows, n=A.n_cols)
    out = run_handle(ctx, e, given_At=False, x0=x0, tol=tol, iters=iters)
    e["db"].free()
    dA.free()
    return out


def test_breakdown_and_optimal_start(ctx):
    # three columns of one entry each (orthogonal, norm 2), b along one of them: every value of the first iteration is a
    # power of two, so u~ = A v - (alpha / beta) u~ is 0 exactly: beta = 0
    A = L.from_triplets(5, 3, [0, 2, 4], [0, 1, 2], [2.0, 2.0, 2.0])
    got = solve_small(ctx, A, np.array([2.0, 0, 0, 0, 0]), tol=0.0)
    print(f"b along a column: {got['iters']} iteration(s), reason {L.REASONS[got['reason']]}, hist {got['hist']}, x {got['x']}")
    assert (got["iters"], got["converged"], got["reason"]) == (1, True, 3)
    assert got["hist"][1] == 0.0 and np.array_equal(got["x"], [1.0, 0.0, 0.0])
    # b anywhere in the range: converged by the second iteration at the latest, x = the coefficients
    got = solve_small(ctx, A, np.array([2.0, 0, -6.0, 0, 3.0]))
    print(f"b in the range: {got['iters']} iteration(s), reason {L.REASONS[got['reason']]}, x {got['x']}")
    assert got["converged"] and got["iters"] <= 2 and relerr(got["x"], np.array([1.0, -3.0, 1.5])) <= 1e-14
    # x0 already optimal, with a residual that is not zero (rows 1 and 3 are outside the range): At r = 0 exactly
    x0 = np.array([1.0, 2.0, 3.0])
    got = solve_small(ctx, A, np.array([2.0, 1, 4, 1, 6]), x0=x0)
    assert (got["iters"], got["converged"], got["reason"]) == (0, True, 3)
    assert got["ar0"] == 0.0 and got["r0"] == np.sqrt(2.0) and same_bits(got["x"], x0) and len(got["hist"]) == 1
    # b = 0 with x0 = 0
    got = solve_small(ctx, A, np.zeros(5))
    assert (got["iters"], got["converged"], got["reason"], got["r0"], got["ar0"]) == (0, True, 3, 0.0, 0.0)
    assert same_bits(got["x"], np.zeros(3))


def test_no_rows_and_no_columns(ctx):
    for m, n in ((0, 3), (3, 0), (0, 0)):
        dA = ctx.matrix(CRS(m, np.zeros(m + 1, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0), n_cols=n))
        db, dx = ctx.alloc(4), ctx.upload(np.full(4, 0.25))
        s = ctx.lsmr(dA, db, dx)
        s.set_damping(0.5)
        assert s.init(TOL) == (0.0, 0.0)
        s.iterate(7)
        st = s.status()
        assert (st["iters"], st["converged"], st["reason"]) == (0, False, 0)
        assert np.array_equal(dx.to_host(), np.full(4, 0.25))
        s.free()
        nrm = dA.row_norms()
        assert nrm.n == m and np.array_equal(nrm.to_host(), np.zeros(m))
        for o in (nrm, db, dx, dA):
            o.free()


def test_launches_after_the_stop_change_nothing(ctx, cache):
    e = cache.system("W")
    dx = ctx.upload(np.zeros(e["n"]))
    s = ctx.lsmr(e["dA"], e["db"], dx, At=e["dAt"])
    s.init(TOL)
    s.iterate(40)
    a, xa = s.status(), dx.to_host()
    assert a["converged"] and a["iters"] < 40
    s.iterate(25)
    b, xb = s.status(), dx.to_host()
    assert (a["iters"], a["reason"]) == (b["iters"], b["reason"])
    assert same_bits(xa, xb) and same_bits(a["hist"], b["hist"]) and same_bits(a["hist_r"], b["hist_r"])
    want = cache.run("W", 0.0)
    assert same_bits(xa, want["x"]) and same_bits(a["hist"], want["hist"])
    s.free()
    dx.free()


# ---- (f) reuse ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,damp,d", [("T", 0.5, None), ("S", 0.0, "norm")])
def test_init_again_gives_the_bits_of_a_new_handle(ctx, cache, name, damp, d):
    e = cache.system(name)
    fresh = run_handle(ctx, e, damp=damp, d=d)
    again = run_handle(ctx, e, damp=damp, d=d, chunks=[3, 7, ITERS])
    assert fresh["converged"]
    for k in ("x", "hist", "hist_r"):
        assert same_bits(fresh[k], again[k]), f"two runs differ in {k}"
    dx = ctx.upload(np.zeros(e["n"]))
    s = ctx.lsmr(e["dA"], e["db"], dx, At=e["dAt"], damp=damp, col_scaling=d)
    for before in (5, ITERS):  # inside a solve, after a stop
        s.init(TOL)
        s.iterate(before)
        st = s.status()
        assert st["iters"] == min(before, fresh["iters"])
        dx.set(np.zeros(e["n"]))
        assert s.init(TOL) == (fresh["r0"], fresh["ar0"])
        assert s.status()["iters"] == 0 and len(s.status()["hist"]) == 1
        s.iterate(ITERS)
        st = s.status()
        assert (st["iters"], st["converged"], st["reason"]) == (fresh["iters"], fresh["converged"], fresh["reason"])
        assert same_bits(dx.to_host(), fresh["x"]) and same_bits(st["hist"], fresh["hist"]) and same_bits(st["hist_r"], fresh["hist_r"])
        dx.set(np.zeros(e["n"]))
    s.free()
    dx.free()


# ---- (g) the grid-stride case ------------------------------------------------------------------------------------------
def test_grid_stride_second_trip(ctx):
    """n = 2 * 8192 * 256 + 1537 columns: 8195 workgroups of pairs, just past the 8192 the reductions' grids are capped at
    (kMaxDotBlocks), so the loops of passes U and V take a second trip; m = n + 2 rows of two entries each."""
    n = 2 * 8192 * 256 + 1537
    m = n + 2
    i = np.arange(m, dtype=np.int64)
    hi = np.minimum(i, n - 1)
    hi[0] = 1
    lo = hi - 1
    col = np.stack([lo, hi], axis=1).ravel().astype(np.int32)
    val = np.stack([-1.0 + (i * 5 % 11) / 11.0, 2.0 + (i * 7 % 13) / 13.0], axis=1).ravel()
    A = CRS(m, 2 * np.arange(m + 1, dtype=np.int64), col, val, n_cols=n)
    dA = ctx.matrix(A)
    dAt = dA.transpose()
    hAt = CRS(n, *dAt.download(), n_cols=m)
    b = L.rhs(m)
    e = dict(dA=dA, dAt=dAt, db=ctx.upload(b), m=m, n=n)
    got = run_handle(ctx, e, damp=0.5, iters=3)
    want = L.lsmr(A, hAt, b, damp=0.5, tol_r=TOL, iters=3)
    compare(f"{m} x {n}, 3 iterations vs numpy", got, want)
    assert got["iters"] == 3 and got["reason"] == 0
    for o in (e["db"], dAt, dA):
        o.free()
