"""GPU: bis_svds_* (Golub-Kahan-Lanczos bidiagonalisation with thick restart, a device schedule) against the numpy restatement
of include/bis_hip.h (tests/svds_ref.py) run on the device's own matrices, downloaded, and against numpy.linalg.svd of those
matrices.  All solves use tol 1e-10.

Inputs (svds_ref.TABLE, the issue's table with one basis size moved for the threshold margins that
tests/test_svds_ref_cpu.py asserts): tall, wide and square; odd and even lengths on either side (1301 / 700, 1025); less than
one workgroup of pairs (3 x 2, 7 x 40, 40 x 7) and more than two; more than 8, 16 and 32 basis blocks; ncv = 64 (every lane of
the restart wave); ncv = ns (the cycle ends on the invariant subspace).

Gate: the project's CG history gate, HIST_TOL["cg"] = 1e-10, on column 0 over the whole history, relative to entry 0 but
not less than 64 eps ||A||_1 (svds_ref.hist_scale); column 1 equal.  tests/test_svds_ref_cpu.py licenses it: the restatement
moves by at most 3.5e-13 between three orders of the sums.  Each test prints what it measured before it asserts."""
import numpy as np
import pytest

import svds_ref as S
from helpers import HIST_TOL
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

TOL = 1e-10
GATE = HIST_TOL["cg"]
ORTH = 1e-12
MAX_CYCLES = 400


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


def host_of(dA):
    return CRS(dA.n_rows, *dA.download(), n_cols=dA.n_cols)


def run_handle(ctx, dA, k, ncv, which, v0=None, At=None, max_cycles=MAX_CYCLES, keep=False):
    """One solve with the handle: status() with the vectors U, V; keep: the handle comes back too (the caller frees it)."""
    s = ctx.svds(dA, k=k, which=which, ncv=ncv, tol=TOL, v0=v0, At=At)
    out = s.solve(max_cycles=max_cycles, batch=4)
    out["U"], out["V"] = s.vectors() if out["restarts"] else (None, None)
    if keep:
        return out, s
    s.free()
    return out


class Cache:
    """Every system, reference and handle run once per module."""

    def __init__(self, ctx):
        self.ctx, self.sys, self.refs, self.runs = ctx, {}, {}, {}

    def system(self, name):
        kind, args = S.TABLE[name][:2]
        key = (kind, args)
        if key not in self.sys:
            dA = self.ctx.matrix(S.make_input(name))
            hA = host_of(dA)
            D = S.dense_of(hA)
            self.sys[key] = dict(dA=dA, hA=hA, hAt=S.transposed(hA), D=D, sv=np.linalg.svd(D, compute_uv=False), norm1=S.norm1_of(hA))
        return self.sys[key]

    def ref(self, name):
        if name not in self.refs:
            e = self.system(name)
            which, k, ncv = S.TABLE[name][2:5]
            self.refs[name] = S.svds(e["hA"], e["hAt"], k, ncv, which, TOL, max_cycles=MAX_CYCLES)
        return self.refs[name]

    def run(self, name):
        if name not in self.runs:
            which, k, ncv = S.TABLE[name][2:5]
            self.runs[name] = run_handle(self.ctx, self.system(name)["dA"], k, ncv, which)
        return self.runs[name]


@pytest.fixture(scope="module")
def cache(ctx):
    return Cache(ctx)


def check_triplets(tag, e, got, k, which):
    """The CPU test's bounds on the device's vectors and values."""
    smax = e["sv"][0]
    w = S.wanted(e["sv"], k, which)
    res = S.residuals(e["D"], got["values"], got["U"], got["V"])
    dval = np.max(np.abs(got["values"] - w))
    ou, ov = S.orth_defect(got["U"]), S.orth_defect(got["V"])
    print(f"{tag}: |sigma - numpy| / sigma_max {dval / smax:.2e}; max residual / sigma_max {np.max(res) / smax:.2e}; U, V orthonormal "
          f"to {ou:.2e}, {ov:.2e}")
    assert np.all(np.isfinite(got["U"])) and np.all(np.isfinite(got["V"]))
    assert dval <= 1e-12 * smax
    assert np.all(res <= 4 * TOL * smax)
    assert ou <= ORTH and ov <= ORTH


@pytest.mark.parametrize("name", S.ROWS)
def test_against_the_restatement(cache, name):
    e, got, want = cache.system(name), cache.run(name), cache.ref(name)
    which, k = S.TABLE[name][2:4]
    cnt = min(len(got["hist"]), len(want["hist"]))
    scale = S.hist_scale(want["hist"], e["norm1"])
    dev = np.max(np.abs(got["hist"][:cnt] - want["hist"][:cnt])) / scale if cnt else 0.0
    allowed = 2 * TOL * want["sigma_ref"]
    print(f"{name}: device products {got['products']} restarts {got['restarts']} reason {S.REASONS[got['reason']]} nconv "
          f"{got['nconv']}; restatement {want['products']} {want['restarts']} {S.REASONS[want['reason']]} {want['nconv']}; "
          f"max |d hist| / scale {dev:.2e}; max |d sigma| / allowed {np.max(np.abs(got['values'] - want['values'])) / allowed:.2e}; "
          f"sigma_ref {got['sigma_ref']:.16e} against {want['sigma_ref']:.16e}")
    for key in ("restarts", "products", "converged", "reason", "nconv"):
        assert got[key] == want[key], key
    assert dev <= GATE
    assert np.array_equal(got["hist_nconv"], want["hist_nconv"])
    assert np.all(np.abs(got["values"] - want["values"]) <= allowed)
    assert abs(got["sigma_ref"] - want["sigma_ref"]) <= allowed
    check_triplets(name, e, got, k, which)


def drive_by_hand(ctx, dA, dAt, k, ncv, which, cycles):
    """The same handle driven through op_begin / bis_spmv / op_end, with A or At as `transposed` says, polled once per cycle."""
    s = ctx.svds(dA, k=k, which=which, ncv=ncv, tol=TOL)
    s.init()
    l = S.keep_count(k, ncv)
    seen = set()
    for cycle in range(cycles):
        for _ in range(2 * (ncv if cycle == 0 else ncv - l)):
            inp, out, tr = s.op_begin()
            seen.add(tr)
            ctx.spmv(dAt if tr else dA, inp, out)
            s.op_end()
        st = s.status()
        if st["stopped"]:
            break
    assert seen == {False, True}
    st["U"], st["V"] = s.vectors()
    s.free()
    return st


def assert_same_run(tag, a, b):
    for key in ("products", "restarts", "stopped", "converged", "reason", "nconv"):
        assert a[key] == b[key], (tag, key)
    for key in ("values", "est", "hist", "U", "V", "sigma_ref"):
        assert same_bits(a[key], b[key]), (tag, key)
    assert np.array_equal(a["hist_nconv"], b["hist_nconv"]), tag


@pytest.mark.parametrize("name", ["T-LM", "W-LM", "B7x40-LM"])
def test_same_bits(ctx, cache, name):
    """Two runs, the loop of single products, launches after the stop, init again, At passed in, the caller's v0."""
    from idr_ref import hashed_shadow
    e, first = cache.system(name), cache.run(name)
    which, k, ncv = S.TABLE[name][2:5]
    dA = e["dA"]
    second, s = run_handle(ctx, dA, k, ncv, which, keep=True)
    assert_same_run("second run", first, second)
    dAt = dA.transpose()
    by_hand = drive_by_hand(ctx, dA, dAt, k, ncv, which, MAX_CYCLES)
    assert_same_run("op_begin / spmv / op_end", first, by_hand)
    s.iterate(2)
    after = s.status()
    after["U"], after["V"] = s.vectors()
    assert_same_run("launches after the stop", first, after)
    again = s.solve(max_cycles=MAX_CYCLES, batch=4)
    again["U"], again["V"] = s.vectors()
    assert_same_run("init again", first, again)
    s.free()
    assert_same_run("At passed in", first, run_handle(ctx, dA, k, ncv, which, At=dAt))
    v0 = ctx.upload(hashed_shadow(min(dA.n_rows, dA.n_cols), 1)[:, 0])
    assert_same_run("caller's v0", first, run_handle(ctx, dA, k, ncv, which, v0=v0))
    v0.free()
    dAt.free()
    print(f"{name}: six runs of {first['products']} products and {first['restarts']} restarts agree bit for bit")


@pytest.mark.parametrize("name", ["W-LM", "T-SM", "B7x40-LM"])
def test_wide_against_tall(ctx, cache, name):
    """svds(A) and svds(A^T): the same values bit for bit, U and V exchanged bit for bit."""
    e, first = cache.system(name), cache.run(name)
    which, k, ncv = S.TABLE[name][2:5]
    dAt = e["dA"].transpose()
    other = run_handle(ctx, dAt, k, ncv, which)
    print(f"{name}: {first['products']} products, {first['restarts']} restarts; transposed {other['products']}, {other['restarts']}")
    for key in ("products", "restarts", "converged", "reason", "nconv"):
        assert first[key] == other[key], key
    for key in ("values", "est", "hist", "sigma_ref"):
        assert same_bits(first[key], other[key]), key
    assert same_bits(first["U"], other["V"]) and same_bits(first["V"], other["U"])
    dAt.free()


D6 = np.array([3.0, 2.0, 5.0, 7.0, 11.0, 13.0])


@pytest.mark.parametrize("shape", [(8, 6), (6, 8)])
def test_breakdowns(ctx, shape):
    """Rectangular "diagonal" matrices with sparse start vectors: ordinary data on which the recurrences end exactly."""
    rows, cols = shape
    tall = rows >= cols
    v0 = ctx.upload(np.array([1.0, 1.0, 0.0, 0.0, 0.0, 0.0]))
    # v0 = e_0 + e_1: span(e_0, e_1) is invariant; a beta breakdown at m_eff = 2
    dD = ctx.matrix(S.diag_rect(rows, cols, D6))
    got = run_handle(ctx, dD, 2, None, "LM", v0=v0, max_cycles=4)
    print(f"{rows} x {cols} beta breakdown: products {got['products']} restarts {got['restarts']} reason {S.REASONS[got['reason']]} nconv "
          f"{got['nconv']} values {got['values']} est {got['est']} hist {got['hist']}")
    assert got["stopped"] and got["converged"] and got["reason"] == S.INVARIANT
    assert (got["products"], got["restarts"], got["nconv"]) == (4, 1, 2)
    assert np.max(np.abs(got["values"] - [3.0, 2.0])) <= 8 * S.EPS and np.all(got["est"] == 0.0)
    assert same_bits(got["hist"], [0.0]) and list(got["hist_nconv"]) == [2]
    U, V = got["U"], got["V"]
    assert np.all(np.isfinite(U)) and np.all(np.isfinite(V)) and np.all(U[2:] == 0.0) and np.all(V[2:] == 0.0)
    assert np.max(np.abs(np.abs(U[:2]) - np.eye(2))) <= 64 * S.EPS and np.max(np.abs(np.abs(V[:2]) - np.eye(2))) <= 64 * S.EPS
    # k > m_eff: not converged, nconv = m_eff
    got = run_handle(ctx, dD, 3, None, "LM", v0=v0, max_cycles=4)
    print(f"{rows} x {cols} k = 3 > m_eff: reason {S.REASONS[got['reason']]} nconv {got['nconv']} values {got['values']}")
    assert got["stopped"] and not got["converged"] and got["reason"] == S.INVARIANT
    assert (got["products"], got["restarts"], got["nconv"]) == (4, 1, 2)
    assert np.max(np.abs(got["values"][:2] - [3.0, 2.0])) <= 8 * S.EPS
    dD.free()
    # d_1 = 0 inside v0's support: F P_1 lies in span(Q_0); an alpha breakdown, a zero sigma whose long-side vector is zero
    d0 = D6.copy()
    d0[1] = 0.0
    dZ = ctx.matrix(S.diag_rect(rows, cols, d0))
    got = run_handle(ctx, dZ, 2, None, "LM", v0=v0, max_cycles=4)
    long_side, short_side = (got["U"], got["V"]) if tall else (got["V"], got["U"])
    print(f"{rows} x {cols} alpha breakdown: products {got['products']} restarts {got['restarts']} reason {S.REASONS[got['reason']]} nconv "
          f"{got['nconv']} values {got['values']} est {got['est']} long-side vector of the zero value {long_side[:, 1]}")
    assert got["stopped"] and got["converged"] and got["reason"] == S.INVARIANT
    assert (got["products"], got["restarts"], got["nconv"]) == (3, 1, 2)
    assert abs(got["values"][0] - 3.0) <= 8 * S.EPS and got["values"][1] == 0.0 and np.all(got["est"] == 0.0)
    assert np.all(np.isfinite(long_side)) and np.all(np.isfinite(short_side))
    assert np.all(long_side[:, 1] == 0.0)
    assert np.max(np.abs(np.abs(long_side[:, 0]) - np.eye(max(rows, cols))[:, 0])) <= 64 * S.EPS
    assert np.max(np.abs(np.abs(short_side) - np.eye(6)[:, :2])) <= 64 * S.EPS  # e_0, and the null vector e_1
    dZ.free()
    # a zero and a non-finite start vector
    dD = ctx.matrix(S.diag_rect(rows, cols, D6))
    for bad in (np.zeros(6), np.array([1.0, np.nan, 0.0, 0.0, 0.0, 0.0])):
        b = ctx.upload(bad)
        s = ctx.svds(dD, k=2, v0=b)
        st = s.solve(max_cycles=2)
        print(f"{rows} x {cols} v0 {bad[:2]}: reason {S.REASONS[st['reason']]} products {st['products']}")
        assert st["stopped"] and not st["converged"] and st["reason"] == S.BAD_START and st["products"] == 0 and st["restarts"] == 0
        s.free()
        b.free()
    dD.free()
    v0.free()


def test_cross_check_with_the_eigensolver(ctx):
    """A symmetric positive definite matrix: its singular values are its eigenvalues."""
    dA = ctx.gen_hpcg(5, 7, 37)
    got = run_handle(ctx, dA, 2, None, "LM")
    e = ctx.eigs(dA, k=2, which="LA", tol=TOL)
    eg = e.solve(max_cycles=MAX_CYCLES, batch=4)
    e.free()
    allowed = 2 * TOL * got["sigma_ref"]
    print(f"hpcg 5 x 7 x 37: sigma {got['values']} ({got['products']} products, {got['restarts']} restarts), lambda {eg['values']} "
          f"({eg['products']} products, {eg['restarts']} restarts); max difference / allowed "
          f"{np.max(np.abs(got['values'] - eg['values'])) / allowed:.2e}")
    assert got["converged"] and eg["converged"]
    assert np.all(np.abs(got["values"] - eg["values"]) <= allowed)
    dA.free()


def test_refusals(ctx, cache):
    import ctypes as C
    from basic_iterative_solvers_amd import BisError
    dA = cache.system("T-LM")["dA"]  # 1301 x 700

    def refused(what, fn):
        with pytest.raises(BisError) as err:
            fn()
        print(f"{what}: {err.value}")
        return str(err.value)

    assert "bis_svds_create: k must be at least 1" in refused("k < 1", lambda: ctx.svds(dA, k=0))
    assert "bis_svds_create: ncv must exceed k" in refused("ncv <= k", lambda: ctx.svds(dA, k=4, ncv=4))
    assert "bis_svds_create: ncv must not exceed min(rows, cols, 64)" in refused("ncv > 64", lambda: ctx.svds(dA, k=4, ncv=65))
    d76 = ctx.matrix(S.diag_rect(8, 6, D6))
    assert "bis_svds_create: ncv must not exceed min(rows, cols, 64)" in refused("ncv > ns", lambda: ctx.svds(d76, k=2, ncv=7))
    assert "bis_svds_create: At must be the transpose of A" in refused("At of the wrong shape", lambda: ctx.svds(dA, k=2, At=d76))
    assert "bis_svds_create: At must be the transpose of A" in refused("At = A", lambda: ctx.svds(d76, k=2, At=d76))
    d76.free()
    assert "bis_svds_create: min(rows, cols) must be at least 2" in refused("ns < 2", lambda: ctx.svds(None, k=1, shape=(5, 1)))
    assert "bis_svds_create: which" in refused("which", lambda: ctx.check(ctx.lib.bis_svds_create(
        ctx.h, dA.h, C.c_void_p(), C.c_int64(1301), C.c_int64(700), C.c_int(2), C.c_int(0), C.c_int(2), C.byref(C.c_void_p()))))
    with pytest.raises(BisError):
        ctx.svds(dA, k=2, which="LA")
    s = ctx.svds(None, k=2, shape=(125, 90))
    s.init()
    assert "bis_svds_iterate" in refused("iterate on a caller-applied handle", lambda: s.iterate(1))
    assert "bis_svds_op_end: call bis_svds_op_begin first" in refused("op_end without op_begin", s.op_end)
    inp, out, tr = s.op_begin()
    assert (inp.n, out.n, tr) == (90, 125, False)
    assert "bis_svds_op_begin: the product before it was not closed" in refused("two op_begin", s.op_begin)
    s.free()
    s = ctx.svds(dA, k=2)
    s.init()
    assert "bis_svds_vectors: no restart yet" in refused("vectors before a restart", s.vectors)
    assert "bis_svds_set_start: call it before bis_svds_init" in refused("set_start after init", lambda: s.set_start(None))
    s.free()
    null = C.c_void_p()
    assert "bis_svds_init: null handle" in refused("init", lambda: ctx.check(ctx.lib.bis_svds_init(ctx.h, null, C.c_double(TOL))))
    assert "bis_svds_set_start: null handle" in refused("set_start", lambda: ctx.check(ctx.lib.bis_svds_set_start(ctx.h, null, null)))
    assert "bis_svds_iterate" in refused("iterate", lambda: ctx.check(ctx.lib.bis_svds_iterate(ctx.h, null, C.c_int(1))))
    assert "bis_svds_op_end: null handle" in refused("op_end", lambda: ctx.check(ctx.lib.bis_svds_op_end(ctx.h, null)))
    assert "bis_svds_vectors: null handle" in refused("vectors", lambda: ctx.check(ctx.lib.bis_svds_vectors(
        ctx.h, null, null, C.c_int64(1), null, C.c_int64(1))))
    assert "bis_svds_status: null handle" in refused("status", lambda: ctx.check(ctx.lib.bis_svds_status(
        ctx.h, null, *([null] * 11), C.c_int(0))))
