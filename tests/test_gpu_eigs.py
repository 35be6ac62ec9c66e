"""GPU: bis_eigs_* (thick-restart Lanczos with full re-orthogonalisation, a device schedule) against the numpy restatement
of include/bis_hip.h (tests/eigs_ref.py) run on the device's own matrices, downloaded, and against numpy.linalg.eigvalsh of
those matrices.  All solves use tol 1e-10.

Inputs (eigs_ref.INPUTS, the issue's table with the seeds and two basis sizes chosen for the threshold margins that
tests/test_eigs_ref_cpu.py asserts): the edges of the passes -- odd n (the single-lane tail), less than one workgroup of pairs
(3, 7, 125), more than two (1295, 1301, 1331), ncv = 64 (every lane of the Ritz wave), ncv = n (the cycle ends on the invariant
subspace).  ncv = k + 1 (l = m - 1: one product per cycle) converges by a few percent per restart, so no seed gives it the
margins; it has a test of its own below that demands the restatement's values, not its restart count.

Gate: the project's CG history gate, HIST_TOL["cg"] = 1e-10, on column 0 over the whole history, relative to entry 0 but
not less than 64 eps ||A||_1 (eigs_ref.hist_scale: with ncv = n, and at a breakdown, entry 0 is 0); column 1 equal.
tests/test_eigs_ref_cpu.py licenses it: the restatement moves by at most 1.7e-14 between three orders of the sums.
Each test prints what it measured before it asserts."""
import numpy as np
import pytest

import eigs_ref as E
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


class DeviceGen:
    """eigs_ref.make_input's generator: the device's matrices."""

    def __init__(self, ctx):
        self.ctx = ctx

    def gen_anderson(self, L, seed=1, shift=0.0):
        return self.ctx.gen_anderson(L, seed=seed, shift=shift)

    def gen_hpcg(self, nx, ny, nz):
        return self.ctx.gen_hpcg(nx, ny, nz)


def host_of(dA):
    return CRS(dA.n_rows, *dA.download(), n_cols=dA.n_cols)


def run_handle(ctx, dA, k, ncv, which, v0=None, max_cycles=MAX_CYCLES, keep=False):
    """One solve with the handle: status() with the vectors X; keep: the handle comes back too (the caller frees it)."""
    s = ctx.eigs(dA, k=k, which=which, ncv=ncv, tol=TOL, v0=v0)
    out = s.solve(max_cycles=max_cycles, batch=4)
    out["X"] = s.vectors() if out["restarts"] else None
    if keep:
        return out, s
    s.free()
    return out


class Cache:
    """Every system, reference and handle run once per module."""

    def __init__(self, ctx):
        self.ctx, self.sys, self.refs, self.runs = ctx, {}, {}, {}

    def system(self, name):
        if name not in self.sys:
            A = E.make_input(name, DeviceGen(self.ctx))
            dA = A if hasattr(A, "download") else self.ctx.matrix(A)
            hA = host_of(dA)
            D = E.dense_of(hA)
            assert np.array_equal(D, D.T)
            self.sys[name] = dict(dA=dA, hA=hA, D=D, lam=np.linalg.eigvalsh(D), norm1=E.norm1_of(hA), n=hA.n_rows)
        return self.sys[name]

    def ref(self, name, which):
        if (name, which) not in self.refs:
            e = self.system(name)
            k, ncv = E.INPUTS[name][2:4]
            self.refs[(name, which)] = E.eigs(lambda v: E.host_spmv(e["hA"], v), e["n"], k, ncv, which, TOL, max_cycles=MAX_CYCLES)
        return self.refs[(name, which)]

    def run(self, name, which):
        if (name, which) not in self.runs:
            k, ncv = E.INPUTS[name][2:4]
            self.runs[(name, which)] = run_handle(self.ctx, self.system(name)["dA"], k, ncv, which)
        return self.runs[(name, which)]


@pytest.fixture(scope="module")
def cache(ctx):
    return Cache(ctx)


def check_pairs(tag, e, got, k, which):
    """The CPU test's bound on the device's vectors, the wanted values, and the orthonormality of X."""
    X, values = got["X"][:, :k], got["values"][:k]
    dist, bound, lam = E.eigen_bound(e["D"], values, X)
    w, _ = E.wanted(lam, k, which)
    orth = np.max(np.abs(X.T @ X - np.eye(k)))
    print(f"{tag}: max |theta - lambda| {np.max(dist):.2e} (bound {np.max(bound):.2e}), max |theta - wanted| "
          f"{np.max(np.abs(values - w)):.2e}, ||X^T X - I||_max {orth:.2e}")
    assert np.all(np.isfinite(X)) and np.all(dist <= bound)
    for th, wi in zip(values, w):
        assert abs(th - wi) < 0.5 * np.min(np.abs(lam[lam != wi] - wi))
    assert orth <= ORTH


@pytest.mark.parametrize("name,which", E.ROWS)
def test_against_the_restatement(cache, name, which):
    e, got, want = cache.system(name), cache.run(name, which), cache.ref(name, which)
    k = E.INPUTS[name][2]
    cnt = min(len(got["hist"]), len(want["hist"]))
    scale = E.hist_scale(want["hist"], e["norm1"])
    dev = np.max(np.abs(got["hist"][:cnt] - want["hist"][:cnt])) / scale if cnt else 0.0
    thr = 2 * TOL * np.maximum(np.abs(want["values"]), E.EPS23)
    print(f"{name} {which}: device products {got['products']} restarts {got['restarts']} reason {E.REASONS[got['reason']]} nconv "
          f"{got['nconv']}; restatement {want['products']} {want['restarts']} {E.REASONS[want['reason']]} {want['nconv']}; "
          f"max |d hist| / scale {dev:.2e}; max |d theta| / allowed {np.max(np.abs(got['values'] - want['values']) / thr):.2e}")
    for key in ("restarts", "products", "converged", "reason", "nconv"):
        assert got[key] == want[key], key
    assert dev <= GATE
    assert np.array_equal(got["hist_nconv"], want["hist_nconv"])
    assert np.all(np.abs(got["values"] - want["values"]) <= thr)
    check_pairs(f"{name} {which}", e, got, k, which)


def test_one_product_per_cycle(ctx):
    """ncv = k + 1, l = m - 1: hundreds of restarts of one product each (eigs_ref.EXTRA_KP1).  The estimates fall by a few
    percent per restart, so the restart at which the test fires is not a fair demand; the values, the bound and the history
    over the common part are."""
    x = E.EXTRA_KP1
    A = E.sym_banded(x["n"], x["half"], x["seed"])
    dA = ctx.matrix(A)
    hA = host_of(dA)
    e = dict(D=E.dense_of(hA))
    got = run_handle(ctx, dA, x["k"], x["ncv"], x["which"], max_cycles=2000)
    want = E.eigs(lambda v: E.host_spmv(hA, v), x["n"], x["k"], x["ncv"], x["which"], TOL, max_cycles=2000)
    cnt = min(len(got["hist"]), len(want["hist"]))
    dev = np.max(np.abs(got["hist"][:cnt] - want["hist"][:cnt])) / E.hist_scale(want["hist"], E.norm1_of(hA))
    thr = 2 * TOL * np.maximum(np.abs(want["values"]), E.EPS23)
    print(f"ncv = k + 1: device restarts {got['restarts']} products {got['products']}, restatement {want['restarts']} "
          f"{want['products']}; max |d hist| / entry 0 over {cnt} entries {dev:.2e}; max |d theta| / allowed "
          f"{np.max(np.abs(got['values'] - want['values']) / thr):.2e}")
    assert got["converged"] and want["converged"] and got["reason"] == E.CONVERGED and got["nconv"] == x["k"]
    assert got["products"] == x["ncv"] + got["restarts"] - 1
    assert dev <= GATE
    assert np.all(np.abs(got["values"] - want["values"]) <= thr)
    check_pairs("ncv = k + 1", e, got, x["k"], x["which"])
    dA.free()


def drive_by_hand(ctx, dA, k, ncv, which, cycles):
    """The same handle driven through op_begin / bis_spmv / op_end, polled once per cycle."""
    s = ctx.eigs(dA, k=k, which=which, ncv=ncv, tol=TOL)
    s.init()
    l = E.keep_count(k, ncv)
    for cycle in range(cycles):
        for _ in range(ncv if cycle == 0 else ncv - l):
            inp, out = s.op_begin()
            ctx.spmv(dA, inp, out)
            s.op_end()
        st = s.status()
        if st["stopped"]:
            break
    st["X"] = s.vectors()
    s.free()
    return st


def assert_same_run(tag, a, b):
    for key in ("products", "restarts", "stopped", "converged", "reason", "nconv"):
        assert a[key] == b[key], (tag, key)
    for key in ("values", "est", "hist", "X"):
        assert same_bits(a[key], b[key]), (tag, key)
    assert np.array_equal(a["hist_nconv"], b["hist_nconv"]), tag


@pytest.mark.parametrize("name,which", [("anderson8", "LM"), ("band1301", "LM"), ("band7", "LM")])
def test_two_runs_the_loop_of_single_products_and_init_again_give_the_same_bits(ctx, cache, name, which):
    e, first = cache.system(name), cache.run(name, which)
    k, ncv = E.INPUTS[name][2:4]
    second, s = run_handle(ctx, e["dA"], k, ncv, which, keep=True)
    assert_same_run("second run", first, second)
    by_hand = drive_by_hand(ctx, e["dA"], k, ncv, which, MAX_CYCLES)
    assert_same_run("op_begin / spmv / op_end", first, by_hand)
    # init after a finished solve starts over; launches after the stop change nothing
    s.iterate(2)
    after = s.status()
    after["X"] = s.vectors()
    assert_same_run("launches after the stop", first, after)
    again = s.solve(max_cycles=MAX_CYCLES, batch=4)
    again["X"] = s.vectors()
    assert_same_run("init again", first, again)
    s.free()
    print(f"{name} {which}: four runs of {first['products']} products and {first['restarts']} restarts agree bit for bit")


def test_the_default_start_vector_given_by_the_caller(ctx, cache):
    from idr_ref import hashed_shadow
    name, which = "anderson5", "SA"
    e, first = cache.system(name), cache.run(name, which)
    k, ncv = E.INPUTS[name][2:4]
    v0 = ctx.upload(hashed_shadow(e["n"], 1)[:, 0])
    got = run_handle(ctx, e["dA"], k, ncv, which, v0=v0)
    assert_same_run("caller's v0", first, got)
    v0.free()


def diag_matrix(ctx, d):
    n = len(d)
    return ctx.matrix(CRS(n, np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), np.asarray(d, dtype=np.float64)))


def test_breakdowns(ctx):
    """None may produce a NaN or a hang."""
    # the identity: the first product stays in span(v0)
    dI = diag_matrix(ctx, np.ones(5))
    for v0_host in (np.array([1.0, 1.0, 1.0, 1.0, 0.0]), None):
        v0 = ctx.upload(v0_host) if v0_host is not None else None
        got = run_handle(ctx, dI, 2, None, "SA", v0=v0, max_cycles=4)
        print(f"identity, v0 {'given' if v0 else 'default'}: products {got['products']} restarts {got['restarts']} reason "
              f"{E.REASONS[got['reason']]} nconv {got['nconv']} values {got['values']} est {got['est']}")
        assert got["stopped"] and not got["converged"] and got["reason"] == E.INVARIANT
        assert (got["products"], got["restarts"], got["nconv"]) == (1, 1, 1)
        assert got["values"][0] == 1.0 and np.all(got["est"] == 0.0) and np.all(np.isfinite(got["X"]))
        assert same_bits(got["hist"], [0.0]) and list(got["hist_nconv"]) == [1]
        if v0:
            v0.free()
    dI.free()
    # diag(1..6) from e_1 + e_2: an invariant subspace of dimension k
    dD = diag_matrix(ctx, np.arange(1.0, 7.0))
    v0 = ctx.upload(np.array([1.0, 1.0, 0.0, 0.0, 0.0, 0.0]))
    for which, want in (("SA", [1.0, 2.0]), ("LA", [2.0, 1.0])):
        got = run_handle(ctx, dD, 2, None, which, v0=v0, max_cycles=4)
        print(f"diag(1..6) {which}: products {got['products']} reason {E.REASONS[got['reason']]} values {got['values']} est {got['est']}")
        assert got["stopped"] and got["converged"] and got["reason"] == E.INVARIANT
        assert (got["products"], got["restarts"], got["nconv"]) == (2, 1, 2)
        assert np.max(np.abs(got["values"] - want)) <= 8 * E.EPS and np.all(got["est"] == 0.0)
        X = got["X"]
        assert np.all(np.isfinite(X)) and np.all(X[2:] == 0.0) and np.max(np.abs(X.T @ X - np.eye(2))) <= ORTH
        assert np.max(np.abs(np.abs(X[:2]) - np.eye(2)[:, ::1 if which == "SA" else -1])) <= 64 * E.EPS
    v0.free()
    # a zero start vector
    z = ctx.upload(np.zeros(6))
    s = ctx.eigs(dD, k=2, which="SA", v0=z)
    st = s.solve(max_cycles=2)
    print(f"zero v0: reason {E.REASONS[st['reason']]} products {st['products']}")
    assert st["stopped"] and not st["converged"] and st["reason"] == E.BAD_START and st["products"] == 0 and st["restarts"] == 0
    s.free()
    nan = ctx.upload(np.array([1.0, np.nan, 0.0, 0.0, 0.0, 0.0]))
    s = ctx.eigs(dD, k=2, which="SA", v0=nan)
    st = s.solve(max_cycles=2)
    assert st["stopped"] and not st["converged"] and st["reason"] == E.BAD_START and st["products"] == 0
    s.free()
    for v in (z, nan):
        v.free()
    dD.free()


def test_refusals(ctx, cache):
    from basic_iterative_solvers_amd import BisError
    dA = cache.system("anderson5")["dA"]  # n = 125

    def refused(what, fn):
        with pytest.raises(BisError) as err:
            fn()
        print(f"{what}: {err.value}")
        return str(err.value)

    assert "ncv must exceed k" in refused("ncv <= k", lambda: ctx.eigs(dA, k=4, ncv=4))
    assert "ncv must not exceed min(n, 64)" in refused("ncv > 64", lambda: ctx.eigs(dA, k=4, ncv=65))
    d7 = diag_matrix(ctx, np.arange(1.0, 8.0))
    assert "ncv must not exceed min(n, 64)" in refused("ncv > n", lambda: ctx.eigs(d7, k=2, ncv=8))
    d7.free()
    assert "k must be at least 1" in refused("k < 1", lambda: ctx.eigs(dA, k=0))
    assert "n must be at least 2" in refused("n < 2", lambda: ctx.eigs(None, k=1, n=1))
    rect = ctx.matrix(CRS(3, np.array([0, 1, 2, 3]), np.zeros(3, np.int32), np.ones(3), n_cols=2))
    assert "square matrix required" in refused("rectangular A", lambda: ctx.eigs(rect, k=1, ncv=2))
    rect.free()
    s = ctx.eigs(None, k=2, n=125)
    s.init()
    assert "bis_eigs_iterate" in refused("iterate on a caller-applied handle", lambda: s.iterate(1))
    assert "bis_eigs_op_end" in refused("op_end without op_begin", s.op_end)
    s.op_begin()
    assert "bis_eigs_op_begin" in refused("two op_begin", s.op_begin)
    s.free()
    s = ctx.eigs(dA, k=2)
    s.init()
    assert "bis_eigs_vectors" in refused("vectors before a restart", s.vectors)
    assert "bis_eigs_set_start" in refused("set_start after init", lambda: s.set_start(None))
    s.free()


def test_shift_and_invert_in_the_caller_applied_mode(ctx):
    """H - 0.3 I from the generator; each product is a MINRES solve from x = 0; 0.3 + 1 / theta are the eigenvalues of H
    nearest 0.3."""
    sigma, k, ncv = 0.3, 4, 24
    dS = ctx.gen_anderson(6, shift=-sigma)
    hS = host_of(dS)
    n = hS.n_rows
    H = E.dense_of(hS) + sigma * np.eye(n)
    lam = np.linalg.eigvalsh(H)
    b, x = ctx.alloc(n), ctx.alloc(n)
    mr = ctx.minres(dS, b, x)
    s = ctx.eigs(None, k=k, which="LM", ncv=ncv, tol=TOL, n=n)
    s.init()
    inner = []
    st = s.status()
    for cycle in range(6):
        for _ in range(ncv if cycle == 0 else ncv - E.keep_count(k, ncv)):
            inp, out = s.op_begin()
            ctx.copy_vector(b, inp, n)
            ctx.init_vector(x, 0.0, n)
            mr.init(1e-12)
            for _ in range(40):
                mr.iterate(50)
                iters, conv, _ = mr.status()
                if conv:
                    break
            assert conv
            inner.append(iters)
            ctx.copy_vector(out, x, n)
            s.op_end()
        st = s.status()
        if st["stopped"]:
            break
    X = s.vectors()
    values = sigma + 1.0 / st["values"]
    want = lam[np.argsort(np.abs(lam - sigma), kind="stable")[:k]]
    dist, bound, _ = E.eigen_bound(H, values, X)
    print(f"shift-and-invert: {st['products']} products in {st['restarts']} cycles, {min(inner)} to {max(inner)} MINRES iterations "
          f"each; eigenvalues {values}, max error {np.max(np.abs(np.sort(values) - np.sort(want))):.2e}, bound {np.max(bound):.2e}")
    assert st["converged"] and st["reason"] == E.CONVERGED
    assert np.all(dist <= bound)
    assert np.max(np.abs(np.sort(values) - np.sort(want))) <= np.max(bound)
    for v in (b, x):
        v.free()
    mr.free()
    s.free()
    dS.free()
