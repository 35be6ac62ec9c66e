"""GPU: bis_mgmres_* (k restarted GMRES(m) solves in lock-step) column by column against a single-column GMRES(m) made of the
library's single-vector calls with host scalars (the Givens algebra in numpy), and against the oracle's GMRES on one column;
restart lengths, the independence of the columns, the freeze of a stopped column, call splitting, a breakdown column,
bis_mgmres_solution, determinism, the argument checks, n = 1 and n = 0.

bis_spmm and bis_mapply_preconditioner equal, per column, what the single-column loop calls bit for bit (with the provisos of
include/bis_hip.h), so only the reduction trees and the rounding of the small dense algebra differ.  The gate is the
project's GMRES gate (tests/helpers.py): 1e-10 r0 over the whole history, restart entries included; `converged` equal;
iteration counts equal, one apart only where the single-column history sits within 1e-10 r0 of the threshold at the shorter
run's last index; the true preconditioned residual within the last history entry + 1e-10 of the initial preconditioned
residual.  What two correct GMRES runs that differ only in their reduction trees do was measured on the host (numpy,
sequential against 256-way strided tree dots; this band, a 16 x 12 x 10 27-point stencil and a wider band; none and Jacobi;
four columns of this kind; m = 1, 3, 5, 10, 30): histories at most 6.6e-15 r0 apart, all iteration counts equal, estimate
and true preconditioned residual at most 6e-17 of the initial preconditioned residual apart."""
import numpy as np
import pytest

from helpers import HIST_TOL, check_history, hist_dev
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

TOL = 1e-8
ITERS = 300
KMAX = 8
M = 10
PCS = [("none", 0), ("j", 0), ("gs", 0), ("sgs", 0), ("ilu0", 0), ("ilu0it", 3)]
MATS = ["hpcg", "anderson", "fem666", "nsband1921"]


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


def host_spmv(A, x):
    rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
    return np.bincount(rows, weights=A.val * x[A.col], minlength=A.n_rows)


def ns_band(n, half, seed):
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
    for r in range(n):
        for d in range(-half, half + 1):
            c = r + d
            if 0 <= c < n:
                rows.append(r); cols.append(c)
                vals.append(diag[r] if d == 0 else (lo[-d][c] if d < 0 else up[d][r]))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return CRS(n, rp, np.array(cols, dtype=np.int32), np.array(vals))


def columns(A, k, seed):
    """B, X0 (n x k): b_0 = A 1, b_1 uniform random, b_2 a unit vector, the rest random at the scales 1e-6, 1, 1e6;
    start vectors zero in columns 0, 1, 3, 6 and random in the others.  (The first k' < k columns are columns(A, k', seed).)"""
    rng = np.random.default_rng(seed)
    n = A.n_rows
    B = np.empty((n, k))
    X0 = np.zeros((n, k))
    scales = (1e-6, 1.0, 1e6)
    for j in range(k):
        if j == 0:
            B[:, j] = host_spmv(A, np.ones(n))
        elif j == 1:
            B[:, j] = rng.uniform(-1, 1, n)
        elif j == 2:
            B[:, j] = 0.0
            B[n // 3, j] = 1.0
        else:
            B[:, j] = scales[(j - 3) % 3] * rng.uniform(-1, 1, n)
        if j == 2:
            X0[:, j] = np.random.default_rng(2).uniform(-1, 1, n)
        elif j not in (0, 1, 3, 6):
            X0[:, j] = rng.uniform(-1, 1, n) * scales[(j - 3) % 3]
    return B, X0


def pc_args(e, pc, inner):
    """keyword arguments of MGMRES.set_preconditioner for this type"""
    if pc == "none":
        return {}
    if pc in ("j", "gs", "sgs"):
        return dict(Ls=e["Ls"], Us=e["Us"], A_D=e["D"], A_D_inv=e["Dinv"], L_D=e["D"], U_D=e["D"])
    return dict(Ls=e["iLs"], Us=e["iUs"], A_D=e["iLD"], A_D_inv=e["iUinv"], L_D=e["iLD"], U_D=e["iUD"], inner=inner)


class Givens:
    """The (m + 1) x m least-squares problem of one GMRES cycle on the host: the new Hessenberg column is rotated by the stored
    rotations, the new rotation is c = a / den, s = b / den with den = sqrt(a^2 + b^2) (least_squares, gmres.hpp), g follows
    (update_g); y by back substitution on the rotated triangle with y[steps] = 0 (get_explicit_x)."""

    def __init__(self, m, beta):
        self.m = m
        self.R = np.zeros((m + 1, m))
        self.cs, self.sn = np.zeros(m), np.zeros(m)
        self.g = np.zeros(m + 1)
        self.g[0] = beta

    def step(self, n, hcol):
        """hcol: h_0 .. h_{n+1}; returns the estimate |g_{n+1}|"""
        h = np.array(hcol, dtype=np.float64)
        for i in range(n):
            a, b = h[i], h[i + 1]
            h[i] = self.cs[i] * a + self.sn[i] * b
            h[i + 1] = self.cs[i] * b - self.sn[i] * a
        a, b = h[n], h[n + 1]
        den = np.sqrt(a * a + b * b)
        c, s = a / den, b / den
        self.cs[n], self.sn[n] = c, s
        self.R[:n, n] = h[:n]
        self.R[n, n] = c * a + s * b
        self.g[n + 1] = -s * self.g[n]
        self.g[n] = c * self.g[n]
        return abs(self.g[n + 1])

    def y(self, steps):
        y = np.zeros(self.m)
        for r in range(steps - 1, -1, -1):
            y[r] = (self.g[r] - np.dot(self.R[r, r + 1:steps], y[r + 1:steps])) / self.R[r, r]
        return y


def single_ops(e, pc, inner):
    kw = pc_args(e, pc, inner)
    return (kw.get("Ls"), kw.get("Us"), kw.get("A_D"), kw.get("A_D_inv"), kw.get("L_D"), kw.get("U_D"))


def run_single(ctx, e, pc, inner, b, x0, m):
    """One column: gmres_separate_iteration, check_restart and GMRESSolver::init_residual from the single-vector calls with
    host scalars, in the order of gmres.hpp; the history includes the entry a restart writes.  Runs none of bis_mgmres_*."""
    dA, n = e["dA"], e["n"]
    ops = single_ops(e, pc, inner)
    db, x = ctx.upload(b), ctx.upload(x0)
    names = ("r", "w", "t", "vy", "xn", "tmp", "work")
    wk = {q: ctx.alloc(n) for q in names}
    for q in names:
        ctx.init_vector(wk[q], 0.0)
    V = ctx.alloc(n * (m + 1))
    ctx.init_vector(V, 0.0)

    def apply(v):
        if pc != "none":
            ctx.apply_preconditioner(pc, n, *ops, v, v, wk["tmp"], wk["work"], inner=inner)

    def start_cycle():
        ctx.spmv(dA, x, wk["t"])
        ctx.subtract_vectors(wk["r"], db, wk["t"], 1.0)  # b - A x
        unpre = ctx.euclidean_vec_norm(wk["r"])
        apply(wk["r"])
        beta = ctx.euclidean_vec_norm(wk["r"])
        ctx.scale(V.offset(0, n), wk["r"], float(np.float64(1.0) / np.float64(beta)))
        return unpre, beta

    def explicit_x(steps):
        nonlocal x
        ctx.multi_axpy(V, n, G.y(steps), steps, wk["vy"], n)
        ctx.sum_vectors(wk["xn"], x, wk["vy"], 1.0)
        x, wk["xn"] = wk["xn"], x

    with np.errstate(all="ignore"):
        r0, beta = start_cycle()
        hist = [r0]
        stop = TOL * r0
        G = Givens(m, beta)
        iters, conv, pos = 0, False, 0
        while iters < ITERS:
            ctx.spmv(dA, V.offset(pos * n, n), wk["w"])
            apply(wk["w"])
            hcol = []
            for i in range(pos + 1):  # modified Gram-Schmidt
                hcol.append(ctx.dot(wk["w"], V.offset(i * n, n)))
                ctx.subtract_vectors(wk["w"], wk["w"], V.offset(i * n, n), float(hcol[-1]))
            hcol.append(ctx.euclidean_vec_norm(wk["w"]))
            ctx.scale(V.offset((pos + 1) * n, n), wk["w"], float(np.float64(1.0) / np.float64(hcol[-1])))
            est = G.step(pos, hcol)
            iters += 1
            pos += 1
            hist.append(est)
            conv = bool(est < stop)
            if conv or not np.isfinite(est):
                break
            if pos == m:  # check_restart
                explicit_x(pos)
                _, beta = start_cycle()
                hist.append(beta)
                G = Givens(m, beta)
                pos = 0
                conv = bool(beta < stop)
                if conv or not np.isfinite(beta):
                    break
        if pos > 0:
            explicit_x(pos)  # save_x_star
    out = dict(iters=iters, conv=conv, hist=np.array(hist), x=x.to_host())
    for v in list(wk.values()) + [db, x, V]:
        v.free()
    return out


def pre_resnorm(ctx, e, pc, inner, b, x):
    """|| M^-1 (b - A x) || with the device's single-vector calls (M = I for none)"""
    n = e["n"]
    db, dx, t, r, tmp, work = ctx.upload(b), ctx.upload(x), ctx.alloc(n), ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
    ctx.spmv(e["dA"], dx, t)
    ctx.subtract_vectors(r, db, t, 1.0)
    if pc != "none":
        ctx.apply_preconditioner(pc, n, *single_ops(e, pc, inner), r, r, tmp, work, inner=inner)
    out = ctx.euclidean_vec_norm(r)
    for v in (db, dx, t, r, tmp, work):
        v.free()
    return out


def mgm_state(m, dX, n, k):
    st = [m.status(j) for j in range(k)]
    return dict(iters=[s[0] for s in st], conv=[s[1] for s in st], hist=[s[2] for s in st], X=dX.to_host().reshape(n, k))


def run_mgm(ctx, e, pc, inner, B, X0, m=M, steps=(ITERS,), solution_after=None):
    """One lock-step solve; pc None: no set_preconditioner call.  Returns the state after each entry of `steps` further
    iterations; solution_after = i: that state also carries bis_mgmres_solution's block ("sol")."""
    n, k = B.shape
    dB, dX = ctx.upload(B.ravel()), ctx.upload(X0.ravel())
    s = ctx.mgmres(e["dA"], dB, dX, k, restart=m)
    if pc is not None:
        s.set_preconditioner(pc, **pc_args(e, pc, inner))
    r0 = s.init(TOL)
    out = []
    for i, it in enumerate(steps):
        s.iterate(it)
        out.append(mgm_state(s, dX, n, k))
        out[-1]["r0"] = r0
        if solution_after == i:
            dS = ctx.alloc(n * k)
            ctx.init_vector(dS, -7.0)
            s.solution(dS)
            out[-1]["sol"] = dS.to_host().reshape(n, k)
            dS.free()
            after = mgm_state(s, dX, n, k)  # bis_mgmres_solution changes nothing
            assert same_bits(after["X"], out[-1]["X"]) and after["iters"] == out[-1]["iters"]
    s.free(); dB.free(); dX.free()
    return out


def make_system(ctx, dA):
    n = dA.n_rows
    A = CRS(n, *dA.download())
    Ls, Us, D, Dinv = ctx.split_strict(dA)
    iLs, iLD, iUs, iUD = ctx.ilu0(dA)
    iUinv = ctx.alloc(n)
    ctx.elemwise_div_vectors(iUinv, iLD, iUD)
    B, X0 = columns(A, KMAX, seed=100 + KMAX)
    return dict(dA=dA, A=A, n=n, Ls=Ls, Us=Us, D=D, Dinv=Dinv, iLs=iLs, iLD=iLD, iUs=iUs, iUD=iUD, iUinv=iUinv, B=B, X0=X0,
                single={}, mgm={})


@pytest.fixture(scope="module")
def systems(ctx):
    """Per matrix: the operands of every preconditioner type and the 8 columns -- built once, never changed."""
    out = {}
    for name in MATS + ["one"]:
        if name == "hpcg":
            dA = ctx.gen_hpcg(16, 12, 10)
        elif name == "anderson":
            dA = ctx.gen_anderson(14, shift=9.0)
        elif name == "fem666":
            dA = ctx.gen_fem(6, 6, 6)
        elif name == "nsband1921":
            dA = ctx.matrix(ns_band(1921, 3, 1))
        else:
            dA = ctx.matrix(CRS(1, np.array([0, 1], dtype=np.int64), np.zeros(1, np.int32), np.array([2.5])))
        out[name] = make_system(ctx, dA)
    return out


def single_refs(ctx, e, pc, inner, m=M):
    """the KMAX single-column solves of this matrix, type and restart length, computed once and shared"""
    key = (pc, inner, m)
    if key not in e["single"]:
        e["single"][key] = [run_single(ctx, e, pc, inner, e["B"][:, j].copy(), e["X0"][:, j].copy(), m) for j in range(KMAX)]
    return e["single"][key]


def mgm_ref(ctx, e, pc, inner, k, m=M):
    key = (pc, inner, k, m)
    if key not in e["mgm"]:
        e["mgm"][key] = run_mgm(ctx, e, pc, inner, e["B"][:, :k].copy(), e["X0"][:, :k].copy(), m=m)[0]
    return e["mgm"][key]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_column(ctx, tag, e, pc, inner, j, m_iters, m_conv, m_hist, m_x, ref):
    r0 = ref["hist"][0]
    dev = hist_dev(m_hist, ref["hist"])
    res = pre_resnorm(ctx, e, pc, inner, e["B"][:, j], m_x)
    res0 = pre_resnorm(ctx, e, pc, inner, e["B"][:, j], e["X0"][:, j])
    print(f"{tag}: mgmres iters {m_iters} conv {m_conv} entries {len(m_hist)}, single iters {ref['iters']} conv {ref['conv']} "
          f"entries {len(ref['hist'])}, hist dev {dev:.3e}, true preconditioned residual {res:.6e}, last history entry "
          f"{m_hist[-1]:.6e}, excess over the estimate {(res - m_hist[-1]) / res0:.3e} of the initial {res0:.6e}, r0 {r0:.6e}")
    assert dev <= HIST_TOL["gm"], tag
    assert m_conv == ref["conv"], tag
    if m_iters != ref["iters"]:  # accepted only as a tie at the threshold
        assert abs(m_iters - ref["iters"]) == 1, tag
        last = min(len(m_hist), len(ref["hist"])) - 1
        gap = abs(ref["hist"][last] - TOL * r0) / r0
        print(f"{tag}: TIE iteration counts {m_iters} / {ref['iters']}, the single-column entry {last} is {gap:.3e} r0 from the threshold")
        assert gap <= 1e-10, tag
    else:
        assert len(m_hist) == len(ref["hist"]), tag
    assert res <= m_hist[-1] + 1e-10 * res0, tag


def check_run(ctx, name, e, pc, inner, k, m):
    ref = single_refs(ctx, e, pc, inner, m)
    run = mgm_ref(ctx, e, pc, inner, k, m)
    print(f"{name} {pc} k={k} m={m}: single iteration counts {[c['iters'] for c in ref[:k]]}, mgmres {run['iters']}")
    for j in range(k):
        check_column(ctx, f"{name} {pc} k={k} m={m} j={j}", e, pc, inner, j, run["iters"][j], run["conv"][j], run["hist"][j],
                     run["X"][:, j], ref[j])
    assert all(run["conv"]), (name, pc, k, m, run["conv"])
    return run


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("pc,inner", PCS)
@pytest.mark.parametrize("name", MATS)
def test_parity_with_single_column_gmres(ctx, systems, name, pc, inner, k):
    check_run(ctx, name, systems[name], pc, inner, k, M)


RESTART_CASES = [(name, pc) for name in ("hpcg", "nsband1921") for pc in ("none", "ilu0")]


@pytest.mark.parametrize("m", [1, 3, 30])
@pytest.mark.parametrize("name,pc", RESTART_CASES)
def test_restart_lengths(ctx, systems, name, pc, m):
    run = check_run(ctx, name, systems[name], pc, 0, KMAX, m)
    restarts = [len(h) - it - 1 for h, it in zip(run["hist"], run["iters"])]
    print(f"{name} {pc} m={m}: iterations {run['iters']}, restarts {restarts}")
    for j in range(KMAX):  # a restart after every full cycle the column did not stop in (one more where it stopped on beta)
        assert restarts[j] in ((run["iters"][j] - 1) // m, run["iters"][j] // m), (name, pc, m, j)
    if m == 1:  # a restart after every iteration
        assert all(r >= it - 1 for r, it in zip(restarts, run["iters"]))


def test_restart_cases_exercise_what_they_are_for(ctx, systems):
    runs = {m: [mgm_ref(ctx, systems[name], pc, 0, KMAX, m) for name, pc in RESTART_CASES] for m in (1, 3, 30)}
    its = {m: [it for run in runs[m] for it in run["iters"]] for m in runs}
    print(f"iterations with m = 1: {its[1]}, m = 3: {its[3]}, m = 30: {its[30]}")
    assert any(it > 3 for it in its[3]), "m = 3: no column restarts"
    assert any(it % 3 != 0 for it in its[3]), "m = 3: no column stops inside a cycle"
    assert any(it <= 30 for it in its[30]), "m = 30: every column restarts"
    assert any(it > 1 for it in its[1]), "m = 1: no column restarts"
    for run in runs[1]:
        for h, it in zip(run["hist"], run["iters"]):
            assert len(h) - it - 1 >= it - 1


@pytest.mark.parametrize("m", [3, 10])
@pytest.mark.parametrize("pc", ["none", "sgs", "ilu0"])
@pytest.mark.parametrize("name", MATS)
def test_anchor_against_the_oracle(ctx, oracle, systems, name, pc, m):
    """One column, b = 1, x0 = 0.1 (the oracle's default start), k = 1, against the oracle's GMRES(m): the same iteration, the
    same restart entries in the history, the same stop test."""
    e = systems[name]
    n = e["n"]
    o = oracle.solve(e["A"], "gm", pc, tol=TOL, restart_len=m, ilu_real=True)
    run = run_mgm(ctx, e, pc, 0, np.ones((n, 1)), np.full((n, 1), 0.1), m=m)[0]
    r = dict(hist=run["hist"][0], converged=run["conv"][0], iters=run["iters"][0])
    print(f"{name} {pc} m={m}: mgmres iters {r['iters']} entries {len(r['hist'])} conv {r['converged']}, oracle entries {len(o['hist'])} "
          f"conv {o['converged']}, hist dev {hist_dev(r['hist'], o['hist']):.3e}")
    check_history(r, o, "gm")
    assert len(r["hist"]) == len(o["hist"])
    assert r["converged"] == o["converged"]


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("pc,inner", PCS)
def test_one_row(ctx, systems, pc, inner, k):
    """n = 1: W - h_0 V_0 is exactly 0 after the first step (a lucky breakdown), so every column converges at iteration 1 --
    except one with b = 0 and x0 = 0, which is NaN at iteration 1 on both sides."""
    e = systems["one"]
    B, X0 = e["B"][:, :k].copy(), e["X0"][:, :k].copy()
    zero = 1 if k > 1 else None  # (columns() starts column 1 at x0 = 0)
    if zero is not None:
        B[:, zero] = 0.0
    run = run_mgm(ctx, e, pc, inner, B, X0)[0]
    for j in range(k):
        ref = run_single(ctx, e, pc, inner, B[:, j].copy(), X0[:, j].copy(), M)
        tag = f"one {pc} k={k} j={j}"
        print(f"{tag}: mgmres {run['iters'][j]} {run['conv'][j]} {run['hist'][j]}, single {ref['iters']} {ref['conv']} {ref['hist']}")
        assert (run["iters"][j], run["conv"][j]) == (ref["iters"], ref["conv"]) == ((1, False) if j == zero else (1, True)), tag
        assert len(run["hist"][j]) == len(ref["hist"]) == 2, tag
        assert np.allclose(run["hist"][j], ref["hist"], rtol=0.0, atol=1e-10 * ref["hist"][0], equal_nan=True), tag
        assert np.array_equal(np.isnan(run["hist"][j]), np.isnan(ref["hist"])), tag
        if j == zero:
            assert run["r0"][j] == 0.0 and np.isnan(run["hist"][j][1]), tag
        else:
            res = abs(B[0, j] - 2.5 * run["X"][0, j])
            assert res <= run["hist"][j][-1] + 1e-10 * run["hist"][j][0], tag


def test_no_rows(ctx):
    """n = 0: create / set_preconditioner / init / iterate / solution / status / destroy return BIS_OK and launch nothing."""
    dA = ctx.matrix(CRS(0, np.zeros(1, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0)))
    dB, dX, dS = ctx.alloc(1), ctx.alloc(1), ctx.alloc(1)
    for k in (1, 3, 8):
        s = ctx.mgmres(dA, dB, dX, k, restart=5)
        s.set_preconditioner("j")
        r0 = s.init(TOL)
        assert r0.shape == (k,) and not r0.any()
        s.iterate(7)
        s.solution(dS)
        it, conv, hist = s.status(k - 1)
        assert (it, conv) == (0, False) and len(hist) == 0
        s.free()
    dB.free(); dX.free(); dS.free(); dA.free()


@pytest.mark.parametrize("pc,inner", [("none", 0), ("ilu0", 0)])
@pytest.mark.parametrize("name", MATS)
def test_columns_never_mix(ctx, systems, name, pc, inner):
    """Column j of a k = 8 solve keeps its bits (x, history, iteration count) when the other seven columns carry other data
    and one of them breaks down at once."""
    e = systems[name]
    full = mgm_ref(ctx, e, pc, inner, KMAX)
    rng = np.random.default_rng(9)
    for j in (0, 5):
        B, X0 = rng.uniform(-3, 3, e["B"].shape), rng.uniform(-3, 3, e["X0"].shape)
        B[:, (j + 1) % KMAX] = 0.0  # (one of the others breaks down at once)
        X0[:, (j + 1) % KMAX] = 0.0
        B[:, j], X0[:, j] = e["B"][:, j], e["X0"][:, j]
        run = run_mgm(ctx, e, pc, inner, B, X0)[0]
        assert (run["iters"][(j + 1) % KMAX], run["conv"][(j + 1) % KMAX]) == (1, False)
        assert run["iters"][j] == full["iters"][j] and run["conv"][j] == full["conv"][j], (name, pc, j)
        assert same_bits(run["hist"][j], full["hist"][j]) and same_bits(run["X"][:, j], full["X"][:, j]), (name, pc, j)
        other = (j + 2) % KMAX
        assert not same_bits(run["hist"][other][:2], full["hist"][other][:2])


@pytest.mark.parametrize("pc,inner", [("none", 0), ("sgs", 0), ("ilu0", 0), ("ilu0it", 3)])
@pytest.mark.parametrize("name", MATS)
def test_freeze_determinism_and_call_splitting(ctx, systems, name, pc, inner):
    e = systems[name]
    k = KMAX
    full = mgm_ref(ctx, e, pc, inner, k)

    def same_state(a, b):
        return (a["iters"] == b["iters"] and a["conv"] == b["conv"] and same_bits(a["X"], b["X"]) and
                all(same_bits(a["hist"][j], b["hist"][j]) for j in range(k)))

    again = run_mgm(ctx, e, pc, inner, e["B"], e["X0"])[0]  # two runs, the same bits
    assert same_state(again, full)
    # the cycle position persists across calls: no call boundary restarts a cycle
    split = run_mgm(ctx, e, pc, inner, e["B"], e["X0"], steps=(4, 3, 1, ITERS - 8))[-1]
    assert same_state(split, full)
    # the column that stops first: its X and history do not move during 20 further iterations (the others go on)
    first = int(np.argmin(full["iters"]))
    it0 = full["iters"][first]
    # (an exact or nearly exact preconditioner stops all eight columns in the same iteration, and then no column is left to
    # advance; without a preconditioner every matrix here has columns that go on, and there the advance is asserted)
    others_go_on = max(full["iters"]) > it0
    assert others_go_on or pc != "none", f"every column stopped at iteration {it0}: the freeze is not exercised"
    at, later = run_mgm(ctx, e, pc, inner, e["B"], e["X0"], steps=(it0, 20))
    assert at["iters"][first] == it0 and later["iters"][first] == it0 and later["conv"][first] == at["conv"][first]
    assert same_bits(later["X"][:, first], at["X"][:, first]) and same_bits(later["hist"][first], at["hist"][first])
    assert same_bits(at["X"][:, first], full["X"][:, first]) and same_bits(at["hist"][first], full["hist"][first])
    if others_go_on:
        assert max(later["iters"]) > it0, "no other column advanced: the freeze was not exercised"
    # ... and when every column has stopped nothing moves at all
    done, after = run_mgm(ctx, e, pc, inner, e["B"], e["X0"], steps=(ITERS, 20))
    assert same_state(done, full) and same_state(after, done)


@pytest.mark.parametrize("pc,inner", [("none", 0), ("ilu0", 0)])
@pytest.mark.parametrize("name", ["hpcg", "nsband1921"])
def test_breakdown_column_stops_alone(ctx, systems, name, pc, inner):
    """b_j = 0 with x0_j = 0: beta = 0, V_0 = 0 / 0 -- NaN at iteration 1, stopped, not converged, as the other lock-step
    solvers pin it; the other columns converge with the bits they have without it."""
    e = systems[name]
    k = 4
    base = mgm_ref(ctx, e, pc, inner, k)
    B, X0 = e["B"][:, :k].copy(), e["X0"][:, :k].copy()
    B[:, 2] = 0.0
    X0[:, 2] = 0.0
    run = run_mgm(ctx, e, pc, inner, B, X0)[0]
    single = run_single(ctx, e, pc, inner, B[:, 2].copy(), X0[:, 2].copy(), M)
    assert (single["iters"], single["conv"]) == (1, False)
    assert (run["iters"][2], run["conv"][2]) == (1, False) and run["r0"][2] == 0.0
    assert np.array_equal(run["hist"][2], single["hist"], equal_nan=True) and np.isnan(run["hist"][2][1])
    for j in (0, 1, 3):
        assert run["conv"][j] and run["iters"][j] == base["iters"][j], j
        assert same_bits(run["hist"][j], base["hist"][j]) and same_bits(run["X"][:, j], base["X"][:, j]), j


@pytest.mark.parametrize("name", MATS)
def test_solution_of_a_run_that_ends_on_a_budget(ctx, systems, name):
    """m = 10, no preconditioner, k = 8, init + 4 iterations: bis_mgmres_solution gives X + V y of the current step for a live
    column (its X is still the start vector) and X itself, bit for bit, for a stopped one; going on afterwards gives the
    bits of an uninterrupted run."""
    e = systems[name]
    k = KMAX
    full = mgm_ref(ctx, e, "none", 0, k)
    mid, end = run_mgm(ctx, e, "none", 0, e["B"], e["X0"], steps=(4, ITERS - 4), solution_after=0)
    live = [j for j in range(k) if full["iters"][j] > 4]
    print(f"{name}: iterations of the full run {full['iters']}, live after 4: {live}")
    for j in range(k):
        tag = f"{name} j={j}"
        if j in live:
            assert mid["iters"][j] == 4 and len(mid["hist"][j]) == 5, tag
            assert same_bits(mid["X"][:, j], e["X0"][:, j]), tag
            res = np.linalg.norm(e["B"][:, j] - host_spmv(e["A"], mid["sol"][:, j]))
            print(f"{tag}: || b - A sol || {res:.6e}, estimate {mid['hist'][j][-1]:.6e}, r0 {mid['hist'][j][0]:.6e}")
            assert res <= mid["hist"][j][-1] + 1e-10 * mid["hist"][j][0], tag
        else:
            assert mid["iters"][j] == full["iters"][j] and same_bits(mid["sol"][:, j], mid["X"][:, j]), tag
            assert same_bits(mid["X"][:, j], full["X"][:, j]), tag
    assert end["iters"] == full["iters"] and end["conv"] == full["conv"] and same_bits(end["X"], full["X"])
    for j in range(k):
        assert same_bits(end["hist"][j], full["hist"][j]), j
    # every column stopped: the solution is X
    done = run_mgm(ctx, e, "none", 0, e["B"], e["X0"], steps=(ITERS,), solution_after=0)[0]
    assert same_bits(done["sol"], done["X"]) and same_bits(done["X"], full["X"])


def test_argument_checks(ctx, systems):
    from basic_iterative_solvers_amd import BisError
    e = systems["nsband1921"]
    k = 3
    dB, dX = ctx.upload(e["B"][:, :k].ravel()), ctx.upload(e["X0"][:, :k].ravel())
    for bad_m in (0, 65):
        with pytest.raises(BisError, match="status 2"):
            ctx.mgmres(e["dA"], dB, dX, k, restart=bad_m)
    for bad_k in (0, 9):
        with pytest.raises(BisError, match="status 2"):
            ctx.mgmres(e["dA"], dB, dX, bad_k)
    s = ctx.mgmres(e["dA"], dB, dX, k, restart=64)
    for pc in ("2st", "s2st"):
        with pytest.raises(BisError, match="status 6"):  # BIS_ERR_UNSUPPORTED
            s.set_preconditioner(pc, Ls=e["Ls"], Us=e["Us"], A_D=e["D"], A_D_inv=e["Dinv"], inner=2)
    with pytest.raises(BisError, match="status 6"):
        s.set_preconditioner("sgs", **pc_args(e, "sgs", 0), outer=2)
    with pytest.raises(BisError, match="status 2"):  # an operand the type reads is missing: refused here, not at init
        s.set_preconditioner("gs", A_D=e["D"])
    with pytest.raises(BisError, match="status 2"):
        s.set_preconditioner("sgs", Ls=e["Ls"], Us=e["Us"])
    s.set_preconditioner("sgs", **pc_args(e, "sgs", 0))
    s.init(TOL)
    with pytest.raises(BisError, match="status 2"):  # BIS_ERR_INVALID after bis_mgmres_init
        s.set_preconditioner("ilu0", **pc_args(e, "ilu0", 0))
    s.free()
    dB.free(); dX.free()
