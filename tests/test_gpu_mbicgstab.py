"""GPU: bis_mbicgstab_* (k BiCGSTAB solves in lock-step) column by column against a single-column BiCGSTAB made of the
library's single-vector calls with host scalars, and against the oracle's BiCGSTAB on one column; the independence of the
columns, the freeze of a stopped column, a breakdown column, determinism, the argument checks, n = 1 and n = 0.

bis_spmm and bis_mapply_preconditioner equal, per column, what the single-column loop calls bit for bit (with the provisos of
include/bis_hip.h), so only the reduction trees differ.  The gates are the project's BiCGSTAB gates (tests/helpers.py):
1e-4 r0 over the whole history, 1e-10 r0 over the first three entries; iteration counts within max(2, len // 10) (the
residuals of BiCGSTAB are not monotone near the threshold); the true residual within the last history entry + 1e-10 r0.
What two correct BiCGSTABs that differ only in their reduction trees do on matrices of these kinds was measured on the
host (numpy, sequential against 256-way strided tree dots, tol 1e-8, these eight columns, none / j / gs / sgs): whole
history at most 4.3e-7 r0 apart, first three entries at most 1.0e-12, iteration counts at most 2."""
import numpy as np
import pytest

from helpers import HIST_TOL, check_history, hist_dev
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

TOL = 1e-8
ITERS = 300
KMAX = 8
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
    """keyword arguments of MBiCGSTAB.set_preconditioner for this type"""
    if pc == "none":
        return {}
    if pc in ("j", "gs", "sgs"):
        return dict(Ls=e["Ls"], Us=e["Us"], A_D=e["D"], A_D_inv=e["Dinv"], L_D=e["D"], U_D=e["D"])
    return dict(Ls=e["iLs"], Us=e["iUs"], A_D=e["iLD"], A_D_inv=e["iUinv"], L_D=e["iLD"], U_D=e["iUD"], inner=inner)


def run_single(ctx, e, pc, inner, b, x0):
    """One column: bicgstab_separate_iteration and BiCGSTABSolver::init_residual from the single-vector calls, host scalars,
    the stop test of solver.hpp:177-192.  Runs none of bis_mbicgstab_*."""
    dA, n = e["dA"], e["n"]
    kw = pc_args(e, pc, inner)
    ops = (kw.get("Ls"), kw.get("Us"), kw.get("A_D"), kw.get("A_D_inv"), kw.get("L_D"), kw.get("U_D"))
    db, x = ctx.upload(b), ctx.upload(x0)
    names = ("xn", "h", "r", "rn", "r0", "p", "pn", "v", "s", "st", "y", "z", "t", "tmp", "work")
    w = {q: ctx.alloc(n) for q in names}
    for q in names:
        ctx.init_vector(w[q], 0.0)

    def apply(out, inp):
        ctx.apply_preconditioner(pc, n, *ops, out, inp, w["tmp"], w["work"], inner=inner)

    f = np.float64
    ctx.spmv(dA, x, w["t"])
    ctx.subtract_vectors(w["r"], db, w["t"], 1.0)  # b - A x0
    hist = [ctx.euclidean_vec_norm(w["r"])]
    stop = TOL * hist[0]
    apply(w["p"], w["r"])
    ctx.copy_vector(w["r0"], w["p"])  # the shadow residual is the preconditioned initial residual
    rho = f(ctx.dot(w["r"], w["p"]))
    conv = False
    with np.errstate(all="ignore"):
        for _ in range(ITERS):
            apply(w["y"], w["p"])
            ctx.spmv(dA, w["y"], w["v"])
            alpha = rho / f(ctx.dot(w["r0"], w["v"]))
            ctx.subtract_vectors(w["s"], w["r"], w["v"], float(alpha))
            apply(w["st"], w["s"])
            ctx.spmv(dA, w["st"], w["z"])
            omega = f(ctx.dot(w["z"], w["s"])) / f(ctx.dot(w["z"], w["z"]))
            ctx.sum_vectors(w["h"], x, w["y"], float(alpha))
            ctx.sum_vectors(w["xn"], w["h"], w["st"], float(omega))
            ctx.subtract_vectors(w["rn"], w["s"], w["z"], float(omega))
            rho_new = f(ctx.dot(w["r0"], w["rn"]))
            beta = (rho_new / rho) * (alpha / omega)
            ctx.subtract_vectors(w["t"], w["p"], w["v"], float(omega))
            ctx.sum_vectors(w["pn"], w["rn"], w["t"], float(beta))
            norm = ctx.euclidean_vec_norm(w["rn"])
            hist.append(norm)
            w["p"], w["pn"] = w["pn"], w["p"]
            w["r"], w["rn"] = w["rn"], w["r"]
            x, w["xn"] = w["xn"], x
            rho = rho_new
            conv = bool(abs(norm) < stop)
            if conv or not np.isfinite(norm):
                break
    out = dict(iters=len(hist) - 1, conv=conv, hist=np.array(hist), x=x.to_host())
    for v in list(w.values()) + [db, x]:
        v.free()
    return out


def mbi_state(m, dX, n, k):
    st = [m.status(j) for j in range(k)]
    return dict(iters=[s[0] for s in st], conv=[s[1] for s in st], hist=[s[2] for s in st], X=dX.to_host().reshape(n, k))


def run_mbi(ctx, e, pc, inner, B, X0, steps=(ITERS,)):
    """One lock-step solve; pc None: no set_preconditioner call.  Returns the state after each entry of `steps` further iterations."""
    n, k = B.shape
    dB, dX = ctx.upload(B.ravel()), ctx.upload(X0.ravel())
    m = ctx.mbicgstab(e["dA"], dB, dX, k)
    if pc is not None:
        m.set_preconditioner(pc, **pc_args(e, pc, inner))
    r0 = m.init(TOL)
    out = []
    for s in steps:
        m.iterate(s)
        out.append(mbi_state(m, dX, n, k))
        out[-1]["r0"] = r0
    m.free(); dB.free(); dX.free()
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
                single={}, mbi={})


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


def single_refs(ctx, e, pc, inner):
    """the KMAX single-column solves of this matrix and type, computed once and shared"""
    key = (pc, inner)
    if key not in e["single"]:
        e["single"][key] = [run_single(ctx, e, pc, inner, e["B"][:, j].copy(), e["X0"][:, j].copy()) for j in range(KMAX)]
    return e["single"][key]


def mbi_ref(ctx, e, pc, inner, k):
    key = (pc, inner, k)
    if key not in e["mbi"]:
        e["mbi"][key] = run_mbi(ctx, e, pc, inner, e["B"][:, :k].copy(), e["X0"][:, :k].copy())[0]
    return e["mbi"][key]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_column(tag, A, b, m_iters, m_conv, m_hist, m_x, ref):
    dev, dev3 = hist_dev(m_hist, ref["hist"]), hist_dev(m_hist[:3], ref["hist"][:3])
    res = np.linalg.norm(b - host_spmv(A, m_x))
    print(f"{tag}: mbicgstab iters {m_iters} conv {m_conv}, single iters {ref['iters']} conv {ref['conv']}, hist dev {dev:.3e}, "
          f"first three {dev3:.3e}, true residual {res:.6e}, last history entry {m_hist[-1]:.6e}, r0 {m_hist[0]:.6e}")
    assert dev <= HIST_TOL["bi"], tag
    assert dev3 <= 1e-10, tag
    assert m_conv == ref["conv"], tag
    assert abs(m_iters - ref["iters"]) <= max(2, len(ref["hist"]) // 10), tag
    assert res <= m_hist[-1] + 1e-10 * m_hist[0], tag


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("pc,inner", PCS)
@pytest.mark.parametrize("name", MATS)
def test_parity_with_single_column_bicgstab(ctx, systems, name, pc, inner, k):
    e = systems[name]
    ref = single_refs(ctx, e, pc, inner)
    run = mbi_ref(ctx, e, pc, inner, k)
    print(f"{name} {pc} k={k}: single iteration counts {[c['iters'] for c in ref[:k]]}, mbicgstab {run['iters']}")
    for j in range(k):
        check_column(f"{name} {pc} k={k} j={j}", e["A"], e["B"][:, j], run["iters"][j], run["conv"][j], run["hist"][j],
                     run["X"][:, j], ref[j])
    assert all(run["conv"]), (name, pc, k, run["conv"])


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("pc,inner", PCS)
def test_one_row(ctx, systems, pc, inner, k):
    """n = 1: every sum has one term, so both sides do the same arithmetic -- the same stop (a 0/0 breakdown where s = 0
    exactly, convergence otherwise), the histories equal to 1e-10 r0 with NaN at the same places."""
    e = systems["one"]
    ref = single_refs(ctx, e, pc, inner)
    run = mbi_ref(ctx, e, pc, inner, k)
    for j in range(k):
        tag = f"one {pc} k={k} j={j}"
        print(f"{tag}: mbicgstab {run['iters'][j]} {run['conv'][j]} {run['hist'][j]}, single {ref[j]['iters']} {ref[j]['conv']} {ref[j]['hist']}")
        assert (run["iters"][j], run["conv"][j]) == (ref[j]["iters"], ref[j]["conv"]), tag
        assert np.allclose(run["hist"][j], ref[j]["hist"], rtol=0.0, atol=1e-10 * ref[j]["hist"][0], equal_nan=True), tag
        if run["conv"][j]:
            res = abs(e["B"][0, j] - 2.5 * run["X"][0, j])
            assert res <= run["hist"][j][-1] + 1e-10 * run["hist"][j][0], tag


def test_no_rows(ctx):
    """n = 0: create / set_preconditioner / init / iterate / status / destroy return BIS_OK and launch nothing."""
    dA = ctx.matrix(CRS(0, np.zeros(1, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0)))
    dB, dX = ctx.alloc(1), ctx.alloc(1)
    for k in (1, 3, 8):
        m = ctx.mbicgstab(dA, dB, dX, k)
        m.set_preconditioner("j")
        r0 = m.init(TOL)
        assert r0.shape == (k,) and not r0.any()
        m.iterate(5)
        assert m.status(k - 1)[:2] == (0, False)
        m.free()
    dB.free(); dX.free(); dA.free()


@pytest.mark.parametrize("pc", ["none", "sgs", "ilu0"])
@pytest.mark.parametrize("name", MATS)
def test_anchor_against_the_oracle(ctx, oracle, systems, name, pc):
    """One column, b = 1, x0 = 0.1 (the oracle's default start), k = 1, against the oracle's BiCGSTAB: the same recurrences,
    the same shadow residual, the same stop test."""
    e = systems[name]
    n = e["n"]
    o = oracle.solve(e["A"], "bi", pc, tol=TOL, ilu_real=True)
    run = run_mbi(ctx, e, pc, 0, np.ones((n, 1)), np.full((n, 1), 0.1))[0]
    r = dict(hist=run["hist"][0], converged=run["conv"][0], iters=run["iters"][0])
    print(f"{name} {pc}: mbicgstab iters {r['iters']} conv {r['converged']}, oracle iters {o['iters']} conv {o['converged']}, "
          f"hist dev {hist_dev(r['hist'], o['hist']):.3e}, first three {hist_dev(r['hist'][:3], o['hist'][:3]):.3e}")
    check_history(r, o, "bi")
    assert r["converged"] == o["converged"]


@pytest.mark.parametrize("pc,inner", [("none", 0), ("ilu0", 0)])
@pytest.mark.parametrize("name", MATS)
def test_columns_never_mix(ctx, systems, name, pc, inner):
    """Column j of a k = 8 solve keeps its bits (x and history) when the other seven columns carry other data."""
    e = systems[name]
    full = mbi_ref(ctx, e, pc, inner, KMAX)
    rng = np.random.default_rng(9)
    for j in (0, 5):
        B, X0 = rng.uniform(-3, 3, e["B"].shape), rng.uniform(-3, 3, e["X0"].shape)
        B[:, (j + 1) % KMAX] = 0.0  # (one of the others breaks down at once)
        X0[:, (j + 1) % KMAX] = 0.0
        B[:, j], X0[:, j] = e["B"][:, j], e["X0"][:, j]
        run = run_mbi(ctx, e, pc, inner, B, X0)[0]
        assert run["iters"][j] == full["iters"][j] and run["conv"][j] == full["conv"][j], (name, pc, j)
        assert same_bits(run["hist"][j], full["hist"][j]) and same_bits(run["X"][:, j], full["X"][:, j]), (name, pc, j)
        other = (j + 2) % KMAX
        assert not same_bits(run["hist"][other][:2], full["hist"][other][:2])


@pytest.mark.parametrize("pc,inner", [("none", 0), ("sgs", 0), ("ilu0", 0), ("ilu0it", 3)])
@pytest.mark.parametrize("name", MATS)
def test_freeze_and_determinism(ctx, systems, name, pc, inner):
    e = systems[name]
    k = KMAX
    full = mbi_ref(ctx, e, pc, inner, k)
    again = run_mbi(ctx, e, pc, inner, e["B"], e["X0"])[0]  # two runs, the same bits
    assert again["iters"] == full["iters"] and again["conv"] == full["conv"] and same_bits(again["X"], full["X"])
    for j in range(k):
        assert same_bits(again["hist"][j], full["hist"][j]), j
    # the column that stops first: its X and history do not move during 20 further iterations (the others go on)
    first = int(np.argmin(full["iters"]))
    it0 = full["iters"][first]
    # (an exact or nearly exact preconditioner stops all eight columns in the same iteration -- nsband1921 with ILU(0): 1,
    # with ilu0it: 3, anderson with SGS: 5 -- and then no column is left to advance; without a preconditioner every matrix
    # here has columns that go on, and there the advance is asserted)
    others_go_on = max(full["iters"]) > it0
    assert others_go_on or pc != "none", f"every column stopped at iteration {it0}: the freeze is not exercised"
    at, later = run_mbi(ctx, e, pc, inner, e["B"], e["X0"], steps=(it0, 20))
    assert at["iters"][first] == it0 and later["iters"][first] == it0 and later["conv"][first] == at["conv"][first]
    assert same_bits(later["X"][:, first], at["X"][:, first]) and same_bits(later["hist"][first], at["hist"][first])
    assert same_bits(at["X"][:, first], full["X"][:, first])
    if others_go_on:
        assert max(later["iters"]) > it0, "no other column advanced: the freeze was not exercised"
    # ... and when every column has stopped nothing moves at all
    done, after = run_mbi(ctx, e, pc, inner, e["B"], e["X0"], steps=(ITERS, 20))
    assert after["iters"] == done["iters"] and same_bits(after["X"], done["X"]) and same_bits(done["X"], full["X"])
    for j in range(k):
        assert same_bits(after["hist"][j], done["hist"][j]), j


@pytest.mark.parametrize("pc,inner", [("none", 0), ("ilu0", 0)])
@pytest.mark.parametrize("name", ["hpcg", "nsband1921"])
def test_breakdown_column_stops_alone(ctx, systems, name, pc, inner):
    """b_j = 0 with x0_j = 0: r0 = 0, alpha = 0 / 0 -- iteration 1, not converged, as bis_mcg pins it for bis_cg
    (tests/test_gpu_mcg.py); the other columns converge with the bits they have without it."""
    e = systems[name]
    k = 4
    base = mbi_ref(ctx, e, pc, inner, k)
    B, X0 = e["B"][:, :k].copy(), e["X0"][:, :k].copy()
    B[:, 2] = 0.0
    X0[:, 2] = 0.0
    run = run_mbi(ctx, e, pc, inner, B, X0)[0]
    single = run_single(ctx, e, pc, inner, B[:, 2].copy(), X0[:, 2].copy())
    assert (single["iters"], single["conv"]) == (1, False)
    assert (run["iters"][2], run["conv"][2]) == (1, False) and run["r0"][2] == 0.0
    assert np.array_equal(run["hist"][2], single["hist"], equal_nan=True) and np.isnan(run["hist"][2][1])
    for j in (0, 1, 3):
        assert run["conv"][j] and run["iters"][j] == base["iters"][j], j
        assert same_bits(run["hist"][j], base["hist"][j]) and same_bits(run["X"][:, j], base["X"][:, j]), j


def test_set_preconditioner_checks(ctx, systems):
    from basic_iterative_solvers_amd import BisError
    e = systems["nsband1921"]
    k = 3
    dB, dX = ctx.upload(e["B"][:, :k].ravel()), ctx.upload(e["X0"][:, :k].ravel())
    m = ctx.mbicgstab(e["dA"], dB, dX, k)
    for pc in ("2st", "s2st"):
        with pytest.raises(BisError, match="status 6"):  # BIS_ERR_UNSUPPORTED
            m.set_preconditioner(pc, Ls=e["Ls"], Us=e["Us"], A_D=e["D"], A_D_inv=e["Dinv"], inner=2)
    with pytest.raises(BisError, match="status 6"):
        m.set_preconditioner("sgs", **pc_args(e, "sgs", 0), outer=2)
    with pytest.raises(BisError, match="status 2"):  # an operand the type reads is missing: refused here, not at init
        m.set_preconditioner("gs", A_D=e["D"])
    with pytest.raises(BisError, match="status 2"):
        m.set_preconditioner("sgs", Ls=e["Ls"], Us=e["Us"])
    m.set_preconditioner("sgs", **pc_args(e, "sgs", 0))
    m.init(TOL)
    with pytest.raises(BisError, match="status 2"):  # BIS_ERR_INVALID after bis_mbicgstab_init
        m.set_preconditioner("ilu0", **pc_args(e, "ilu0", 0))
    m.free()
    for bad_k in (0, 9):
        with pytest.raises(BisError, match="status 2"):
            ctx.mbicgstab(e["dA"], dB, dX, bad_k)
    dB.free(); dX.free()
