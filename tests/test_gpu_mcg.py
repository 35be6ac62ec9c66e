"""GPU: bis_mcg_* (k CG solves in lock-step on one matrix stream) against the existing single-vector CG column by column,
the independence of the columns, the freeze of a stopped column, determinism."""
import numpy as np
import pytest

from helpers import HIST_TOL, hist_dev
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

TOL = 1e-8
ITERS = 300


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


def spd_band(n, half, seed):
    """Random symmetric, strictly diagonally dominant band: SPD."""
    rng = np.random.default_rng(seed)
    off = {d: rng.uniform(-1, 1, n - d) for d in range(1, half + 1)}
    absum = np.zeros(n)
    for d, v in off.items():
        absum[:n - d] += np.abs(v)
        absum[d:] += np.abs(v)
    diag = absum * rng.uniform(1.1, 1.5, n) + 1e-3
    rows, cols, vals = [], [], []
    for r in range(n):
        for d in range(-half, half + 1):
            c = r + d
            if 0 <= c < n:
                rows.append(r); cols.append(c)
                vals.append(diag[r] if d == 0 else off[abs(d)][min(r, c)])
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return CRS(n, rp, np.array(cols, dtype=np.int32), np.array(vals))


def columns(A, k, seed):
    """B, X0 (n x k): b_0 = A 1, b_1 uniform random, b_2 a unit vector, the rest random at the scales 1e-6, 1, 1e6;
    start vectors zero in columns 0, 1, 3, 6 and random in the others."""
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
        if j == 2:  # (its own generator: on the well-conditioned Anderson matrix this start makes column 2 stop an iteration early)
            X0[:, j] = np.random.default_rng(2).uniform(-1, 1, n)
        elif j not in (0, 1, 3, 6):
            X0[:, j] = rng.uniform(-1, 1, n) * scales[(j - 3) % 3]
    return B, X0


def run_cg(ctx, dA, dD, b, x0):
    db, dx = ctx.upload(b), ctx.upload(x0)
    cg = ctx.cg(dA, db, dx, A_D=dD)
    r0 = cg.init(TOL)
    cg.iterate(ITERS)
    iters, conv, hist = cg.status()
    x = dx.to_host()
    cg.free(); db.free(); dx.free()
    return dict(iters=iters, conv=conv, hist=hist, x=x, r0=r0)


def run_mcg(ctx, dA, dD, B, X0, extra=0):
    n, k = B.shape
    dB, dX = ctx.upload(B.ravel()), ctx.upload(X0.ravel())
    m = ctx.mcg(dA, dB, dX, k, A_D=dD)
    r0 = m.init(TOL)
    m.iterate(ITERS)
    st = [m.status(j) for j in range(k)]
    out = dict(r0=r0, iters=[s[0] for s in st], conv=[s[1] for s in st], hist=[s[2] for s in st], X=dX.to_host().reshape(n, k))
    if extra:
        m.iterate(extra)
        st = [m.status(j) for j in range(k)]
        out["after"] = dict(iters=[s[0] for s in st], conv=[s[1] for s in st], hist=[s[2] for s in st], X=dX.to_host().reshape(n, k))
    m.free(); dB.free(); dX.free()
    return out


MATS = ["hpcg", "anderson_jacobi", "band1921"]


@pytest.fixture(scope="module")
def solves(ctx):
    """Per matrix: device matrix, host CRS, Jacobi diagonal or None, and per k the columns, the k single CG solves and the
    MCG run -- computed once, shared by the tests below, never changed."""
    out = {}
    for name in MATS:
        if name == "hpcg":
            dA = ctx.gen_hpcg(16, 12, 10)
        elif name == "anderson_jacobi":
            dA = ctx.gen_anderson(14, shift=9.0)
        else:
            dA = ctx.matrix(spd_band(1921, 3, 1))
        rp, col, val = dA.download()
        A = CRS(dA.n_rows, rp, col, val)
        dD = ctx.mat_diag(dA)[0] if name == "anderson_jacobi" else None
        e = dict(dA=dA, A=A, dD=dD)
        for k in (4, 7):
            B, X0 = columns(A, k, seed=100 + k)
            e[k] = dict(B=B, X0=X0, cg=[run_cg(ctx, dA, dD, B[:, j].copy(), X0[:, j].copy()) for j in range(k)],
                        mcg=run_mcg(ctx, dA, dD, B, X0))
        out[name] = e
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_column(tag, A, b, m_iters, m_conv, m_hist, m_x, cg):
    print(f"{tag}: mcg iters {m_iters} conv {m_conv}, cg iters {cg['iters']} conv {cg['conv']}, "
          f"hist dev {hist_dev(m_hist, cg['hist']):.3e}")
    assert hist_dev(m_hist, cg["hist"]) <= HIST_TOL["cg"], tag
    assert abs(m_iters - cg["iters"]) <= 2 and m_conv == cg["conv"], tag
    res = np.linalg.norm(b - host_spmv(A, m_x))
    print(f"{tag}: true residual {res:.6e}, last history entry {m_hist[-1]:.6e}, r0 {m_hist[0]:.6e}")
    assert res <= m_hist[-1] + 1e-10 * m_hist[0], tag


@pytest.mark.parametrize("k", [4, 7])
@pytest.mark.parametrize("name", MATS)
def test_parity_with_cg_column_by_column(solves, name, k):
    """Iteration counts of the single-vector CG (tol 1e-8), columns 0 .. k-1 -- at least two distinct counts per case, so
    that some column freezes while others go on:
    (filled in from the measured run, see the table in docs/EXPERIMENTS.md section 18)"""
    e = solves[name]
    s = e[k]
    cg_counts = [c["iters"] for c in s["cg"]]
    print(f"{name} k={k}: cg iteration counts {cg_counts}, mcg {s['mcg']['iters']}")
    assert len(set(cg_counts)) >= 2, cg_counts
    for j in range(k):
        check_column(f"{name} k={k} j={j}", e["A"], s["B"][:, j], s["mcg"]["iters"][j], s["mcg"]["conv"][j], s["mcg"]["hist"][j],
                     s["mcg"]["X"][:, j], s["cg"][j])
    assert len(set(s["mcg"]["iters"])) >= 2, "every column stopped in the same iteration: the freeze path did not run"
    assert all(s["mcg"]["conv"])


@pytest.mark.parametrize("name", MATS)
def test_independence_freeze_and_determinism(ctx, solves, name):
    e = solves[name]
    k = 4
    s = e[k]
    B, X0 = s["B"].copy(), s["X0"].copy()
    B[:, 2] = 0.0
    X0[:, 2] = 0.0
    run = run_mcg(ctx, e["dA"], e["dD"], B, X0, extra=50)
    zero = run_cg(ctx, e["dA"], e["dD"], B[:, 2].copy(), X0[:, 2].copy())  # r0 = 0: iteration 1, not converged, through 0/0
    assert (zero["iters"], zero["conv"]) == (1, False)
    assert (run["iters"][2], run["conv"][2]) == (zero["iters"], zero["conv"]) and run["r0"][2] == 0.0
    assert np.array_equal(run["hist"][2], zero["hist"], equal_nan=True)
    for j in (0, 1, 3):  # the other columns: not a bit differs from the run with the original column 2
        assert same_bits(run["hist"][j], s["mcg"]["hist"][j]), j
        assert same_bits(run["X"][:, j], s["mcg"]["X"][:, j]), j
        assert run["iters"][j] == s["mcg"]["iters"][j] and run["conv"][j] == s["mcg"]["conv"][j]
    after = run["after"]  # 50 more iterations after every column has stopped: nothing moves
    assert after["iters"] == run["iters"] and after["conv"] == run["conv"]
    assert same_bits(after["X"], run["X"])
    for j in range(k):
        assert same_bits(after["hist"][j], run["hist"][j]), j
    again = run_mcg(ctx, e["dA"], e["dD"], s["B"], s["X0"])  # the reductions are deterministic
    assert again["iters"] == s["mcg"]["iters"] and same_bits(again["X"], s["mcg"]["X"])
    for j in range(k):
        assert same_bits(again["hist"][j], s["mcg"]["hist"][j]), j


@pytest.mark.parametrize("name", MATS)
def test_single_column(ctx, solves, name):
    e = solves[name]
    s = e[4]
    one = run_mcg(ctx, e["dA"], e["dD"], s["B"][:, 1:2].copy(), s["X0"][:, 1:2].copy())  # k = 1: the SpMM is bis_spmv
    check_column(f"{name} k=1", e["A"], s["B"][:, 1], one["iters"][0], one["conv"][0], one["hist"][0], one["X"][:, 0], s["cg"][1])


def test_changing_one_column_changes_no_other(ctx, solves):
    e = solves["hpcg"]
    s = e[4]
    B = s["B"].copy()
    B[:, 3] = np.random.default_rng(9).uniform(-3, 3, B.shape[0])
    run = run_mcg(ctx, e["dA"], e["dD"], B, s["X0"])
    assert not same_bits(run["hist"][3][:2], s["mcg"]["hist"][3][:2])
    for j in (0, 1, 2):
        assert same_bits(run["hist"][j], s["mcg"]["hist"][j]), j
        assert same_bits(run["X"][:, j], s["mcg"]["X"][:, j]), j
