"""GPU: bis_mcg_* with a general preconditioner (bis_mcg_set_preconditioner: SGS, ILU(0), iterative ILU(0)) against
bis_cg_set_preconditioner + bis_cg column by column, the freeze of a stopped column, determinism, the argument checks, and
the None / Jacobi schedule left as it was.

The multi-vector sweeps are bit-identical to the single-vector ones (tests/test_gpu_sptrsm.py), so only the reduction
tree differs between MCG and CG, exactly as without a preconditioner: the gate is tests/test_gpu_mcg.py's, no new number."""
import numpy as np
import pytest

from helpers import HIST_TOL, hist_dev
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

TOL = 1e-8
ITERS = 300
KMAX = 8
PCS = [("sgs", 0), ("ilu0", 0), ("ilu0it", 3)]


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
    """keyword arguments of CG.set_preconditioner / MCG.set_preconditioner for this type"""
    if pc == "sgs":
        return dict(Ls=e["Ls"], Us=e["Us"], A_D=e["D"], A_D_inv=e["Dinv"], L_D=e["D"], U_D=e["D"])
    return dict(Ls=e["iLs"], Us=e["iUs"], A_D=e["iLD"], A_D_inv=e["iUinv"], L_D=e["iLD"], U_D=e["iUD"], inner=inner)


def run_cg(ctx, e, pc, inner, b, x0):
    db, dx = ctx.upload(b), ctx.upload(x0)
    cg = ctx.cg(e["dA"], db, dx)
    cg.set_preconditioner(pc, **pc_args(e, pc, inner))
    r0 = cg.init(TOL)
    cg.iterate(ITERS)
    iters, conv, hist = cg.status()
    x = dx.to_host()
    cg.free(); db.free(); dx.free()
    return dict(iters=iters, conv=conv, hist=hist, x=x, r0=r0)


def mcg_state(m, dX, n, k):
    st = [m.status(j) for j in range(k)]
    return dict(iters=[s[0] for s in st], conv=[s[1] for s in st], hist=[s[2] for s in st], X=dX.to_host().reshape(n, k))


def run_mcg(ctx, e, pc, inner, B, X0, A_D=None, steps=(ITERS,)):
    """One MCG solve; pc None: no set_preconditioner call.  Returns the state after each entry of `steps` further iterations."""
    n, k = B.shape
    dB, dX = ctx.upload(B.ravel()), ctx.upload(X0.ravel())
    m = ctx.mcg(e["dA"], dB, dX, k, A_D=A_D)
    if pc is not None:
        m.set_preconditioner(pc, **pc_args(e, pc, inner))
    r0 = m.init(TOL)
    out = []
    for s in steps:
        m.iterate(s)
        out.append(mcg_state(m, dX, n, k))
        out[-1]["r0"] = r0
    m.free(); dB.free(); dX.free()
    return out


MATS = ["hpcg", "anderson", "band1921", "fem666"]


@pytest.fixture(scope="module")
def systems(ctx):
    """Per matrix: the operands of every preconditioner type and the 8 columns -- built once, never changed."""
    out = {}
    for name in MATS:
        if name == "hpcg":
            dA = ctx.gen_hpcg(16, 12, 10)
        elif name == "anderson":
            dA = ctx.gen_anderson(14, shift=9.0)
        elif name == "band1921":
            dA = ctx.matrix(spd_band(1921, 3, 1))
        else:
            dA = ctx.gen_fem(6, 6, 6)
        n = dA.n_rows
        A = CRS(n, *dA.download())
        Ls, Us, D, Dinv = ctx.split_strict(dA)
        iLs, iLD, iUs, iUD = ctx.ilu0(dA)
        iUinv = ctx.alloc(n)
        ctx.elemwise_div_vectors(iUinv, iLD, iUD)
        B, X0 = columns(A, KMAX, seed=100 + KMAX)
        out[name] = dict(dA=dA, A=A, n=n, Ls=Ls, Us=Us, D=D, Dinv=Dinv, iLs=iLs, iLD=iLD, iUs=iUs, iUD=iUD, iUinv=iUinv, B=B, X0=X0,
                         cg={}, mcg={})
    return out


def cg_refs(ctx, e, pc, inner):
    """the KMAX single-vector solves of this matrix and type, computed once and shared"""
    key = (pc, inner)
    if key not in e["cg"]:
        e["cg"][key] = [run_cg(ctx, e, pc, inner, e["B"][:, j].copy(), e["X0"][:, j].copy()) for j in range(KMAX)]
    return e["cg"][key]


def mcg_ref(ctx, e, pc, inner, k):
    key = (pc, inner, k)
    if key not in e["mcg"]:
        e["mcg"][key] = run_mcg(ctx, e, pc, inner, e["B"][:, :k].copy(), e["X0"][:, :k].copy())[0]
    return e["mcg"][key]


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


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("pc,inner", PCS)
@pytest.mark.parametrize("name", MATS)
def test_parity_with_preconditioned_cg_column_by_column(ctx, systems, name, pc, inner, k):
    e = systems[name]
    cg = cg_refs(ctx, e, pc, inner)
    run = mcg_ref(ctx, e, pc, inner, k)
    print(f"{name} {pc} k={k}: cg iteration counts {[c['iters'] for c in cg[:k]]}, mcg {run['iters']}")
    for j in range(k):
        check_column(f"{name} {pc} k={k} j={j}", e["A"], e["B"][:, j], run["iters"][j], run["conv"][j], run["hist"][j],
                     run["X"][:, j], cg[j])


@pytest.mark.parametrize("pc,inner", PCS)
@pytest.mark.parametrize("name", MATS)
def test_freeze_and_determinism(ctx, systems, name, pc, inner):
    e = systems[name]
    k = 8
    full = mcg_ref(ctx, e, pc, inner, k)
    again = run_mcg(ctx, e, pc, inner, e["B"], e["X0"])[0]  # two runs, the same bits
    assert again["iters"] == full["iters"] and again["conv"] == full["conv"] and same_bits(again["X"], full["X"])
    for j in range(k):
        assert same_bits(again["hist"][j], full["hist"][j]), j
    # the column that stops first: its X and history do not move during 20 further iterations (the others go on)
    first = int(np.argmin(full["iters"]))
    it0 = full["iters"][first]
    at, later = run_mcg(ctx, e, pc, inner, e["B"], e["X0"], steps=(it0, 20))
    assert at["iters"][first] == it0 and later["iters"][first] == it0 and later["conv"][first] == at["conv"][first]
    assert same_bits(later["X"][:, first], at["X"][:, first]) and same_bits(later["hist"][first], at["hist"][first])
    assert same_bits(at["X"][:, first], full["X"][:, first])
    if max(full["iters"]) > it0:
        assert max(later["iters"]) > it0, "no other column advanced: the freeze was not exercised"
    # ... and when every column has stopped nothing moves at all
    done, after = run_mcg(ctx, e, pc, inner, e["B"], e["X0"], steps=(ITERS, 20))
    assert after["iters"] == done["iters"] and same_bits(after["X"], done["X"]) and same_bits(done["X"], full["X"])


def test_set_preconditioner_checks(ctx, systems):
    from basic_iterative_solvers_amd import BisError
    e = systems["band1921"]
    n, k = e["n"], 3
    dB, dX = ctx.upload(e["B"][:, :k].ravel()), ctx.upload(e["X0"][:, :k].ravel())
    m = ctx.mcg(e["dA"], dB, dX, k)
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
    with pytest.raises(BisError, match="status 2"):  # BIS_ERR_INVALID after bis_mcg_init
        m.set_preconditioner("ilu0", **pc_args(e, "ilu0", 0))
    m.free(); dB.free(); dX.free()


@pytest.mark.parametrize("name", ["hpcg", "anderson"])
def test_none_and_jacobi_schedules_are_unchanged(ctx, systems, name):
    """Without set_preconditioner MCG launches its fused None / Jacobi schedule as before.  The general-preconditioner
    schedule with type NONE / JACOBI performs, per column, the same operations in the same order (the same lanes, the same
    partial sums, the same last-arriver order; only the split of pass B into three launches differs), so the two runs must
    agree bit for bit: a change of either schedule's arithmetic shows here."""
    e = systems[name]
    k = 4
    B, X0 = e["B"][:, :k].copy(), e["X0"][:, :k].copy()
    for pc, A_D in (("none", None), ("j", e["D"])):
        fused = run_mcg(ctx, e, None, 0, B, X0, A_D=A_D)[0]
        dB, dX = ctx.upload(B.ravel()), ctx.upload(X0.ravel())
        m = ctx.mcg(e["dA"], dB, dX, k)
        m.set_preconditioner(pc, A_D=e["D"])
        m.init(TOL)
        m.iterate(ITERS)
        general = mcg_state(m, dX, e["n"], k)
        m.free(); dB.free(); dX.free()
        assert all(fused["conv"]) and fused["iters"] == general["iters"] and fused["conv"] == general["conv"], (name, pc)
        assert same_bits(fused["X"], general["X"]), (name, pc)
        for j in range(k):
            assert same_bits(fused["hist"][j], general["hist"][j]), (name, pc, j)
