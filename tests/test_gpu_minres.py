"""GPU: bis_minres_* (preconditioned MINRES for symmetric, possibly indefinite matrices, a device schedule) against a
single-column MINRES loop made of the library's single-vector calls (spmv, dot, sum_vectors / subtract_vectors, scale,
apply_preconditioner) with the scalar algebra in numpy; the loop runs none of bis_minres_*.  Both sides share the SpMV and
the preconditioner apply; the handle's fused dots keep bis_dot's order of the sums, so the two agree bit for bit (printed,
not asserted: the gates below are what is held).  On the smallest input a pure numpy restatement with a
host SpMV ties the loop to an independent implementation at the same gate.

Indefinite matrices are H - sigma I, made on the host from a downloaded generator matrix; preconditioner operands come from
the unshifted H or from the shift = 9 Anderson matrix, so M is symmetric positive definite while A is not.  tol 1e-8,
x0 = 0, b uniform in [-1, 1] from default_rng(3).

Gates.  The nine well-conditioned rows: the project's history gate for CG and GMRES, 1e-10 r0 over the whole history,
`converged` and the iteration counts equal.  The two rows that are sensitive to the order of the sums (several eigenvalues
at +-0.05 .. 0.17: the restatement itself moves by 1e-7 .. 7e-7 r0 between np.dot, long double sums and sums in blocks of
256): the first 40 entries at 1e-10 r0, the whole history within ten times the largest deviation the restatement shows
between its three sum orders on that input (measured here on the host and printed; the margin is for the device's fourth
order), never more than the BiCGSTAB gate 1e-4 r0, and the counts within +-2.

Each test prints what it measured before it asserts."""
import numpy as np
import pytest

from helpers import HIST_TOL, OptionScope, hist_dev
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

TOL = 1e-8
ITERS = 300
GATE = HIST_TOL["cg"]


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


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def shifted(A, sigma):
    """A - sigma I on the host (every row of the generator matrices holds its diagonal entry)."""
    rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
    val = A.val.copy()
    diag = rows == A.col
    assert np.count_nonzero(diag) == A.n_rows
    val[diag] -= sigma
    return CRS(A.n_rows, A.row_ptr, A.col, val)


# ---- the numpy restatement ---------------------------------------------------------------------------------------------
def dot_np(a, b):
    return np.float64(np.dot(a, b))


def dot_long(a, b):
    return np.float64(np.sum(a.astype(np.longdouble) * b.astype(np.longdouble)))


def dot_blocks(a, b):
    s = np.float64(0.0)
    for i in range(0, len(a), 256):
        s = s + np.float64(np.dot(a[i:i + 256], b[i:i + 256]))
    return s


def np_minres(A, b, dot=dot_np, Dinv=None, iters=ITERS, tol=TOL):
    """The iteration of include/bis_hip.h, line by line, on the host (M = diag(1 / Dinv) or none)."""
    n = A.n_rows
    with np.errstate(all="ignore"):
        x = np.zeros(n)
        r1 = b - host_spmv(A, x)
        y = r1 * Dinv if Dinv is not None else r1.copy()
        beta1 = np.sqrt(dot(r1, y))
        r2 = r1.copy()
        w, w2 = np.zeros(n), np.zeros(n)
        oldb, beta, dbar, epsln, phibar, cs, sn = np.float64(0), beta1, np.float64(0), np.float64(0), beta1, np.float64(-1), np.float64(0)
        hist, true, conv, k = [beta1], [np.linalg.norm(b - host_spmv(A, x))], False, 0
        while k < iters:
            k += 1
            v = y * (1.0 / beta)
            y = host_spmv(A, v)
            if k >= 2:
                y = y - (beta / oldb) * r1
            alpha = dot(v, y)
            y = y - (alpha / beta) * r2
            r1, r2 = r2, y
            y = r2 * Dinv if Dinv is not None else r2
            oldb, beta = beta, np.sqrt(dot(r2, y))
            oldeps, delta, gbar = epsln, cs * dbar + sn * alpha, sn * dbar - cs * alpha
            epsln, dbar = sn * beta, -cs * beta
            gamma = np.sqrt(gbar * gbar + beta * beta)
            cs, sn = gbar / gamma, beta / gamma
            phi, phibar = cs * phibar, sn * phibar
            w1, w2 = w2, w
            w = (v - oldeps * w1 - delta * w2) * (1.0 / gamma)
            x = x + phi * w
            hist.append(phibar)
            true.append(np.linalg.norm(b - host_spmv(A, x)))
            if phibar < tol * beta1:
                conv = True
                break
            if not np.isfinite(phibar):
                break
    return dict(iters=k, conv=conv, hist=np.array(hist), x=x, true=np.array(true))


# ---- systems -----------------------------------------------------------------------------------------------------------
GENERATORS = dict(and12s7=lambda c: c.gen_anderson(12, shift=7.0), fem=lambda c: c.gen_fem(6, 6, 6), hpcg=lambda c: c.gen_hpcg(16, 12, 10),
                  and10=lambda c: c.gen_anderson(10, shift=6.5), and10s9=lambda c: c.gen_anderson(10, shift=9.0),
                  and8s6=lambda c: c.gen_anderson(8, shift=6.0), hpcg975=lambda c: c.gen_hpcg(9, 7, 5),
                  one=lambda c: c.matrix(CRS(1, np.array([0, 1], dtype=np.int64), np.zeros(1, np.int32), np.array([2.5]))))
# name: (generator, sigma, the matrix the preconditioner's operands come from)
SYSTEMS = {"and12s7": ("and12s7", 0.0, None), "fem": ("fem", 0.0, None), "hpcg-2": ("hpcg", 2.0, "hpcg"), "fem-2": ("fem", 2.0, "fem"),
           "and10": ("and10", 0.0, "and10s9"), "and8s6": ("and8s6", 0.0, None), "hpcg-4": ("hpcg", 4.0, None),
           "hpcg975": ("hpcg975", 0.0, None), "one": ("one", 0.0, None)}
# (system, preconditioner, iterations of the numpy restatement -- printed next to what ran, not asserted)
ROWS9 = [("and12s7", "none", 43), ("fem", "none", 35), ("hpcg-2", "none", 52), ("hpcg-2", "sgs", 25), ("fem-2", "none", 46),
         ("fem-2", "sgs", 19), ("and10", "none", 78), ("and10", "j", 72), ("and10", "sgs", 38)]
ROWS2 = [("and8s6", 102), ("hpcg-4", 84)]
UNPRECONDITIONED = [r[0] for r in ROWS9 if r[1] == "none"] + [r[0] for r in ROWS2]


class Cache:
    def __init__(self, ctx):
        self.ctx, self.gen, self.sys, self.ops, self.refs, self.runs, self.mgs = ctx, {}, {}, {}, {}, {}, {}

    def generator(self, name):
        if name not in self.gen:
            self.gen[name] = GENERATORS[name](self.ctx)
        return self.gen[name]

    def system(self, name):
        if name not in self.sys:
            gen, sigma, src = SYSTEMS[name]
            dG = self.generator(gen)
            G = CRS(dG.n_rows, *dG.download())
            A = shifted(G, sigma) if sigma else G
            dA = self.ctx.matrix(A) if sigma else dG
            b = np.random.default_rng(3).uniform(-1, 1, A.n_rows)
            self.sys[name] = dict(name=name, dA=dA, A=A, n=A.n_rows, b=b, src=src)
        return self.sys[name]

    def operands(self, src):
        if src not in self.ops:
            dH = self.generator(src)
            Ls, Us, D, Dinv = self.ctx.split_strict(dH)
            self.ops[src] = dict(dH=dH, Ls=Ls, Us=Us, D=D, Dinv=Dinv)
        return self.ops[src]

    def hierarchy(self, src, cycle):
        if (src, cycle) not in self.mgs:
            self.mgs[(src, cycle)] = self.ctx.mg(self.generator(src), cycle=cycle, coarse_limit=30)
        return self.mgs[(src, cycle)]

    def precond(self, e, pc):
        """(keyword arguments of MINRES.set_preconditioner, the type for Context.apply_preconditioner, its six operands, inner)"""
        if pc == "none":
            return None, None, None, 0
        o = self.operands(e["src"])
        ctx, inner = self.ctx, 0
        if pc in ("j", "sgs"):
            kw = dict(Ls=o["Ls"], Us=o["Us"], A_D=o["D"], A_D_inv=o["Dinv"], L_D=o["D"], U_D=o["D"])
            typ = pc
        elif pc == "ilu0it":
            if "ilu" not in o:
                iLs, iLD, iUs, iUD = ctx.ilu0(o["dH"])
                iUinv = ctx.alloc(e["n"])
                ctx.elemwise_div_vectors(iUinv, iLD, iUD, n=e["n"])
                o["ilu"] = dict(Ls=iLs, Us=iUs, A_D=iLD, A_D_inv=iUinv, L_D=iLD, U_D=iUD)
            kw, typ, inner = dict(o["ilu"], inner=3), pc, 3
        elif pc == "fsai":
            if "fsai" not in o:
                o["fsai"] = ctx.fsai(o["dH"])
            kw, typ = dict(Ls=o["fsai"][0], Us=o["fsai"][1]), pc
        else:  # mgv, mgw
            kw, typ = dict(Ls=self.hierarchy(e["src"], pc[2:]).operand), "mg"
        ops = (kw.get("Ls"), kw.get("Us"), kw.get("A_D"), kw.get("A_D_inv"), kw.get("L_D"), kw.get("U_D"))
        return kw, typ, ops, inner

    def ref(self, name, pc, iters=ITERS):
        if (name, pc, iters) not in self.refs:
            e = self.system(name)
            self.refs[(name, pc, iters)] = run_ref(self.ctx, e, self.precond(e, pc), iters=iters)
        return self.refs[(name, pc, iters)]

    def run(self, name, pc, iters=ITERS):
        if (name, pc, iters) not in self.runs:
            e = self.system(name)
            self.runs[(name, pc, iters)] = run_mr(self.ctx, e, self.precond(e, pc), steps=(iters,))[0]
        return self.runs[(name, pc, iters)]


@pytest.fixture(scope="module")
def cache(ctx):
    return Cache(ctx)


def run_ref(ctx, e, pcinfo, iters=ITERS, b=None, tol=TOL, x0=None):
    """MINRES from the single-vector calls with host scalars; runs none of bis_minres_*."""
    dA, n = e["dA"], e["n"]
    _, typ, ops, inner = pcinfo
    b = e["b"] if b is None else b
    db, x = ctx.upload(b), ctx.upload(np.zeros(n) if x0 is None else x0)
    names = ("v", "y", "r1", "r2", "t", "w", "w1", "w2", "tmp", "work")
    wk = {q: ctx.alloc(n) for q in names}
    for q in names:
        ctx.init_vector(wk[q], 0.0)
    v, y, r1, r2, t, w, w1, w2 = (wk[q] for q in names[:8])

    def apply(src):
        if not typ:
            return src
        ctx.apply_preconditioner(typ, n, *ops, y, src, wk["tmp"], wk["work"], inner=inner)
        return y

    f = np.float64
    with np.errstate(all="ignore"):
        ctx.spmv(dA, x, t)
        ctx.subtract_vectors(r2, db, t, 1.0)  # r1 = b - A x0; r2 = r1 (r1 is not read at k = 1)
        yv = apply(r2)
        beta1 = np.sqrt(f(ctx.dot(r2, yv)))
        oldb, beta, dbar, epsln, phibar, cs, sn = f(0), beta1, f(0), f(0), beta1, f(-1), f(0)
        hist, conv, k = [beta1], False, 0
        while k < iters:
            k += 1
            ctx.scale(v, yv, float(f(1.0) / beta))
            ctx.spmv(dA, v, t)
            if k >= 2:
                ctx.subtract_vectors(t, t, r1, float(beta / oldb))
            alpha = f(ctx.dot(v, t))
            ctx.subtract_vectors(t, t, r2, float(alpha / beta))
            r1, r2, t = r2, t, r1
            yv = apply(r2)
            oldb, beta = beta, np.sqrt(f(ctx.dot(r2, yv)))
            oldeps, delta, gbar = epsln, cs * dbar + sn * alpha, sn * dbar - cs * alpha
            epsln, dbar = sn * beta, -cs * beta
            gamma = np.sqrt(gbar * gbar + beta * beta)
            cs, sn = gbar / gamma, beta / gamma
            phi, phibar = cs * phibar, sn * phibar
            w1, w2, w = w2, w, w1
            ctx.subtract_vectors(w, v, w1, float(oldeps))
            ctx.subtract_vectors(w, w, w2, float(delta))
            ctx.scale(w, w, float(f(1.0) / gamma))
            ctx.sum_vectors(x, x, w, float(phi))
            hist.append(phibar)
            if phibar < tol * beta1:
                conv = True
                break
            if not np.isfinite(phibar):
                break
    out = dict(iters=k, conv=conv, hist=np.array(hist, dtype=np.float64), x=x.to_host())
    for q in list(wk.values()) + [db, x]:
        q.free()
    return out


def state(s, dx):
    it, conv, hist = s.status()
    return dict(iters=it, conv=conv, hist=hist, x=dx.to_host())


def run_mr(ctx, e, pcinfo, steps=(ITERS,), b=None, mg=None):
    """One solve on the handle; returns the state after each entry of `steps`: n further iterations, or (n, times)."""
    b = e["b"] if b is None else b
    db, dx = ctx.upload(b), ctx.upload(np.zeros(e["n"]))
    s = ctx.minres(e["dA"], db, dx)
    kw, typ, _, _ = pcinfo
    if mg is not None:
        s.set_preconditioner(mg)
    elif typ:
        s.set_preconditioner(typ, **kw)
    r0 = s.init(TOL)
    out = []
    for it in steps:
        for _ in range(it[1]) if isinstance(it, tuple) else (0,):
            s.iterate(it[0] if isinstance(it, tuple) else it)
        out.append(state(s, dx))
        out[-1]["r0"] = r0
    s.free(); db.free(); dx.free()
    return out


def same_state(a, c):
    return a["iters"] == c["iters"] and a["conv"] == c["conv"] and same_bits(a["x"], c["x"]) and same_bits(a["hist"], c["hist"])


def check_against(tag, run, ref, expect=None):
    r0 = ref["hist"][0]
    dev = hist_dev(run["hist"], ref["hist"])
    print(f"{tag}: minres iters {run['iters']} conv {run['conv']}, reference loop iters {ref['iters']} conv {ref['conv']}"
          f"{'' if expect is None else f' (numpy restatement: {expect})'}, hist dev {dev:.3e} r0, r0 {r0:.6e}, same bits in history / x: "
          f"{same_bits(run['hist'], ref['hist'])} / {same_bits(run['x'], ref['x'])}")
    assert dev <= GATE, tag
    assert run["conv"] == ref["conv"], tag
    assert run["iters"] == ref["iters"] and len(run["hist"]) == len(ref["hist"]), tag
    return dev


# ---- 1. the inputs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pc,expect", ROWS9, ids=[f"{r[0]}-{r[1]}" for r in ROWS9])
def test_rows_at_the_history_gate(cache, name, pc, expect):
    run, ref = cache.run(name, pc), cache.ref(name, pc)
    check_against(f"{name} {pc}", run, ref, expect)
    assert run["conv"] and run["hist"][0] == run["r0"]


def order_spread(e):
    """The restatement's own history deviation between its three sum orders, / r0: (whole history, first 40 entries, counts)."""
    runs = [np_minres(e["A"], e["b"], dot=d) for d in (dot_np, dot_long, dot_blocks)]
    pairs = [(0, 1), (0, 2), (1, 2)]
    whole = max(hist_dev(runs[i]["hist"], runs[j]["hist"]) for i, j in pairs)
    head = max(hist_dev(runs[i]["hist"][:41], runs[j]["hist"][:41]) for i, j in pairs)
    return whole, head, [r["iters"] for r in runs], runs[0]


def check_sensitive(tag, run, ref, spread):
    r0 = ref["hist"][0]
    gate = min(10.0 * spread, HIST_TOL["bi"])
    head = hist_dev(run["hist"][:41], ref["hist"][:41])
    dev = hist_dev(run["hist"], ref["hist"])
    print(f"{tag}: iters {run['iters']} conv {run['conv']} against iters {ref['iters']} conv {ref['conv']}; first 40 entries apart "
          f"{head:.3e} r0, whole history {dev:.3e} r0, gate {gate:.3e} r0, r0 {r0:.6e}")
    assert head <= GATE, tag
    assert dev <= gate, tag
    assert run["conv"] and ref["conv"] and abs(run["iters"] - ref["iters"]) <= 2, tag


@pytest.mark.parametrize("name,expect", ROWS2, ids=[r[0] for r in ROWS2])
def test_rows_sensitive_to_the_order_of_the_sums(cache, name, expect):
    e = cache.system(name)
    whole, head, counts, _ = order_spread(e)
    print(f"{name}: the restatement between np.dot, long double and blocks of 256: whole history {whole:.3e} r0, first 40 entries "
          f"{head:.3e} r0, iterations {counts} (recorded: {expect})")
    check_sensitive(f"{name} none, handle against the reference loop", cache.run(name, "none"), cache.ref(name, "none"), whole)


def test_numpy_restatement_on_the_smallest_input(cache):
    """The reference loop against an implementation that shares nothing with the library, at that input's gate."""
    name = min((r[0] for r in ROWS9 + ROWS2), key=lambda q: cache.system(q)["n"])
    e = cache.system(name)
    assert name == "and8s6" and e["n"] == 512
    whole, _, counts, host = order_spread(e)
    print(f"{name}: n = {e['n']}, restatement spread {whole:.3e} r0, iterations {counts}; its largest |true - estimate| "
          f"{np.max(np.abs(host['true'] - host['hist'])) / host['hist'][0]:.3e} r0")
    check_sensitive(f"{name}: reference loop against the numpy restatement", cache.ref(name, "none"), host, whole)
    check_sensitive(f"{name}: handle against the numpy restatement", cache.run(name, "none"), host, whole)


# ---- 2. more shapes ------------------------------------------------------------------------------------------------------
def test_one_row(cache):
    e = cache.system("one")
    run = run_mr(cache.ctx, e, cache.precond(e, "none"), b=np.array([3.0]))[0]
    print(f"one row: {run['iters']} {run['conv']} {run['hist']} x {run['x']}")
    assert (run["iters"], run["conv"]) == (1, True) and len(run["hist"]) == 2
    assert run["hist"][0] == 3.0 and run["hist"][1] < TOL * 3.0
    assert abs(3.0 - 2.5 * run["x"][0]) <= 1e-10 * 3.0


def test_odd_size_with_vector_tails(cache):
    e = cache.system("hpcg975")
    assert e["n"] == 315
    check_against("hpcg 9x7x5", cache.run("hpcg975", "none"), cache.ref("hpcg975", "none"))
    assert cache.run("hpcg975", "none")["conv"]


@pytest.mark.parametrize("rp64", [0, 1])
def test_many_workgroups(ctx, rp64):
    """n = 122880: 240 workgroups in the passes that reduce; 10 iterations; also with 64-bit row pointers."""
    with OptionScope(ctx, **({"force_rp64": 1} if rp64 else {})):
        dA = ctx.gen_hpcg(64, 48, 40)
        assert dA.n_rows == 122880 and dA.rp_width == (8 if rp64 else 4)
        e = dict(dA=dA, n=dA.n_rows, b=np.random.default_rng(3).uniform(-1, 1, dA.n_rows))
        none = (None, None, None, 0)
        run, ref = run_mr(ctx, e, none, steps=(10,))[0], run_ref(ctx, e, none, iters=10)
        dA.free()
    check_against(f"hpcg 64x48x40 rp64={rp64}, 10 iterations", run, ref)
    assert run["iters"] == 10 and not run["conv"]
    dx = np.max(np.abs(run["x"] - ref["x"])) / np.max(np.abs(ref["x"]))
    print(f"x apart {dx:.3e} of max |x|")
    assert dx <= 1e-12


# ---- 3. preconditioner types ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", ["j", "sgs", "fsai", "ilu0it", "mgv", "mgw"])
def test_preconditioner_types(cache, pc):
    run, ref = cache.run("hpcg-2", pc), cache.ref("hpcg-2", pc)
    check_against(f"hpcg-2 {pc}", run, ref)
    assert run["conv"]
    assert np.all(np.diff(run["hist"]) <= 0.0)  # phibar = sn phibar with 0 <= sn <= 1
    if pc.startswith("mg"):
        mg = cache.hierarchy("hpcg", pc[2:])
        assert mg.levels >= 2
        e = cache.system("hpcg-2")
        obj = run_mr(cache.ctx, e, cache.precond(e, "none"), mg=mg)[0]
        assert same_state(obj, run)  # the MG object and its operand are the same preconditioner


def test_v_and_w_cycles_are_different_operators(cache):
    assert not same_bits(cache.run("hpcg-2", "mgv")["hist"][:3], cache.run("hpcg-2", "mgw")["hist"][:3])


# ---- 4. invariants -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", UNPRECONDITIONED)
def test_history_is_the_true_residual_and_never_rises(cache, name):
    ctx, e = cache.ctx, cache.system(name)
    n, full = e["n"], cache.run(name, "none")
    db, dx, t, r = ctx.upload(e["b"]), ctx.upload(np.zeros(n)), ctx.alloc(n), ctx.alloc(n)
    s = ctx.minres(e["dA"], db, dx)
    r0 = s.init(TOL)
    true = []
    for _ in range(full["iters"] + 1):
        ctx.spmv(e["dA"], dx, t)
        ctx.subtract_vectors(r, db, t, 1.0)
        true.append(ctx.euclidean_vec_norm(r))
        s.iterate(1)
    it, conv, hist = s.status()
    x = dx.to_host()
    s.free()
    for q in (db, dx, t, r):
        q.free()
    true = np.array(true)
    gap = np.max(np.abs(true - hist)) / r0
    rise = np.max(np.diff(true)) / r0
    print(f"{name}: {it} iterations, largest |true - estimate| {gap:.3e} r0, largest rise of the true residual {rise:.3e} r0, "
          f"largest rise of the history {np.max(np.diff(hist)) / r0:.3e} r0")
    assert it == full["iters"] and conv and same_bits(hist, full["hist"]) and same_bits(x, full["x"])  # iterate(1) x iters = iterate(300)
    assert hist[0] == r0  # entry 0 is what init returned
    assert np.all(np.diff(hist) <= 0.0)
    assert gap <= 1e-12
    assert rise <= 1e-12
    assert hist[-1] < TOL * r0 and np.all(hist[:-1] >= TOL * r0)  # the stop fired at the first entry below the threshold


SCHEDULE = [("and10", "none"), ("and8s6", "none"), ("hpcg-2", "sgs"), ("and10", "j")]


@pytest.mark.parametrize("name,pc", SCHEDULE, ids=[f"{c[0]}-{c[1]}" for c in SCHEDULE])
def test_schedule_properties(cache, name, pc):
    ctx, e = cache.ctx, cache.system(name)
    info = cache.precond(e, pc)
    full = cache.run(name, pc)
    assert full["conv"]
    again = run_mr(ctx, e, info)[0]  # a second solve on a fresh handle
    assert same_state(again, full)
    split = run_mr(ctx, e, info, steps=((1, ITERS),))[0]  # 300 x iterate(1)
    assert same_state(split, full)
    done, after = run_mr(ctx, e, info, steps=(ITERS, 20))  # 20 more iterations after the stop change nothing
    assert same_state(done, full) and same_state(after, done)


# ---- 5. edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", ["none", "sgs"])
def test_zero_right_hand_side_from_zero(cache, pc):
    e = cache.system("hpcg-2")
    run, later = run_mr(cache.ctx, e, cache.precond(e, pc), steps=(ITERS, 5), b=np.zeros(e["n"]))
    print(f"zero rhs {pc}: iters {run['iters']} conv {run['conv']} hist {run['hist']}")
    assert (run["iters"], run["conv"], run["r0"]) == (1, False, 0.0)
    assert len(run["hist"]) == 2 and run["hist"][0] == 0.0 and np.isnan(run["hist"][1])
    assert later["iters"] == 1 and not later["conv"] and len(later["hist"]) == 2


def test_a_negative_definite_preconditioner_stops_the_solve(cache):
    """M = -I handed in as Jacobi with D = -1: (r, M^-1 r) < 0, its root is NaN"""
    ctx, e = cache.ctx, cache.system("and10")
    D = ctx.upload(np.full(e["n"], -1.0))
    run = run_mr(ctx, e, (dict(A_D=D), "j", None, 0))[0]
    D.free()
    print(f"M = -I: iters {run['iters']} conv {run['conv']} hist {run['hist']}")
    assert run["iters"] == 1 and not run["conv"]
    assert len(run["hist"]) == 2 and np.isnan(run["hist"][1])


def test_a_jacobi_diagonal_off_a_16_byte_boundary(cache):
    """The fused Jacobi pass reads D 16 bytes per lane; a D at 8 mod 16 takes the apply and the dot pass: the same bits.
    b or x off the boundary is refused."""
    import ctypes as C
    ctx, e = cache.ctx, cache.system("and10")
    n, full = e["n"], cache.run("and10", "j")
    big = ctx.alloc(n + 2)
    D = big.offset(1, n)
    assert D.ptr % 16 == 8
    ctx.copy_vector(D, cache.operands("and10s9")["D"], n=n)
    run = run_mr(ctx, e, (dict(A_D=D), "j", None, 0))[0]
    print(f"and10 j, D at 8 mod 16: {run['iters']} iterations, aligned {full['iters']}")
    assert same_state(run, full)
    h = C.c_void_p()
    for pb, px in ((big.offset(1, n), big), (big, big.offset(1, n))):
        assert ctx.lib.bis_minres_create(ctx.h, e["dA"].h, C.c_void_p(pb.ptr), C.c_void_p(px.ptr), C.byref(h)) == 2 and not h
    big.free()


def test_no_rows(ctx):
    dA = ctx.matrix(CRS(0, np.zeros(1, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0)))
    db, dx = ctx.alloc(2), ctx.alloc(2)
    s = ctx.minres(dA, db, dx)
    s.set_preconditioner("j")
    assert s.init(TOL) == 0.0
    s.iterate(7)
    it, conv, hist = s.status()
    assert (it, conv) == (0, False)
    s.free()
    db.free(); dx.free(); dA.free()


def test_argument_checks(cache):
    import ctypes as C

    from basic_iterative_solvers_amd import BisError
    ctx, e = cache.ctx, cache.system("hpcg-2")
    o = cache.operands("hpcg")
    db, dx = ctx.upload(e["b"]), ctx.upload(np.zeros(e["n"]))
    lib, pb, px = ctx.lib, C.c_void_p(db.ptr), C.c_void_p(dx.ptr)
    for args in ((None, pb, px), (e["dA"].h, None, px), (e["dA"].h, pb, None)):
        h = C.c_void_p()
        assert lib.bis_minres_create(ctx.h, *args, C.byref(h)) == 2 and not h
    assert lib.bis_minres_create(ctx.h, e["dA"].h, pb, px, None) == 2
    rect = ctx.matrix(CRS(2, np.array([0, 1, 2], dtype=np.int64), np.array([0, 2], np.int32), np.array([1.0, 1.0]), n_cols=3))
    h = C.c_void_p()
    assert lib.bis_minres_create(ctx.h, rect.h, pb, px, C.byref(h)) == 2 and not h
    rect.free()
    for call in (lambda: lib.bis_minres_init(ctx.h, None, C.c_double(TOL), None), lambda: lib.bis_minres_iterate(ctx.h, None, C.c_int(1)),
                 lambda: lib.bis_minres_status(ctx.h, None, None, None, None, C.c_int(0)),
                 lambda: lib.bis_minres_set_preconditioner(ctx.h, None, C.c_int(1), None, None, None, None, None, None, C.c_int(1), C.c_int(0))):
        assert call() == 2
    s = ctx.minres(e["dA"], db, dx)
    with pytest.raises(BisError, match="status 2"):  # iterate before init
        s.iterate(1)
    with pytest.raises(BisError, match="status 2"):  # a missing operand: refused here, not inside iterate
        s.set_preconditioner("sgs", Ls=o["Ls"], Us=o["Us"])
    with pytest.raises(BisError, match="status 2"):
        s.set_preconditioner("j")
    with pytest.raises(BisError, match="status 2"):
        s.set_preconditioner("fsai", Ls=o["Ls"])
    with pytest.raises(BisError, match="status 2"):  # outer_iters = 0, as bis_apply_preconditioner
        s.set_preconditioner("j", A_D=o["D"], outer=0)
    with pytest.raises(BisError, match="status 2"):  # an MG operand of another size
        s.set_preconditioner("mg", Ls=cache.hierarchy("fem", "v").operand)
    with pytest.raises(BisError, match="status 2"):  # "mg" with something that is no hierarchy's operand
        s.set_preconditioner("mg", Ls=o["Ls"])
    with pytest.raises(BisError, match="status 6"):  # BIS_ERR_UNSUPPORTED, as bis_apply_preconditioner
        s.set_preconditioner("mg", Ls=cache.hierarchy("hpcg", "v").operand, outer=2)
    s.set_preconditioner("sgs", **cache.precond(e, "sgs")[0])
    s.init(TOL)
    with pytest.raises(BisError, match="status 2"):  # BIS_ERR_INVALID after bis_minres_init
        s.set_preconditioner("j", A_D=o["D"])
    s.iterate(ITERS)
    it, conv, hist = s.status()
    assert conv and same_bits(hist, cache.run("hpcg-2", "sgs")["hist"])
    s.free()
    db.free(); dx.free()
