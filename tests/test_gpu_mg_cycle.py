"""GPU: the W- and K-cycles of the aggregation multigrid hierarchy (bis_mg_set_cycle) against a numpy restatement of the
definitions in include/bis_hip.h, on the hierarchy downloaded from the device (test_gpu_mg.py proves matrices, aggregates
and weights bit for bit): the apply to 1e-13 |.|_inf (the project's kernel gate), the bit-for-bit promises (two applies,
aliasing, the dispatcher, V restored, two levels, cycle_levels past the hierarchy), the guards (in = 0), W as a fixed SPD
operator, the error table, and the solves: fused CG with V, W and K against a numpy PCG using the restated cycle, and the
call-by-call BiCGSTAB with the GCR K-cycle on an unstructured input.

Reference: `cycle_reference` below.  It is test_gpu_mg.py's V-cycle with the coarse solve replaced as the header states; the
SpMV row sums and the K step's dot products are taken in np.longdouble and rounded once."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_mg as base
from helpers import HIST_TOL, OptionScope, hist_dev

pytestmark = pytest.mark.gpu

LD = np.longdouble
GATE = 1e-13
INVALID, UNSUPPORTED = 2, 6
V, W, K, KGCR = 0, 1, 2, 3
NAMES = {V: "V", W: "W", K: "K", KGCR: "K-GCR"}
same_bits, host_spmv, host_crs, downloaded = base.same_bits, base.host_spmv, base.host_crs, base.downloaded


# ---- the restatement -----------------------------------------------------------------------------------------------

def ldot(a, b):
    return np.float64(np.dot(a.astype(LD), b.astype(LD)))


def transition_kind(n_levels, t, cycle, cycle_levels):
    return cycle if (t < n_levels - 2 and (cycle_levels == 0 or t < cycle_levels)) else V


def coarse_solve(levels, rc, l, cfg):
    """e_c of transition l for the restricted residual rc."""
    N = l + 1
    A = levels[N]["A"]
    kind = transition_kind(len(levels), l, cfg["cycle"], cfg["cycle_levels"])
    c = cycle_reference(levels, rc, cfg, N)
    if kind == V:
        return c
    if kind == W:
        r2 = rc - host_spmv(A, c)
        return c + cycle_reference(levels, r2, cfg, N)
    with np.errstate(all="ignore"):
        v = host_spmv(A, c)
        t = c if kind == K else v
        rho1, alpha1 = ldot(t, v), ldot(t, rc)
        if rho1 == 0.0 or not np.isfinite(rho1):
            return np.zeros_like(rc)
        s1 = alpha1 / rho1
        rt = rc - s1 * v
        d = cycle_reference(levels, rt, cfg, N)
        w = host_spmv(A, d)
        t2 = d if kind == K else w
        gamma, beta, alpha2 = ldot(t2, v), ldot(t2, w), ldot(t2, rt)
        rho2 = beta - (gamma * gamma) / rho1
        if not rho2 > 0.0:
            c1, c2 = s1, np.float64(0.0)
        else:
            c2 = alpha2 / rho2
            c1 = s1 - (gamma * c2) / rho1
        return (c1 * c) + (c2 * d)


def cycle_reference(levels, b, cfg, l=0):
    """cfg: nu, coarse_sweeps, coarse_scale, cycle, cycle_levels."""
    L = levels[l]
    A, w = L["A"], L["w"]

    def sweep(x):
        return x + w * (b - host_spmv(A, x))

    x = w * b
    if l + 1 == len(levels):
        for _ in range(cfg["coarse_sweeps"] - 1):
            x = sweep(x)
        return x
    for _ in range(cfg["nu"] - 1):
        x = sweep(x)
    d = b - host_spmv(A, x)
    agg = L["agg"]
    order = np.argsort(agg, kind="stable")
    ptr = np.searchsorted(agg[order], np.arange(int(agg.max()) + 2))
    rc = base.run_sums(d[order], ptr[:-1], ptr[1:])
    ec = coarse_solve(levels, rc, l, cfg)
    x = x + cfg["coarse_scale"] * ec[agg]
    for _ in range(cfg["nu"]):
        x = sweep(x)
    return x


def config(cycle=V, cycle_levels=0, nu=1, coarse_scale=1.0, coarse_sweeps=4):
    return dict(cycle=cycle, cycle_levels=cycle_levels, nu=nu, coarse_scale=coarse_scale, coarse_sweeps=coarse_sweeps)


def test_the_restatement_with_cycle_v_is_the_v_cycle_of_test_gpu_mg(built):
    e = built("hpcg997")
    v = np.random.default_rng(3).uniform(-1, 1, e["n"])
    assert same_bits(cycle_reference(e["levels"], v, config(nu=2, coarse_scale=1.5)),
                     base.cycle_reference(e["levels"], v, nu=2, coarse_scale=1.5))


# ---- device side ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


# name -> (generator, coarse_limit, the rows the hierarchy must have: the cycle is exercised as the name says)
INPUTS = {
    "hpcg876": (lambda c: c.gen_hpcg(8, 7, 6), 8, [336, 48, 8]),                          # one W / K transition
    "hpcg16": (lambda c: c.gen_hpcg(16, 16, 16), 8, [4096, 512, 64, 8]),                  # K nested in K
    "hpcg997": (lambda c: c.gen_hpcg(9, 7, 5), 8, [315, 60, 12, 2]),                      # odd lengths, vector tails
    "hpcg402420": (lambda c: c.gen_hpcg(40, 24, 20), 30, [19200, 2400, 300, 45, 12]),     # three nested transitions
    "hpcg644840": (lambda c: c.gen_hpcg(64, 48, 40), 256, None),                          # dots over many workgroups
    "unstr666": (lambda c: c.gen_unstr(6, 6, 6), 8, None),                                # MIS aggregates
    "fem666": (lambda c: c.gen_fem(6, 6, 6), 8, None),                                    # three unknowns per node
}
RP64 = ["hpcg876", "hpcg16"]
CASES = list(INPUTS) + [n + "_rp64" for n in RP64]


@pytest.fixture(scope="module")
def built(ctx):
    """Per input, made once and left alone: the matrix, its host copy, the downloaded hierarchy (it does not depend on nu,
    coarse_scale or the cycle) and the three right-hand sides."""
    cache = {}

    def get(name):
        if name not in cache:
            key = name.replace("_rp64", "")
            make, limit, rows = INPUTS[key]
            if name.endswith("_rp64"):
                with OptionScope(ctx, force_rp64=1):
                    dA = make(ctx)
                    mg = ctx.mg(dA, coarse_limit=limit)
                    levels = downloaded(mg)
                assert all(L["rp_width"] == 8 for L in levels)
            else:
                dA = make(ctx)
                mg = ctx.mg(dA, coarse_limit=limit)
                levels = downloaded(mg)
            A = levels[0]["A"]
            n = A.n_rows
            assert mg.levels >= 3, (name, mg.rows)
            if rows is not None:
                assert mg.rows == rows, (name, mg.rows)
            if key == "hpcg644840":
                assert mg.rows[0] == 122880 and mg.rows[1] == 15360
            rng = np.random.default_rng(17)
            rhs = [host_spmv(A, np.ones(n)), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n) * 1e3]
            mg.free()
            cache[name] = dict(dA=dA, A=A, n=n, levels=levels, limit=limit, rhs=rhs, rp64=name.endswith("_rp64"))
        return cache[name]
    return get


def make_mg(ctx, e, **kw):
    if e["rp64"]:
        with OptionScope(ctx, force_rp64=1):
            return ctx.mg(e["dA"], coarse_limit=e["limit"], **kw)
    return ctx.mg(e["dA"], coarse_limit=e["limit"], **kw)


apply_host = base.apply_host


@pytest.mark.parametrize("nu,scale", [(1, 1.0), (2, 1.5)], ids=["nu1", "nu2_scale1.5"])
@pytest.mark.parametrize("cycle_levels", [0, 1])
@pytest.mark.parametrize("cycle", [W, K, KGCR], ids=["W", "K", "KGCR"])
@pytest.mark.parametrize("name", CASES)
def test_apply_against_the_restatement(ctx, built, name, cycle, cycle_levels, nu, scale):
    e = built(name)
    mg = make_mg(ctx, e, nu=nu, coarse_scale=scale, cycle=cycle, cycle_levels=cycle_levels)
    assert mg.cycle == (cycle, cycle_levels)
    cfg = config(cycle, cycle_levels, nu, scale)
    worst = 0.0
    for k, v in enumerate(e["rhs"]):
        ref = cycle_reference(e["levels"], v, cfg)
        out = apply_host(ctx, mg, v)
        dev = np.max(np.abs(out - ref)) / np.max(np.abs(ref))
        worst = max(worst, dev)
        print(f"{name} {NAMES[cycle]} cycle_levels {cycle_levels} nu {nu} scale {scale} rhs {k}: |dev - ref|_inf / |ref|_inf = {dev:.3e}")
    mg.free()
    assert worst <= GATE


@pytest.mark.parametrize("name", list(INPUTS))
def test_the_cycle_is_really_another_operator(ctx, built, name):
    """The parity test would pass on V's result if the restatement and the device both ignored the setting: they do not."""
    e = built(name)
    v = e["rhs"][1]
    ref_v = cycle_reference(e["levels"], v, config())
    for cycle in (W, K, KGCR):
        mg = make_mg(ctx, e, cycle=cycle)
        out = apply_host(ctx, mg, v)
        mg.free()
        assert np.max(np.abs(out - ref_v)) > 1e-6 * np.max(np.abs(ref_v)), NAMES[cycle]


@pytest.mark.parametrize("name", list(INPUTS))
def test_bits(ctx, built, name):
    e = built(name)
    v = e["rhs"][1]
    fresh = make_mg(ctx, e)
    assert fresh.cycle == (V, 0)
    out_v = apply_host(ctx, fresh, v)
    fresh.free()
    two = make_mg(ctx, e, max_levels=2)
    assert two.levels == 2
    two_v = apply_host(ctx, two, v)
    mg = make_mg(ctx, e)
    for cycle in (W, K, KGCR):
        mg.set_cycle(cycle)
        out = apply_host(ctx, mg, v)
        assert not same_bits(out, out_v)
        assert same_bits(apply_host(ctx, mg, v), out), "two applies differ"
        assert same_bits(apply_host(ctx, mg, v, alias=True), out), "out aliasing in differs"
        assert same_bits(apply_host(ctx, mg, v, through_dispatcher=True), out), "type 10 through bis_apply_preconditioner differs"
        assert same_bits(apply_host(ctx, mg, v, alias=True, through_dispatcher=True), out)
        mg.set_cycle(cycle, 99)
        assert mg.cycle == (cycle, 99)
        assert same_bits(apply_host(ctx, mg, v), out), "cycle_levels past the hierarchy is not cycle_levels = 0"
        mg.set_cycle(cycle, 1)
        one = apply_host(ctx, mg, v)
        if mg.levels > 3:
            assert not same_bits(one, out)
        else:  # one transition can carry the cycle: 1 is all of them
            assert same_bits(one, out)
        mg.set_cycle("v")
        assert mg.cycle == (V, 0)
        assert same_bits(apply_host(ctx, mg, v), out_v), "V set again does not give the bits of a hierarchy that never left V"
        two.set_cycle(cycle)
        assert same_bits(apply_host(ctx, two, v), two_v), "a two-level hierarchy does not give V's bits"
    mg.free()
    two.free()


@pytest.mark.parametrize("name", list(INPUTS))
def test_zero_in_gives_zero_out(ctx, built, name):
    e = built(name)
    mg = make_mg(ctx, e)
    for cycle in ("v", "w", "k", "kgcr"):
        mg.set_cycle(cycle)
        for alias in (False, True):
            out = apply_host(ctx, mg, np.zeros(e["n"]), alias=alias)
            assert not np.isnan(out).any() and np.array_equal(out, np.zeros(e["n"])), (cycle, alias)
    mg.free()


@pytest.mark.parametrize("name", ["hpcg876", "hpcg16", "hpcg997", "hpcg402420", "unstr666", "fem666"])
def test_w_is_a_fixed_symmetric_positive_definite_operator(ctx, built, name):
    e = built(name)
    n = e["n"]
    rng = np.random.default_rng(13)
    u, v = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    mg = make_mg(ctx, e, cycle="w")
    Mv, Mu = apply_host(ctx, mg, v), apply_host(ctx, mg, u)
    Muv = apply_host(ctx, mg, u + v)
    mg.free()
    a, b = u @ Mv, v @ Mu
    scale = np.linalg.norm(u) * np.linalg.norm(Mv)
    print(f"{name}: (u, M^-1 v) = {a:.15e}, (v, M^-1 u) = {b:.15e}, difference / (|u| |M^-1 v|) = {abs(a - b) / scale:.3e}")
    assert abs(a - b) <= 1e-12 * scale
    assert v @ Mv > 0 and u @ Mu > 0
    assert np.max(np.abs(Muv - (Mu + Mv))) <= 1e-12 * np.max(np.abs(Muv))  # linear


def test_errors(ctx, built):
    from basic_iterative_solvers_amd import BisError
    e = built("fem666")
    mg = make_mg(ctx, e, cycle="w", cycle_levels=1)
    lib = ctx.lib
    for cycle, levels in ((-1, 0), (4, 0), (K, -1), (V, -3)):
        assert lib.bis_mg_set_cycle(ctx.h, mg.h, C.c_int(cycle), C.c_int(levels)) == INVALID, (cycle, levels)
        assert mg.cycle == (W, 1), "a refused call changed the setting"
    assert lib.bis_mg_set_cycle(ctx.h, None, C.c_int(K), C.c_int(0)) == INVALID
    assert lib.bis_mg_set_cycle(None, mg.h, C.c_int(K), C.c_int(0)) == 1
    c, k = C.c_int(-7), C.c_int(-7)
    assert lib.bis_mg_cycle(None, C.byref(c), C.byref(k)) == INVALID and (c.value, k.value) == (-7, -7)
    assert lib.bis_mg_cycle(mg.h, None, C.byref(k)) == 0 and k.value == 1
    assert lib.bis_mg_cycle(mg.h, C.byref(c), None) == 0 and c.value == W
    with pytest.raises(BisError):
        mg.set_cycle("x")
    with pytest.raises(BisError, match="status 2"):
        make_mg(ctx, e, cycle=7)
    # what is not built stays refused with K set
    mg.set_cycle("k")
    dA, n, k = e["dA"], e["n"], 2
    X, B, T = ctx.upload(np.zeros(n * k)), ctx.upload(np.ones(n * k)), ctx.upload(np.zeros(n * k))
    with pytest.raises(BisError, match="status 6"):
        ctx.mapply_preconditioner("mg", n, k, mg.operand, None, None, None, None, None, X, B, T, None)
    for solver in (ctx.mcg(dA, B, X, k), ctx.mbicgstab(dA, B, X, k), ctx.mgmres(dA, B, X, k)):
        with pytest.raises(BisError, match="status 6"):
            solver.set_preconditioner("mg", Ls=mg.operand)
        solver.free()
    x, b = ctx.upload(np.zeros(n)), ctx.upload(np.ones(n))
    cg = ctx.cg(dA, b, x)
    with pytest.raises(BisError, match="status 6"):
        cg.set_preconditioner("mg", Ls=mg.operand, outer=2)
    cg.free()
    with pytest.raises(BisError, match="status 6"):
        ctx.apply_preconditioner("mg", n, mg.operand, None, None, None, None, None, x, b, None, None, outer=2)
    for vec in (X, B, T, x, b):
        vec.free()
    mg.free()


# ---- solves --------------------------------------------------------------------------------------------------------

CG_TOL = 1e-10
CG_PROTOTYPE = {V: 24, W: 18, K: 16}  # the CPU prototype's counts on HPCG 32^3


@pytest.fixture(scope="module")
def hpcg32(ctx):
    dA = ctx.gen_hpcg(32, 32, 32)
    mg = ctx.mg(dA, coarse_limit=64)
    assert mg.rows == [32768, 4096, 512, 64]
    levels = downloaded(mg)
    A = levels[0]["A"]
    b = host_spmv(A, np.ones(A.n_rows))
    runs = {}

    def device(cycle):
        if cycle not in runs:
            mg.set_cycle(cycle)
            runs[cycle] = base.device_cg(ctx, dA, b, "mg", Ls=mg.operand)
            mg.set_cycle(V)
        return runs[cycle]
    yield dict(dA=dA, A=A, b=b, mg=mg, levels=levels, device=device)
    mg.free()
    dA.free()


@pytest.mark.parametrize("cycle", [V, W, K], ids=["V", "W", "K"])
def test_cg_against_numpy_pcg_with_the_restated_cycle(hpcg32, cycle):
    e = hpcg32
    A, b = e["A"], e["b"]
    run = e["device"](cycle)
    cfg = config(cycle)
    ref_hist, _ = base.numpy_pcg(A, lambda r: cycle_reference(e["levels"], r, cfg), b, CG_TOL, 100)
    r0 = ref_hist[0]
    ref_iters = len(ref_hist) - 1
    dev = hist_dev(run["hist"], ref_hist)
    res = np.linalg.norm(b - host_spmv(A, run["x"]))
    print(f"hpcg32 {NAMES[cycle]}: device {run['iters']} iterations conv {run['conv']}, numpy {ref_iters}, prototype "
          f"{CG_PROTOTYPE[cycle]}, hist dev {dev:.3e}, true residual / r0 {res / r0:.3e}")
    assert run["conv"] and ref_hist[-1] < CG_TOL * r0
    assert abs(run["iters"] - ref_iters) <= (0 if cycle == V else 1)
    assert dev <= HIST_TOL["cg"]
    assert res <= 1e-9 * r0


def test_cg_needs_fewer_iterations_with_k_than_w_than_v(hpcg32):
    it = {c: hpcg32["device"](c)["iters"] for c in (V, W, K)}
    print(f"hpcg32 CG iterations: V {it[V]}, W {it[W]}, K {it[K]}")
    assert all(hpcg32["device"](c)["conv"] for c in (V, W, K))
    assert it[K] < it[W] < it[V]


def device_bicgstab(ctx, dA, b, mg, tol, budget):
    """The call-by-call BiCGSTAB of the host CLI (bicgstab_separate_iteration) from the single-vector calls, host scalars,
    x0 = 0, z = M^-1 r by bis_apply_preconditioner type 10."""
    n = len(b)
    db, x = ctx.upload(b), ctx.upload(np.zeros(n))
    names = ("xn", "h", "r", "rn", "r0", "p", "pn", "v", "s", "st", "y", "z", "t")
    w = {q: ctx.upload(np.zeros(n)) for q in names}

    def apply(out, inp):
        ctx.apply_preconditioner("mg", n, mg.operand, None, None, None, None, None, out, inp, None, None)

    f = np.float64
    ctx.copy_vector(w["r"], db)
    hist = [ctx.euclidean_vec_norm(w["r"])]
    apply(w["p"], w["r"])
    ctx.copy_vector(w["r0"], w["p"])
    rho = f(ctx.dot(w["r"], w["p"]))
    conv = False
    with np.errstate(all="ignore"):
        for _ in range(budget):
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
            hist.append(ctx.euclidean_vec_norm(w["rn"]))
            w["p"], w["pn"] = w["pn"], w["p"]
            w["r"], w["rn"] = w["rn"], w["r"]
            x, w["xn"] = w["xn"], x
            rho = rho_new
            conv = bool(abs(hist[-1]) < tol * hist[0])
            if conv or not np.isfinite(hist[-1]):
                break
    out = dict(iters=len(hist) - 1, conv=conv, hist=np.array(hist), x=x.to_host())
    for vec in list(w.values()) + [db, x]:
        vec.free()
    return out


def test_bicgstab_with_the_gcr_k_cycle_on_an_unstructured_input(ctx):
    dA = ctx.gen_unstr(8, 8, 8)
    A = host_crs(dA)
    b = host_spmv(A, np.ones(A.n_rows))
    mg = ctx.mg(dA, coarse_limit=64)
    assert mg.kinds[0] == 2 and mg.levels >= 3, mg.rows
    runs = {}
    for cycle in ("v", "kgcr"):
        mg.set_cycle(cycle)
        runs[cycle] = device_bicgstab(ctx, dA, b, mg, CG_TOL, 200)
    r0 = np.linalg.norm(b)
    res = np.linalg.norm(b - host_spmv(A, runs["kgcr"]["x"]))
    print(f"unstr888 rows {mg.rows}: BiCGSTAB V {runs['v']['iters']} iterations conv {runs['v']['conv']}, K-GCR {runs['kgcr']['iters']} "
          f"conv {runs['kgcr']['conv']}, true residual / r0 {res / r0:.3e}")
    assert runs["kgcr"]["conv"] and res <= 1e-9 * r0
    assert runs["v"]["conv"] and runs["kgcr"]["iters"] <= runs["v"]["iters"]
    mg.free()
    dA.free()
