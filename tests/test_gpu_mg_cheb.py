"""GPU: the Chebyshev smoother of the multigrid hierarchy (bis_mg_set_smoother) against tests/mg_cheb_ref.py, on the hierarchy
downloaded from the device (test_gpu_mg.py and test_gpu_mg_smoothed.py prove matrices, aggregates, weights and transfers
bit for bit): the bound bit for bit, the power iteration's estimate at the project's history gate (1e-10 relative: only the
order of the reductions differs), the rule for lambda_max, the coefficients bit for bit from the device's own lambda_max;
the cycle at the project's kernel gate 1e-13 |.|_inf (V, W, K; plain and smoothed hierarchies; degrees 1..4; nu 1 and 2; with
and without the estimate); the bit-for-bit promises; symmetry and definiteness; the fused CG against a numpy PCG with the
restated cycle; the one-level polynomial preconditioner; MINRES, FGMRES and IDR; and the refusals.

The restated cycle takes its coefficients from the device's lambda_max (the coefficients themselves are compared bit for
bit), so that a deviation of the cycle is the cycle's and not the estimate's."""
import ctypes as C

import numpy as np
import pytest

import mg_cheb_ref as cheb
import test_gpu_mg as base
import test_gpu_mg_cycle as cyc
import test_gpu_mg_smoothed as sa
from helpers import HIST_TOL, hist_dev

pytestmark = pytest.mark.gpu
GATE = base.GATE
K_GATE = cyc.GATE
EST_GATE = 1e-10
INVALID = 2
V, W, K, KGCR = cheb.V, cheb.W, cheb.K, cheb.KGCR
same_bits, host_crs, host_spmv, apply_host = base.same_bits, base.host_crs, base.host_spmv, base.apply_host

# name -> (generator, creation keywords)
INPUTS = {
    "hpcg876": (base.MATRICES["hpcg876"], dict(coarse_limit=30)),    # grid aggregates, three levels
    "fem666": (base.MATRICES["fem666"], dict(coarse_limit=30)),      # three unknowns per node, three levels
    "unstr666": (base.MATRICES["unstr666"], dict(coarse_limit=30)),  # MIS aggregates
    "band600": (base.MATRICES["band600"], dict(coarse_limit=30)),
    "hpcg753": (lambda c: c.gen_hpcg(7, 5, 3), dict(coarse_limit=30, max_levels=1)),  # 105 rows: the scalar tail, no coarsening
}
CASES = [(n, s) for n in INPUTS for s in (False, True)]
IDS = [f"{n}-{'smoothed' if s else 'plain'}" for n, s in CASES]


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


@pytest.fixture(scope="module")
def built(ctx):
    """Per (input, smoothed), made once and left alone: the matrix, the downloaded hierarchy and two right-hand sides."""
    mats, cache = {}, {}

    def get(name, smooth):
        if (name, smooth) not in cache:
            make, kw = INPUTS[name]
            if name not in mats:
                mats[name] = make(ctx)
            dA = mats[name]
            mg = ctx.mg(dA, smooth=smooth, **kw)
            levels = sa.downloaded(mg) if smooth else base.downloaded(mg)
            mg.free()
            n = dA.n_rows
            rng = np.random.default_rng(11)
            if name == "hpcg753":
                assert n == 105 and len(levels) == 1
            else:
                assert len(levels) >= 2
            cache[(name, smooth)] = dict(dA=dA, A=levels[0]["A"], n=n, levels=levels, kw=dict(kw, smooth=smooth),
                                         rhs=[rng.uniform(-1, 1, n), host_spmv(levels[0]["A"], np.ones(n))])
        return cache[(name, smooth)]
    return get


def device_smoother(mg, levels):
    """cfg["cheb"] from the device's own lambda_max (and the check that the device's coefficients are those)."""
    s = mg.smoother()
    lmax = [mg.spectrum(l)["lambda_max"] for l in range(mg.levels)]
    sm = cheb.smoother(levels, degree=s["degree"], ratio=s["ratio"], lambda_max=lmax)
    for l in range(mg.levels):
        c1, c2 = mg.cheb_coeffs(l)
        assert same_bits(c1, sm[l][0]) and same_bits(c2, sm[l][1]), f"coefficients of level {l}"
    return sm


@pytest.mark.parametrize("name,smooth", CASES, ids=IDS)
def test_spectrum_and_coefficients(ctx, built, name, smooth):
    e = built(name, smooth)
    levels = e["levels"]
    mg = ctx.mg(e["dA"], **e["kw"])
    assert mg.smoother() == dict(kind=0, degree=0, ratio=0.0, est_steps=0, safety=0.0) and mg.spectrum(0) is None and mg.cheb_coeffs(0) is None
    for degree, ratio, est, safety in ((3, 4.0, 10, 1.1), (8, 30.0, 0, 1.0), (2, 10.0, 3, 4.0)):
        mg.set_smoother("cheb", degree=degree, ratio=ratio, est_steps=est, safety=safety)
        assert mg.smoother() == dict(kind=1, degree=degree, ratio=ratio, est_steps=est, safety=safety)
        for l, L in enumerate(levels):
            d = mg.spectrum(l)
            want_bound = cheb.bound(L["A"], L["w"])
            assert same_bits(d["bound"], want_bound), (l, d["bound"], want_bound)
            if est == 0:
                assert d["estimate"] == 0.0 and d["lambda_max"] == d["bound"]
            else:
                want = cheb.power_estimates(L["A"], L["w"], est)[-1]
                dev = abs(d["estimate"] - want) / abs(want)
                print(f"{name} smooth {smooth} level {l} ({L['A'].n_rows} rows) est {est}: bound {d['bound']:.15e}, estimate {d['estimate']:.15e}, "
                      f"restated {want:.15e}, relative difference {dev:.3e}")
                assert dev <= EST_GATE
                assert 0.0 < d["estimate"] <= d["bound"] * (1 + 1e-12)
                assert d["lambda_max"] == min(np.float64(d["bound"]), np.float64(safety) * np.float64(d["estimate"]))
                if safety == 4.0:
                    assert d["lambda_max"] == d["bound"]  # (the estimates are above a quarter of the bound: the minimum takes the bound)
            assert d["lambda_min"] == np.float64(d["lambda_max"]) / np.float64(ratio)
            c1, c2 = mg.cheb_coeffs(l)
            w1, w2 = cheb.coeffs(d["lambda_max"], d["lambda_min"], degree)
            assert len(c1) == degree and same_bits(c1, w1) and same_bits(c2, w2), (l, c1, w1, c2, w2)
        assert mg.spectrum(mg.levels) is None and mg.spectrum(-1) is None and mg.cheb_coeffs(mg.levels) is None
    mg.free()


@pytest.mark.parametrize("cycle", [V, W], ids=["V", "W"])
@pytest.mark.parametrize("est", [0, 10], ids=["est0", "est10"])
@pytest.mark.parametrize("name,smooth", CASES, ids=IDS)
def test_cycle_against_the_restatement(ctx, built, name, smooth, est, cycle):
    e = built(name, smooth)
    levels, v = e["levels"], e["rhs"][0]
    worst = 0.0
    for nu in (1, 2):
        mg = ctx.mg(e["dA"], nu=nu, cycle=cycle, **e["kw"])
        for degree in (1, 2, 3, 4):
            mg.set_smoother("cheb", degree=degree, est_steps=est)
            cfg = cheb.config(cheb=device_smoother(mg, levels), cycle=cycle, nu=nu)
            ref = cheb.cycle(levels, v, cfg)
            out = apply_host(ctx, mg, v)
            dev = np.max(np.abs(out - ref)) / np.max(np.abs(ref))
            worst = max(worst, dev)
            print(f"{name} smooth {smooth} est {est} cycle {cyc.NAMES[cycle]} nu {nu} degree {degree}: |dev - ref|_inf / |ref|_inf = {dev:.3e}")
            assert dev <= GATE
            if degree == 2:
                assert same_bits(apply_host(ctx, mg, v, through_dispatcher=True), out), "type 10 through bis_apply_preconditioner differs"
                jac = cheb.cycle(levels, v, cheb.config(cycle=cycle, nu=nu))
                assert np.max(np.abs(out - jac)) > 1e-6 * np.max(np.abs(jac)), "the smoother is Jacobi's"
        mg.free()
    print(f"{name} smooth {smooth} est {est} cycle {cyc.NAMES[cycle]}: worst deviation {worst:.3e}")


@pytest.mark.parametrize("cycle", [K, KGCR], ids=["K", "KGCR"])
@pytest.mark.parametrize("smooth", [False, True], ids=["plain", "smoothed"])
@pytest.mark.parametrize("name", ["hpcg876", "fem666"])
def test_k_cycle_against_the_restatement(ctx, built, name, smooth, cycle):
    e = built(name, smooth)
    levels = e["levels"]
    assert len(levels) >= 3
    mg = ctx.mg(e["dA"], cycle=cycle, smoother="cheb", degree=2, est_steps=10, **e["kw"])
    cfg = cheb.config(cheb=device_smoother(mg, levels), cycle=cycle)
    worst = 0.0
    for k, v in enumerate(e["rhs"]):
        ref = cheb.cycle(levels, v, cfg)
        out = apply_host(ctx, mg, v)
        dev = np.max(np.abs(out - ref)) / np.max(np.abs(ref))
        worst = max(worst, dev)
        print(f"{name} smooth {smooth} {cyc.NAMES[cycle]} rhs {k}: |dev - ref|_inf / |ref|_inf = {dev:.3e}")
        assert same_bits(apply_host(ctx, mg, v), out), "two applies differ"
    mg.free()
    assert worst <= K_GATE


@pytest.mark.parametrize("name,smooth", CASES, ids=IDS)
def test_bits(ctx, built, name, smooth):
    e = built(name, smooth)
    v = e["rhs"][0]
    fresh = ctx.mg(e["dA"], **e["kw"])
    jac = {c: None for c in (V, W, K)}
    for c in jac:
        fresh.set_cycle(c)
        jac[c] = apply_host(ctx, fresh, v)
    fresh.free()
    mg = ctx.mg(e["dA"], **e["kw"])
    mg.set_smoother("cheb", degree=3)
    out = apply_host(ctx, mg, v)
    assert not same_bits(out, jac[V])
    assert same_bits(apply_host(ctx, mg, v), out), "two applies differ"
    assert same_bits(apply_host(ctx, mg, v, alias=True), out), "out aliasing in differs"
    assert same_bits(apply_host(ctx, mg, v, alias=True, through_dispatcher=True), out)
    assert not apply_host(ctx, mg, np.zeros(e["n"])).any(), "in = 0 does not give out = 0"
    # the cycle set after the smoother, and before it
    after = {}
    for c in (W, K):
        mg.set_cycle(c)
        after[c] = apply_host(ctx, mg, v)
    for c in (W, K):
        other = ctx.mg(e["dA"], cycle=c, **e["kw"])
        other.set_smoother("cheb", degree=3)
        assert same_bits(apply_host(ctx, other, v), after[c]), f"set_cycle({c}) before and after set_smoother differ"
        other.set_smoother("jacobi")
        assert other.smoother()["kind"] == 0 and other.spectrum(0) is None
        assert same_bits(apply_host(ctx, other, v), jac[c]), f"Jacobi set again under cycle {c} does not give a fresh hierarchy's bits"
        other.free()
    mg.set_cycle(V)
    assert same_bits(apply_host(ctx, mg, v), out)
    mg.set_smoother(0, degree=99, ratio=-1.0, est_steps=-5, safety=0.0)  # (for Jacobi the other fields are ignored)
    assert same_bits(apply_host(ctx, mg, v), jac[V]), "Jacobi set again does not give a fresh hierarchy's bits"
    mg.free()


@pytest.mark.parametrize("n", [301, 1400])
def test_on_a_diagonal_matrix_the_sweeps_are_the_restatement_bit_for_bit(ctx, n):
    """A diagonal matrix is one level (every row is a root: the step is dropped), and with powers of two on the diagonal its
    SpMV is exact on the device and in the restatement alike (the restatement's longdouble product, rounded twice, is not the
    fp64 product in general), so the polynomial's own arithmetic is compared bit for bit: a product contracted into the sum
    that follows it (c1 d + c2 u, or x + d at step 0) shows here and nowhere else."""
    rng = np.random.default_rng(n)
    a = 2.0 ** rng.integers(-2, 3, n)
    dA = ctx.matrix(base.CRS(n, np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), a))
    v = rng.uniform(-1, 1, n)
    for degree in (1, 2, 3, 4):
        mg = ctx.mg(dA, omega=0.7, coarse_sweeps=3, coarse_limit=30, smoother="cheb", degree=degree, ratio=6.0)
        levels = base.downloaded(mg)
        assert len(levels) == 1
        ref = cheb.cycle(levels, v, cheb.config(cheb=device_smoother(mg, levels), coarse_sweeps=3))
        out = apply_host(ctx, mg, v)
        assert np.max(np.abs(ref)) > 0 and same_bits(out, ref), (degree, int(np.sum(out != ref)), float(np.max(np.abs(out - ref))))
        mg.free()
    dA.free()


@pytest.mark.parametrize("name", ["hpcg876", "hpcg753"])
def test_vectors_off_a_16_byte_boundary_give_the_same_bits(ctx, built, name):
    """in and out 8 bytes off: level 0 takes the 8-byte path of both kernels (even and odd n)."""
    e = built(name, False)
    n, v = e["n"], e["rhs"][0]
    mg = ctx.mg(e["dA"], smoother="cheb", degree=3, nu=2, **e["kw"])
    want = apply_host(ctx, mg, v)
    din, dout = ctx.upload(np.concatenate([[7.0], v])), ctx.upload(np.full(n + 1, np.nan))
    assert din.ptr % 16 == 0 and dout.ptr % 16 == 0
    mg.apply(dout.offset(1), din.offset(1))
    got = dout.to_host()
    assert np.isnan(got[0]) and same_bits(got[1:], want)
    mg.apply(din.offset(1), din.offset(1))
    got = din.to_host()
    assert got[0] == 7.0 and same_bits(got[1:], want), "aliased, off the boundary"
    din.free(); dout.free(); mg.free()


@pytest.mark.parametrize("cycle", [V, W], ids=["V", "W"])
@pytest.mark.parametrize("name,smooth", CASES, ids=IDS)
def test_symmetry_and_definiteness(ctx, built, name, smooth, cycle):
    e = built(name, smooth)
    n = e["n"]
    rng = np.random.default_rng(13)
    u, v = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    mg = ctx.mg(e["dA"], cycle=cycle, smoother="cheb", degree=3, **e["kw"])
    Mv, Mu = apply_host(ctx, mg, v), apply_host(ctx, mg, u)
    mg.free()
    a, b = u @ Mv, v @ Mu
    scale = np.linalg.norm(u) * np.linalg.norm(Mv)
    print(f"{name} smooth {smooth} {cyc.NAMES[cycle]}: (u, M^-1 v) = {a:.15e}, (v, M^-1 u) = {b:.15e}, difference / (|u| |M^-1 v|) = "
          f"{abs(a - b) / scale:.3e}")
    assert abs(a - b) <= 1e-12 * scale
    assert v @ Mv > 0 and u @ Mu > 0


CG_TOL = base.CG_TOL


@pytest.mark.parametrize("smooth", [False, True], ids=["plain", "smoothed"])
@pytest.mark.parametrize("name,make", [("hpcg16", lambda c: c.gen_hpcg(16, 16, 16)), ("unstr888", lambda c: c.gen_unstr(8, 8, 8))],
                         ids=["hpcg16", "unstr888"])
def test_cg_against_numpy_pcg_with_the_restated_cycle(ctx, name, make, smooth):
    dA = make(ctx)
    mg = ctx.mg(dA, smooth=smooth, coarse_limit=64, smoother="cheb", degree=2, est_steps=10)
    levels = sa.downloaded(mg) if smooth else base.downloaded(mg)
    A = levels[0]["A"]
    assert len(levels) >= 2
    b = host_spmv(A, np.ones(A.n_rows))
    run = base.device_cg(ctx, dA, b, "mg", Ls=mg.operand)
    cfg = cheb.config(cheb=device_smoother(mg, levels))
    ref_hist, _ = base.numpy_pcg(A, lambda r: cheb.cycle(levels, r, cfg), b, CG_TOL, 400)
    jacobi = ctx.mg(dA, smooth=smooth, coarse_limit=64, nu=2)  # the same number of SpMVs a cycle: a measurement, not a gate
    jrun = base.device_cg(ctx, dA, b, "mg", Ls=jacobi.operand)
    jacobi.free()
    r0 = ref_hist[0]
    dev = hist_dev(run["hist"], ref_hist)
    res = np.linalg.norm(b - host_spmv(A, run["x"]))
    print(f"{name} smooth {smooth}: rows {mg.rows}, lambda_max {[mg.spectrum(l)['lambda_max'] for l in range(mg.levels)]}; Chebyshev degree 2 nu 1: "
          f"device {run['iters']} iterations conv {run['conv']}, numpy {len(ref_hist) - 1}; Jacobi nu 2: {jrun['iters']} iterations conv "
          f"{jrun['conv']}; hist dev {dev:.3e}, true residual {res:.6e}, last entry {run['hist'][-1]:.6e}, r0 {r0:.6e}")
    assert run["conv"] and ref_hist[-1] < CG_TOL * r0
    assert run["iters"] == len(ref_hist) - 1
    assert dev <= HIST_TOL["cg"]
    assert res <= run["hist"][-1] + 1e-10 * r0
    mg.free()
    dA.free()


def test_the_one_level_polynomial_preconditioner(ctx):
    dA = ctx.gen_hpcg(16, 16, 16)
    mg = ctx.mg(dA, max_levels=1, coarse_sweeps=1, smoother="cheb", degree=4)
    assert mg.levels == 1
    levels = base.downloaded(mg)
    A = levels[0]["A"]
    b = host_spmv(A, np.ones(A.n_rows))
    run = base.device_cg(ctx, dA, b, "mg", Ls=mg.operand)
    plain = base.device_cg(ctx, dA, b)
    jacobi = ctx.mg(dA, max_levels=1, coarse_sweeps=4)
    jrun = base.device_cg(ctx, dA, b, "mg", Ls=jacobi.operand)
    jacobi.free()
    cfg = cheb.config(cheb=device_smoother(mg, levels), coarse_sweeps=1)
    ref_hist, _ = base.numpy_pcg(A, lambda r: cheb.cycle(levels, r, cfg), b, CG_TOL, 400)
    res = np.linalg.norm(b - host_spmv(A, run["x"]))
    print(f"hpcg16, one level: Chebyshev degree 4: {run['iters']} iterations (numpy {len(ref_hist) - 1}), four Jacobi sweeps {jrun['iters']}, "
          f"unpreconditioned {plain['iters']}; true residual / r0 {res / ref_hist[0]:.3e}")
    assert run["conv"] and plain["conv"] and run["iters"] < plain["iters"]
    assert run["iters"] == len(ref_hist) - 1 and hist_dev(run["hist"], ref_hist) <= HIST_TOL["cg"]
    assert res <= run["hist"][-1] + 1e-10 * ref_hist[0]
    mg.free()
    dA.free()


@pytest.mark.parametrize("solver", ["minres", "fgmres_k", "idr"])
def test_the_other_solver_families_take_the_hierarchy(ctx, built, solver):
    e = built("hpcg876", False)
    dA, A, b = e["dA"], e["A"], e["rhs"][1]
    mg = ctx.mg(dA, cycle="k" if solver == "fgmres_k" else None, smoother="cheb", degree=2, **e["kw"])
    db, dx = ctx.upload(b), ctx.upload(np.zeros_like(b))
    s = ctx.minres(dA, db, dx) if solver == "minres" else ctx.idr(dA, db, dx) if solver == "idr" else ctx.fgmres(dA, db, dx, restart=10)
    s.set_preconditioner("mg", Ls=mg.operand)
    s.init(CG_TOL)
    s.iterate(200)
    iters, conv, _ = s.status()
    res = np.linalg.norm(b - host_spmv(A, dx.to_host()))
    print(f"{solver} on hpcg876 with the Chebyshev hierarchy: {iters} iterations, converged {conv}, true residual / |b| {res / np.linalg.norm(b):.3e}")
    # 1e-6 |b|: the solvers stop at 1e-10 on their own estimate (MINRES: in the preconditioner's norm), four orders of room
    assert conv and iters < 100 and res <= 1e-6 * np.linalg.norm(b)
    s.free(); db.free(); dx.free(); mg.free()


def test_refusals(ctx, built):
    from basic_iterative_solvers_amd import BisError, MGSmoother
    e = built("hpcg876", False)
    v = e["rhs"][0]
    lib = ctx.lib
    mg = ctx.mg(e["dA"], smoother="cheb", degree=3, ratio=5.0, est_steps=4, safety=1.2, **e["kw"])
    state, out = mg.smoother(), apply_host(ctx, mg, v)
    good = dict(kind=1, degree=2, ratio=4.0, est_steps=10, safety=1.1)

    def call(h, **kw):
        p = dict(good, **kw)
        s = MGSmoother(p["kind"], p["degree"], p["ratio"], p["est_steps"], p["safety"])
        return lib.bis_mg_set_smoother(ctx.h, h, C.byref(s))

    assert call(None) == INVALID
    assert lib.bis_mg_set_smoother(ctx.h, mg.h, None) == INVALID
    for bad in (dict(kind=2), dict(kind=-1), dict(degree=0), dict(degree=9), dict(ratio=1.0), dict(ratio=float("nan")), dict(ratio=float("inf")),
                dict(est_steps=-1), dict(est_steps=101), dict(safety=0.5), dict(safety=float("nan"))):
        assert call(mg.h, **bad) == INVALID, bad
        assert mg.smoother() == state, f"a refused call changed the setting: {bad}"
    assert same_bits(apply_host(ctx, mg, v), out), "a refused call changed the cycle"
    with pytest.raises(BisError):
        mg.set_smoother("x")
    with pytest.raises(BisError, match="status 2"):
        ctx.mg(e["dA"], smoother="cheb", degree=9, **e["kw"])
    c1, c2 = (C.c_double * 8)(), (C.c_double * 8)()
    for level in (-1, mg.levels, 16):
        assert lib.bis_mg_level_cheb_coeffs(mg.h, C.c_int(level), c1, c2) == INVALID
    assert lib.bis_mg_level_cheb_coeffs(mg.h, C.c_int(0), c1, c2) == 0
    mg.set_smoother("jacobi")
    assert lib.bis_mg_level_cheb_coeffs(mg.h, C.c_int(0), c1, c2) == INVALID
    mg.free()
