"""GPU: smoothed aggregation (bis_mg_create_smoothed, Context.mg(smooth=True)) against tests/spgemm_ref.py.

Hierarchies: omega_l, P, R and the level operators bit for bit against the restatement, with the aggregates, weights and
hints test_gpu_mg.py already compares.  The cycle (two new transfer kernels) at 1e-13 |.|_inf against the restated cycle on
the downloaded hierarchy, the project's kernel gate; bit-for-bit promises (two applies, aliasing, the dispatcher); W and K
transitions on a smoothed hierarchy; the operator's symmetry and definiteness at the project's gates; the fused CG against a
numpy PCG with the restated cycle, in fewer iterations than on the unsmoothed hierarchy of the same input; MINRES and IDR;
and the refusals."""
import ctypes as C

import numpy as np
import pytest

import spgemm_ref as ref
import test_gpu_mg as base
from helpers import HIST_TOL, OptionScope, hist_dev

pytestmark = pytest.mark.gpu
GATE = 1e-13
INVALID = 2
same_bits, host_crs, host_spmv, apply_host = base.same_bits, base.host_crs, base.host_spmv, base.apply_host

# name -> (generator, coarse_limit)
INPUTS = {
    "hpcg876": (base.MATRICES["hpcg876"], 8),              # grid aggregates, odd sizes
    "fem666": (base.MATRICES["fem666"], 30),               # three unknowns per node
    "unstr666": (base.MATRICES["unstr666"], 8),            # MIS aggregates
    "band600": (base.MATRICES["band600"], 30),
    "band600_isolated": (base.MATRICES["band600_isolated"], 30),  # rows that are their own aggregate
    "hpcg402420": (base.MATRICES["hpcg402420"], 30),       # several workgroups in both transfer kernels
}
HIERARCHY_CASES = ["hpcg876", "fem666", "unstr666", "band600", "band600_isolated"]


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


def downloaded(mg):
    """The device hierarchy in the restatement's form: test_gpu_mg's dicts plus P, R, omega_l."""
    out = base.downloaded(mg)
    for l, L in enumerate(out):
        P, R = mg.prolongator(l), mg.restrictor(l)
        L["P"] = host_crs_rect(P) if P else None
        L["R"] = host_crs_rect(R) if R else None
        L["omega_l"] = mg.prolong_omega(l)
        L["transfer_rp_width"] = (P.rp_width, R.rp_width) if P else None
    return out


def host_crs_rect(dM):
    rp, col, val = dM.download()
    return ref.crs(dM.n_rows, dM.n_cols, rp, col, val)


@pytest.fixture(scope="module")
def built(ctx):
    """Per input, made once and left alone: the matrix, its host copy, the smoothed hierarchy and its download."""
    cache = {}

    def get(name):
        if name not in cache:
            make, limit = INPUTS[name]
            dA = make(ctx)
            mg = ctx.mg(dA, smooth=True, coarse_limit=limit)
            assert mg.smoothed
            cache[name] = dict(dA=dA, A=host_crs(dA), grid=base.grid_of(dA), mg=mg, dev=downloaded(mg), limit=limit)
        return cache[name]
    return get


def same_crs(a, b):
    return (a.n_rows, a.n_cols) == (b.n_rows, b.n_cols) and np.array_equal(a.row_ptr, b.row_ptr) and np.array_equal(a.col, b.col) and \
        same_bits(a.val, b.val)


def compare_smoothed(dev, want, tag):
    base.compare_hierarchies(dev, want, tag)
    for l, (d, r) in enumerate(zip(dev, want)):
        if r["P"] is None:
            assert d["P"] is None and d["R"] is None and d["omega_l"] is None, f"{tag}: level {l} is the coarsest"
            continue
        assert d["omega_l"] == r["omega_l"], f"{tag}: omega of level {l}: {d['omega_l']!r} != {r['omega_l']!r}"
        assert same_crs(d["P"], r["P"]), f"{tag}: P of level {l}"
        assert same_crs(d["R"], r["R"]), f"{tag}: R of level {l}"


@pytest.mark.parametrize("name", HIERARCHY_CASES)
def test_hierarchy_against_the_restatement(ctx, built, name):
    e = built(name)
    want = ref.hierarchy(e["A"], e["grid"], coarse_limit=e["limit"])
    dev = e["dev"]
    print(f"{name}: rows {[L['A'].n_rows for L in dev]}, nnz {[L['A'].nnz for L in dev]}, kinds {[L['kind'] for L in dev]}, "
          f"omega_l {[L['omega_l'] for L in dev[:-1]]}, nnz(P) {[L['P'].nnz for L in dev[:-1]]}")
    assert len(dev) >= 2 and dev[0]["kind"] == base.KIND[name]
    compare_smoothed(dev, want, name)
    assert e["mg"].nnz == [L["A"].nnz for L in dev]  # the level operators only
    assert dev[0]["omega_l"] == (4.0 / 3.0) / np.max(ref.abs_row_sums(e["A"]) / np.abs(ref.first_diagonal(e["A"])))
    if name == "band600_isolated":  # a row that is its own aggregate: one entry, 1 - c_i a_ii
        P, A = dev[0]["P"], e["A"]
        for i in (0, 311, 599):
            assert P.row_ptr[i + 1] - P.row_ptr[i] == 1
            d = A.val[A.row_ptr[i]]
            assert P.val[P.row_ptr[i]] == 1.0 - (dev[0]["omega_l"] / d) * d
    if name == "hpcg876":
        with OptionScope(ctx, force_rp64=1):
            dA = INPUTS[name][0](ctx)
            mg = ctx.mg(dA, smooth=True, coarse_limit=e["limit"])
            wide = downloaded(mg)
        assert all(L["rp_width"] == 8 for L in wide) and all(w == (8, 8) for w in [L["transfer_rp_width"] for L in wide[:-1]])
        assert all(L["rp_width"] == 4 for L in dev) and dev[0]["transfer_rp_width"] == (4, 4)
        for L in wide:
            L.pop("rp_width")
        compare_smoothed(wide, want, name + " rp64")
        mg.free()
        dA.free()


def test_two_setups_give_the_same_bits(ctx, built):
    for name in ("unstr666", "hpcg876"):
        e = built(name)
        mg2 = ctx.mg(e["dA"], smooth=True, coarse_limit=e["limit"])
        compare_smoothed(downloaded(mg2), e["dev"], name + " again")
        mg2.free()


def test_the_unsmoothed_hierarchy_is_what_it_was(ctx, built):
    for name in ("hpcg876", "unstr666"):
        e = built(name)
        mg = ctx.mg(e["dA"], coarse_limit=e["limit"])
        assert not mg.smoothed
        for l in range(-1, mg.levels + 1):
            assert mg.prolongator(l) is None and mg.restrictor(l) is None and mg.prolong_omega(l) is None
        base.compare_hierarchies(base.downloaded(mg), base.hierarchy_reference(e["A"], e["grid"], coarse_limit=e["limit"]), name)
        mg.free()
        sm = e["mg"]
        assert sm.prolongator(sm.levels - 1) is None and sm.prolongator(sm.levels) is None and sm.prolongator(-1) is None
        assert sm.prolong_omega(sm.levels - 1) is None


@pytest.mark.parametrize("name", list(INPUTS))
def test_cycle_against_the_restatement(ctx, built, name):
    e = built(name)
    n = e["A"].n_rows
    v = np.random.default_rng(11).uniform(-1, 1, n)
    levels = e["dev"]
    if name == "hpcg402420":
        assert levels[1]["A"].n_rows == 2400 and levels[0]["R"].n_rows > 4 * 256 // 64 and n > 256
    worst = 0.0
    for nu in (1, 2):
        for scale in (1.0, 1.5):
            mg = ctx.mg(e["dA"], smooth=True, coarse_limit=e["limit"], nu=nu, coarse_scale=scale)
            want = ref.cycle(levels, v, ref.config(nu=nu, coarse_scale=scale))
            out = apply_host(ctx, mg, v)
            dev = np.max(np.abs(out - want)) / np.max(np.abs(want))
            worst = max(worst, dev)
            print(f"{name}: nu {nu} scale {scale}: |dev - ref|_inf / |ref|_inf = {dev:.3e}")
            assert dev <= GATE
            assert same_bits(apply_host(ctx, mg, v), out), "two applies differ"
            assert same_bits(apply_host(ctx, mg, v, alias=True), out), "out aliasing in differs"
            assert same_bits(apply_host(ctx, mg, v, through_dispatcher=True), out), "type 10 differs from bis_mg_apply"
            mg.free()
    zero = apply_host(ctx, e["mg"], np.zeros(n))
    assert not zero.any()
    print(f"{name}: worst deviation {worst:.3e}")


@pytest.mark.parametrize("cycle", [ref.W, ref.K], ids=["W", "K"])
def test_w_and_k_cycles_on_a_smoothed_hierarchy(ctx, cycle):
    dA = ctx.gen_hpcg(16, 16, 16)
    mg = ctx.mg(dA, smooth=True, coarse_limit=8, cycle=cycle)
    assert mg.rows == [4096, 512, 64, 8] and mg.cycle == (cycle, 0)
    levels = downloaded(mg)
    A = levels[0]["A"]
    rng = np.random.default_rng(17)
    for k, v in enumerate([host_spmv(A, np.ones(A.n_rows)), rng.uniform(-1, 1, A.n_rows)]):
        want = ref.cycle(levels, v, ref.config(cycle=cycle))
        out = apply_host(ctx, mg, v)
        dev = np.max(np.abs(out - want)) / np.max(np.abs(want))
        print(f"hpcg16 smoothed, cycle {cycle}, rhs {k}: |dev - ref|_inf / |ref|_inf = {dev:.3e}")
        assert dev <= GATE
        assert same_bits(apply_host(ctx, mg, v), out)
    plain = ref.cycle(levels, v, ref.config())
    assert np.max(np.abs(plain - want)) > 1e-6 * np.max(np.abs(want)), "the cycle is V's"
    mg.set_cycle(0)
    assert np.max(np.abs(apply_host(ctx, mg, v) - plain)) <= GATE * np.max(np.abs(plain))
    mg.free()
    dA.free()


@pytest.mark.parametrize("name", list(INPUTS))
def test_the_operator_is_symmetric_and_definite(ctx, built, name):
    e = built(name)
    n = e["A"].n_rows
    rng = np.random.default_rng(13)
    u, v = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    Mv, Mu = apply_host(ctx, e["mg"], v), apply_host(ctx, e["mg"], u)
    a, b = u @ Mv, v @ Mu
    scale = np.linalg.norm(u) * np.linalg.norm(Mv)
    print(f"{name}: (u, M^-1 v) = {a:.15e}, (v, M^-1 u) = {b:.15e}, difference / (|u| |M^-1 v|) = {abs(a - b) / scale:.3e}")
    assert abs(a - b) <= 1e-12 * scale
    assert v @ Mv > 0 and u @ Mu > 0


CG_TOL = base.CG_TOL


@pytest.mark.parametrize("name,make", [("hpcg32", lambda c: c.gen_hpcg(32, 32, 32)), ("unstr888", lambda c: c.gen_unstr(8, 8, 8))],
                         ids=["hpcg32", "unstr888"])
def test_cg_against_numpy_pcg_and_fewer_iterations_than_unsmoothed(ctx, name, make):
    dA = make(ctx)
    A = host_crs(dA)
    mg = ctx.mg(dA, smooth=True, coarse_limit=64)
    levels = downloaded(mg)
    assert levels[0]["kind"] == (2 if name.startswith("unstr") else 1) and len(levels) >= 2
    b = host_spmv(A, np.ones(A.n_rows))
    run = base.device_cg(ctx, dA, b, "mg", Ls=mg.operand)
    ref_hist, _ = base.numpy_pcg(A, lambda r: ref.cycle(levels, r), b, CG_TOL, 400)
    plain_mg = ctx.mg(dA, coarse_limit=64)
    unsmoothed = base.device_cg(ctx, dA, b, "mg", Ls=plain_mg.operand)
    r0 = ref_hist[0]
    dev = hist_dev(run["hist"], ref_hist)
    res = np.linalg.norm(b - host_spmv(A, run["x"]))
    print(f"{name}: smoothed rows {mg.rows} nnz {mg.nnz}, unsmoothed rows {plain_mg.rows} nnz {plain_mg.nnz}; device {run['iters']} "
          f"iterations conv {run['conv']}, numpy {len(ref_hist) - 1}, unsmoothed {unsmoothed['iters']}, hist dev {dev:.3e}, "
          f"true residual {res:.6e}, last entry {run['hist'][-1]:.6e}, r0 {r0:.6e}")
    assert run["conv"] and ref_hist[-1] < CG_TOL * r0
    assert run["iters"] == len(ref_hist) - 1
    assert dev <= HIST_TOL["cg"]
    assert res <= run["hist"][-1] + 1e-10 * r0
    assert unsmoothed["conv"] and run["iters"] < unsmoothed["iters"]
    plain_mg.free()
    mg.free()
    dA.free()


@pytest.mark.parametrize("solver", ["minres", "idr"])
def test_minres_and_idr_take_the_smoothed_hierarchy(ctx, solver):
    dA = ctx.gen_hpcg(16, 16, 16)
    A = host_crs(dA)
    b = host_spmv(A, np.ones(A.n_rows))
    counts = {}
    for smooth in (False, True):
        mg = ctx.mg(dA, smooth=smooth, coarse_limit=64)
        db, dx = ctx.upload(b), ctx.upload(np.zeros_like(b))
        s = ctx.minres(dA, db, dx) if solver == "minres" else ctx.idr(dA, db, dx)
        s.set_preconditioner("mg", Ls=mg.operand)
        s.init(CG_TOL)
        s.iterate(200)
        iters, conv, hist = s.status()
        res = np.linalg.norm(b - host_spmv(A, dx.to_host()))
        print(f"{solver} on hpcg16, smooth {smooth}: {iters} iterations, converged {conv}, true residual / |b| {res / np.linalg.norm(b):.3e}")
        # 1e-6 |b|: the solvers stop at 1e-10 on their own estimate (MINRES: in the preconditioner's norm), four orders of room;
        # a solver that did not take the hierarchy would not converge within the budget of 200
        assert conv and res <= 1e-6 * np.linalg.norm(b)
        counts[smooth] = iters
        s.free(); db.free(); dx.free(); mg.free()
    print(f"{solver} on hpcg16: {counts[True]} iterations smoothed, {counts[False]} unsmoothed")
    dA.free()


def raw_create(ctx, A_h, prolong_omega, with_out=True):
    from basic_iterative_solvers_amd import MGParams
    p = base.DEFAULTS
    params = MGParams(p["max_levels"], 30, p["coarsening"], p["nu"], p["coarse_sweeps"], p["omega"], p["coarse_scale"])
    out = C.c_void_p()
    st = ctx.lib.bis_mg_create_smoothed(ctx.h, A_h, C.byref(params), C.c_double(prolong_omega), C.byref(out) if with_out else None)
    return st, out


def test_refusals(ctx, built):
    from basic_iterative_solvers_amd import BisError
    e = built("fem666")
    dA, mg, n = e["dA"], e["mg"], e["A"].n_rows
    for bad in (-1.0, 2.0, float("nan")):
        st, out = raw_create(ctx, dA.h, bad)
        assert st == INVALID and not out, bad
    st, out = raw_create(ctx, None, 0.0)
    assert st == INVALID and not out
    assert raw_create(ctx, dA.h, 0.0, with_out=False)[0] == INVALID
    st, out = raw_create(ctx, dA.h, 1.0)
    assert st == 0 and out
    w = C.c_double()
    rho = np.max(ref.abs_row_sums(e["A"]) / np.abs(ref.first_diagonal(e["A"])))
    assert ctx.lib.bis_mg_level_prolong_omega(out, C.c_int(0), C.byref(w)) == 0 and w.value == 1.0 / rho
    ctx.lib.bis_mg_destroy(ctx.h, out)
    # what -p mg refuses stays refused (test_gpu_mg.test_what_is_not_built_is_refused, on a smoothed hierarchy)
    k = 2
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
    with pytest.raises(BisError, match="status 2"):
        ctx.apply_preconditioner("mg", n - 1, mg.operand, None, None, None, None, None, x, b, None, None)
    for v in (X, B, T, x, b):
        v.free()
