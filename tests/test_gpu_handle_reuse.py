"""GPU: the solver handles on reuse -- bis_cg_*, bis_mcg_*, bis_mbicgstab_*, bis_mgmres_*, bis_fgmres_*, bis_minres_*,
bis_idr_* and bis_stat_* share one life cycle (create, [set_preconditioner], init, iterate ..., status / solution, destroy), and every other
module builds a fresh handle per solve.  Here a handle is used again:

A. `init` a second time on a handle that has converged, that was cut off inside a cycle after 7 iterations, or that was
   poisoned with NaN by b = 0 from x0 = 0.  The second system is written into the handle's own device buffers.  The run that
   follows must give the bits of a fresh handle on the same system: r0, iteration counts, converged flags, histories, x and
   solution().  (Vec.set is a blocking upload, so no launch of the first solve is still queued at the second init; the test
   makes no other synchronisation of its own between the two.)  The fresh handle's correctness is each solver module's
   business; here one figure anchors the re-initialised run outside the library: the residual of the returned x, recomputed
   in np.longdouble from the host CRS, in the norm the handle's history records (bis_hip.h: the 2-norm of b - A x for
   bis_cg, bis_mcg, bis_mbicgstab, bis_fgmres, bis_idr, bis_stat and every unpreconditioned handle; || M^-1 (b - A x) ||_2 for a
   preconditioned bis_mgmres; sqrt((r, M^-1 r)) for a preconditioned bis_minres, M^-1 r by the oracle's apply), is at most the
   last history entry + 1e-10 times entry 0 -- tests/test_gpu_fgmres.py's bound.
B. Two live handles on one context, advanced one iteration at a time in turn, against the same solves made alone on another
   context; and a live handle next to one that has already stopped.
C. The plain kernels on a context whose handles have stopped: the stop flag of a solve must not outlive its iterate call.
D. What set_preconditioner answers on an initialised handle (include/bis_hip.h states it per family).

Each test prints what it measured before it asserts."""
import numpy as np
import pytest

from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

K = 3            # columns of the lock-step handles
M = 5            # restart length of both GMRES forms
S = 4            # shadow vectors of IDR(s): a cycle of S + 1 positions
Q = 7            # the budget stop: odd, no multiple of 3 (MINRES' rotation), no multiple of M or S + 1 (inside a cycle)
BUDGET = 400
PATTERN = (3, 4, BUDGET)  # the iterate calls of every second solve: call boundaries inside a cycle, then past the stop
LOCKSTEP = ("mcg", "mbicgstab", "mgmres")
HAS_SOLUTION = ("mgmres", "fgmres", "stat")
NONSYMMETRIC = ("mbicgstab", "mgmres", "fgmres", "idr")
CONFIGS = {
    "cg": ["none", "A_D", "sgs", "ilu0"],
    "mcg": ["none", "A_D", "sgs"],
    "mbicgstab": ["none", "ilu0"],
    "mgmres": ["none", "sgs"],
    "fgmres": ["none", "sgs", "sgs-outer2"],
    "minres": ["none", "j", "sgs"],
    "idr": ["none", "sgs"],
    "stat": ["j", "gs", "sgs"],
}
CASES = [(kind, cfg) for kind, cfgs in CONFIGS.items() for cfg in cfgs]
WIDE_CASES = [("cg", "sgs"), ("mcg", "A_D"), ("mbicgstab", "ilu0"), ("mgmres", "sgs"), ("fgmres", "sgs"), ("minres", "j"),
              ("idr", "sgs"), ("stat", "j")]
# b = 0 from x0 = 0: NaN at iteration 1, stopped, not converged -- pinned by tests/test_gpu_mcg.py (bis_cg and bis_mcg),
# test_gpu_mgmres.py, test_gpu_fgmres.py, test_gpu_minres.py and test_gpu_idr.py
ZERO_RHS_PINNED = ("cg", "mcg", "mgmres", "fgmres", "minres", "idr")


def tol_first(kind, cfg=None):
    """The converged first solve's tolerance.  BiCGSTAB with ILU(0) on 693 rows gains 2 to 3 digits per iteration and its three
    columns all cross 1e-11 in iteration 5; their histories at iteration 4 are 1.9e-10, 2.9e-11 and 3.2e-11 of r0, so 1e-10
    stops them at 5, 4 and 4."""
    if kind == "stat":
        return 1e-3
    return 1e-10 if (kind, cfg) == ("mbicgstab", "ilu0") else 1e-11


def tol_second(kind):
    return 1e-2 if kind == "stat" else 1e-5


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


def make_system(ctx, dims, nonsymmetric=False):
    """The 27-point matrix on a dims grid (nonsymmetric: its strict upper triangle scaled by 0.5 on the host) with the
    operands of the preconditioners; the ILU(0) factors are made at their first use."""
    dA = ctx.gen_hpcg(*dims)
    A = CRS(dA.n_rows, *dA.download())
    if nonsymmetric:
        rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
        A = CRS(A.n_rows, A.row_ptr, A.col, np.where(A.col > rows, 0.5 * A.val, A.val))
        dA.free()
        dA = ctx.matrix(A)
    Ls, Us, D, Dinv = ctx.split_strict(dA)
    return dict(ctx=ctx, dA=dA, A=A, n=A.n_rows, Ls=Ls, Us=Us, D=D, Dinv=Dinv, ilu=None, fresh={}, host={})


def pc_args(e, pc):
    if pc == "ilu0":
        if e["ilu"] is None:
            iLs, iLD, iUs, iUD = e["ctx"].ilu0(e["dA"])
            iUinv = e["ctx"].alloc(e["n"])
            e["ctx"].elemwise_div_vectors(iUinv, iLD, iUD, n=e["n"])
            e["ilu"] = dict(Ls=iLs, Us=iUs, A_D=iLD, A_D_inv=iUinv, L_D=iLD, U_D=iUD)
        return e["ilu"]
    return dict(Ls=e["Ls"], Us=e["Us"], A_D=e["D"], A_D_inv=e["Dinv"], L_D=e["D"], U_D=e["D"])


@pytest.fixture(scope="module")
def systems(ctx):
    """693 rows (odd: every n & 1 tail; more than one 512-entry workgroup), symmetric and not; 8379 rows (odd; 17 workgroups
    of 512 entries: both levels of the last-arriver counters).  Built once, never changed."""
    return dict(spd=make_system(ctx, (9, 7, 11)), ns=make_system(ctx, (9, 7, 11), nonsymmetric=True),
                wide=make_system(ctx, (21, 21, 19)))


def small_system(systems, kind):
    return systems["ns" if kind in NONSYMMETRIC else "spd"]


class Solve:
    """One handle of `kind` in configuration `cfg` with device buffers b, x of its own; every handle type behind one
    interface, the lock-step ones with K interleaved columns (host arrays n x K)."""

    def __init__(self, ctx, e, kind, cfg, b, x0):
        self.ctx, self.e, self.kind, self.cfg = ctx, e, kind, cfg
        self.k = K if kind in LOCKSTEP else 1
        self.n = e["n"]
        self.db, self.dx = ctx.upload(np.ravel(b)), ctx.upload(np.ravel(x0))
        self.sol = ctx.alloc(self.n * self.k) if kind in HAS_SOLUTION else None
        dA, db, dx = e["dA"], self.db, self.dx
        pc, outer = (cfg.split("-")[0], 2 if cfg.endswith("outer2") else 1) if cfg not in ("none", "A_D") else (None, 1)
        if kind == "cg":
            self.h = ctx.cg(dA, db, dx, e["D"] if cfg == "A_D" else None)
        elif kind == "mcg":
            self.h = ctx.mcg(dA, db, dx, K, A_D=e["D"] if cfg == "A_D" else None)
        elif kind == "mbicgstab":
            self.h = ctx.mbicgstab(dA, db, dx, K)
        elif kind == "mgmres":
            self.h = ctx.mgmres(dA, db, dx, K, restart=M)
        elif kind == "fgmres":
            self.h = ctx.fgmres(dA, db, dx, restart=M)
        elif kind == "minres":
            self.h = ctx.minres(dA, db, dx)
        elif kind == "idr":
            self.h = ctx.idr(dA, db, dx, s=S)
        else:
            self.h = ctx.stat(cfg, dA, e["D"], db, dx, e["Ls"] if cfg != "j" else None, e["Us"] if cfg != "j" else None)
            pc = None
        if pc:
            self.h.set_preconditioner(pc, outer=outer, **pc_args(e, pc))

    def load(self, b, x0):
        self.db.set(np.ravel(b))
        self.dx.set(np.ravel(x0))

    def init(self, tol):
        return np.atleast_1d(np.asarray(self.h.init(tol), dtype=np.float64)).copy()

    def iterate(self, n):
        self.h.iterate(n)

    def state(self):
        st = [self.h.status(j) for j in range(self.k)] if self.kind in LOCKSTEP else [self.h.status()]
        out = dict(iters=tuple(s[0] for s in st), conv=tuple(s[1] for s in st), hist=[np.array(s[2]) for s in st],
                   x=self.dx.to_host().reshape(self.n, self.k), sol=None)
        if self.sol is not None:
            self.ctx.init_vector(self.sol, -7.0)
            self.h.solution(self.sol)
            out["sol"] = self.sol.to_host().reshape(self.n, self.k)
        return out

    def free(self):
        self.h.free()
        for v in (self.db, self.dx, self.sol):
            if v is not None:
                v.free()


def assert_same_run(tag, r0, got, r0_ref, ref):
    assert same_bits(r0, r0_ref), f"{tag}: r0 {r0} differs from the fresh handle's {r0_ref}"
    assert got["iters"] == ref["iters"], f"{tag}: iterations {got['iters']}, the fresh handle made {ref['iters']}"
    assert got["conv"] == ref["conv"], f"{tag}: converged {got['conv']}, the fresh handle {ref['conv']}"
    for j, (h, g) in enumerate(zip(got["hist"], ref["hist"])):
        assert len(h) == len(g), f"{tag}: column {j} has {len(h)} history entries, the fresh handle {len(g)}"
        assert same_bits(h, g), f"{tag}: history of column {j} differs from the fresh handle's, first at entry " \
                                f"{int(np.argmax(h.view(np.uint64) != g.view(np.uint64)))}"
    assert same_bits(got["x"], ref["x"]), f"{tag}: x differs from the fresh handle's"
    if ref["sol"] is not None:
        assert same_bits(got["sol"], ref["sol"]), f"{tag}: solution() differs from the fresh handle's"


def assert_just_initialised(tag, r0, pre, x0):
    assert pre["iters"] == (0,) * len(r0) and pre["conv"] == (False,) * len(r0), f"{tag}: {pre['iters']} {pre['conv']} after init"
    for j, h in enumerate(pre["hist"]):
        assert len(h) == 1 and same_bits(h, r0[j:j + 1]), f"{tag}: history of column {j} after init is {h}, r0 {r0[j]}"
    assert same_bits(pre["x"], x0), f"{tag}: init changed x"
    if pre["sol"] is not None:
        assert same_bits(pre["sol"], x0), f"{tag}: solution() after init is not x0"


def second_system(n, k):
    rng = np.random.default_rng(77)
    b2 = rng.uniform(-1.0, 1.0, (n, k))
    x2 = rng.uniform(0.25, 1.0, (n, k)) * rng.choice([-1.0, 1.0], (n, k))
    return b2, x2


def first_leg(n, k, kind, cfg, leg):
    """(b, x0, tol, iterate calls) of the first solve.  The budget leg's tolerance is 0: no norm is below it, so no
    configuration converges before Q (BiCGSTAB with ILU(0) reaches 1e-16 r0 in 6 iterations)."""
    rng = np.random.default_rng(5)
    b = np.ones((n, k))
    if leg == "converged":
        if k > 1:  # columns that stop at different iterations
            b[:, 1] = rng.uniform(-1.0, 1.0, n)
            b[:, 2] = 0.0
            b[n // 2, 2] = 1.0
        return b, np.zeros((n, k)), tol_first(kind, cfg), (BUDGET,)
    if leg == "budget":
        if k > 1:  # column 2 stops at iteration 1 (b = 0 from 0), the others are live at Q
            b[:, 1] = rng.uniform(-1.0, 1.0, n)
            b[:, 2] = 0.0
        return b, np.zeros((n, k)), 0.0, (Q,)
    return np.zeros((n, k)), np.zeros((n, k)), tol_first(kind, cfg), (BUDGET,)


def fresh_run(ctx, e, kind, cfg):
    """The second system on a fresh handle with buffers of its own: computed once per configuration, shared by the legs."""
    key = (kind, cfg)
    if key not in e["fresh"]:
        k = K if kind in LOCKSTEP else 1
        b2, x2 = second_system(e["n"], k)
        s = Solve(ctx, e, kind, cfg, b2, x2)
        try:
            r0 = s.init(tol_second(kind))
            pre = s.state()
            for c in PATTERN:
                s.iterate(c)
            e["fresh"][key] = dict(r0=r0, pre=pre, post=s.state())
        finally:
            s.free()
    return e["fresh"][key]


def host_residual(A, x, b):
    """b - A x in np.longdouble"""
    rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
    Ax = np.zeros(A.n_rows, dtype=np.longdouble)
    np.add.at(Ax, rows, A.val.astype(np.longdouble) * x.astype(np.longdouble)[A.col])
    return b.astype(np.longdouble) - Ax


def recorded_norm(orc, e, kind, cfg, r):
    """The norm of the residual r (np.longdouble) that this handle's history records (include/bis_hip.h)."""
    pc = cfg.split("-")[0]
    two_norm = np.sqrt(np.sum(r * r))
    if cfg == "none" or kind not in ("mgmres", "minres"):
        return two_norm
    if pc == "j":
        return np.sqrt(np.sum(r * r / e["D"].to_host().astype(np.longdouble)))
    if "sgs" not in e["host"]:
        D = e["D"].to_host()
        e["host"]["sgs"] = (CRS(e["n"], *e["Ls"].download()), CRS(e["n"], *e["Us"].download()), D, e["Dinv"].to_host())
    Ls, Us, D, Dinv = e["host"]["sgs"]
    z = orc.apply_preconditioner("sgs", Ls, Us, D, Dinv, D, D, r.astype(np.float64)).astype(np.longdouble)
    return np.sqrt(np.sum(z * z)) if kind == "mgmres" else np.sqrt(np.sum(r * z))


def reinit_case(ctx, orc, e, kind, cfg, leg):
    tag = f"{kind}/{cfg}/{leg}/n={e['n']}"
    k = K if kind in LOCKSTEP else 1
    n = e["n"]
    b1, x1, tol1, calls = first_leg(n, k, kind, cfg, leg)
    b2, x2 = second_system(n, k)
    ref = fresh_run(ctx, e, kind, cfg)
    s = Solve(ctx, e, kind, cfg, b1, x1)
    try:
        r0_first = s.init(tol1)
        for c in calls:
            s.iterate(c)
        first = s.state()
        print(f"{tag}: first solve r0 {r0_first} iters {first['iters']} conv {first['conv']} last "
              f"{[float(h[-1]) for h in first['hist']]}")
        if leg == "converged":
            assert all(first["conv"]) and max(first["iters"]) < BUDGET, f"{tag}: the first solve did not converge"
            assert k == 1 or len(set(first["iters"])) > 1, f"{tag}: every column stopped at iteration {first['iters'][0]}"
        elif leg == "budget":
            assert not any(first["conv"]) and first["iters"][0] == Q, f"{tag}: the first solve is not live at {Q}"
            assert k == 1 or (first["iters"][1] == Q and first["iters"][2] < Q), f"{tag}: columns at {first['iters']}"
        elif kind in ZERO_RHS_PINNED:
            assert first["iters"] == (1,) * k and not any(first["conv"]) and np.all(r0_first == 0.0), tag
            assert all(len(h) == 2 and np.isnan(h[1]) for h in first["hist"]), tag
        if leg == "poisoned":
            print(f"{tag}: {int(np.sum(np.isnan(first['x'])))} of {first['x'].size} entries of the first solve's x are NaN")
        s.load(b2, x2)
        r0 = s.init(tol_second(kind))
        pre = s.state()
        assert_just_initialised(tag, r0, pre, x2)
        for c in PATTERN:
            s.iterate(c)
        post = s.state()
    finally:
        s.free()
    print(f"{tag}: second solve r0 {r0} iters {post['iters']} conv {post['conv']}; fresh handle r0 {ref['r0']} iters "
          f"{ref['post']['iters']} conv {ref['post']['conv']}")
    assert_same_run(tag + " after init", r0, pre, ref["r0"], ref["pre"])
    assert_same_run(tag, r0, post, ref["r0"], ref["post"])
    if leg == "converged":
        assert all(i2 < i1 for i1, i2 in zip(first["iters"], post["iters"])), \
            f"{tag}: the second solve ({post['iters']}) is not shorter than the first ({first['iters']})"
        for j in range(k):
            hist = post["hist"][j]
            r = host_residual(e["A"], post["x"][:, j], b2[:, j])
            res = recorded_norm(orc, e, kind, cfg, r)
            print(f"{tag}: column {j} recomputed residual {float(res):.6e} (2-norm {float(np.sqrt(np.sum(r * r))):.6e}), last "
                  f"history entry {hist[-1]:.6e}, entry 0 {hist[0]:.6e}")
            assert res <= np.longdouble(hist[-1]) + np.longdouble(1e-10) * np.longdouble(hist[0]), \
                f"{tag}: column {j}: residual {float(res)} of the returned x above the last history entry {hist[-1]}"


# ---- A. init again gives the bits of a fresh handle ----------------------------------------------------------------------

@pytest.mark.parametrize("leg", ["converged", "budget", "poisoned"])
@pytest.mark.parametrize("kind,cfg", CASES)
def test_init_again_gives_the_bits_of_a_fresh_handle(ctx, systems, oracle, kind, cfg, leg):
    """converged: b = 1 from x0 = 0 run past its stop (lock-step: three columns that stop at different iterations); budget:
    cut off after 7 iterations, inside a cycle, Jacobi's iterate in its second buffer (lock-step: one column already
    stopped); poisoned: b = 0 from x0 = 0, every work vector and scalar NaN.  Then the second system in the same buffers."""
    reinit_case(ctx, oracle, small_system(systems, kind), kind, cfg, leg)


@pytest.mark.parametrize("kind,cfg", WIDE_CASES)
def test_init_again_inside_a_cycle_with_both_counter_levels(ctx, systems, oracle, kind, cfg):
    """The budget stop at 8379 rows: 17 workgroups in the reductions, so the last arriver is found over two counter levels."""
    reinit_case(ctx, oracle, systems["wide"], kind, cfg, "budget")


# ---- B. two live handles on one context ---------------------------------------------------------------------------------

def stopped(state, calls):
    return all(c or it < calls or not np.isfinite(h[-1]) for c, it, h in zip(state["conv"], state["iters"], state["hist"]))


def drive_together(specs, max_rounds=300, extra=3):
    """specs: (system, kind, cfg, b, x0, tol) per handle, all on one context.  iterate(1) on each handle in turn until all
    have stopped, then `extra` rounds more.  Returns (rounds, [(r0, state)])."""
    hs = [Solve(e["ctx"], e, kind, cfg, b, x0) for e, kind, cfg, b, x0, _ in specs]
    try:
        r0s = [h.init(spec[5]) for h, spec in zip(hs, specs)]
        rounds, left = 0, None
        while left is None or left > 0:
            for h in hs:
                h.iterate(1)
            rounds += 1
            assert rounds <= max_rounds, "the handles did not stop"
            if left is None:
                if all(stopped(h.state(), rounds) for h in hs):
                    left = extra
            else:
                left -= 1
        return rounds, [(r0, h.state()) for r0, h in zip(r0s, hs)]
    finally:
        for h in hs:
            h.free()


def drive_alone(spec, rounds):
    e, kind, cfg, b, x0, tol = spec
    s = Solve(e["ctx"], e, kind, cfg, b, x0)
    try:
        r0 = s.init(tol)
        for _ in range(rounds):
            s.iterate(1)
        return r0, s.state()
    finally:
        s.free()


def rhs(n, k, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, k)), np.zeros((n, k))


@pytest.fixture()
def two_contexts():
    from basic_iterative_solvers_amd import Context
    cs = [Context(), Context()]
    yield cs
    for c in cs:
        c.close()


def test_cg_and_fgmres_share_the_triangles(two_contexts):
    """bis_cg + SGS and bis_fgmres + SGS on the same A, L, U, D (the triangles' sweep plans and scratch are shared), in turn;
    then bis_fgmres next to a bis_cg that has already stopped: a handle's stop flag must not reach the other's launches."""
    shared, alone = (make_system(c, (9, 7, 11)) for c in two_contexts)
    n = shared["n"]
    (b_cg, x_cg), (b_fg, x_fg) = rhs(n, 1, 11), rhs(n, 1, 12)
    rounds, got = drive_together([(shared, "cg", "sgs", b_cg, x_cg, 1e-8), (shared, "fgmres", "sgs", b_fg, x_fg, 1e-8)])
    ref = [drive_alone((alone, "cg", "sgs", b_cg, x_cg, 1e-8), rounds), drive_alone((alone, "fgmres", "sgs", b_fg, x_fg, 1e-8), rounds)]
    for name, (r0, st), (r0_ref, st_ref) in zip(("cg", "fgmres"), got, ref):
        print(f"{name} next to the other: iters {st['iters']} conv {st['conv']}; alone: {st_ref['iters']} {st_ref['conv']} ({rounds} rounds)")
        assert all(st_ref["conv"]), f"{name} alone did not converge"
        assert_same_run(f"{name} next to a live handle", r0, st, r0_ref, st_ref)
    # the CG has stopped (tolerance 0.5: at once) before the FGMRES makes its first step, and keeps being called
    a = Solve(shared["ctx"], shared, "cg", "sgs", b_cg, x_cg)
    f = Solve(shared["ctx"], shared, "fgmres", "sgs", b_fg, x_fg)
    try:
        a.init(0.5)
        r0 = f.init(1e-8)
        a.iterate(BUDGET)
        sa = a.state()
        print(f"the stopped CG: iters {sa['iters']} conv {sa['conv']}")
        assert all(sa["conv"]) and sa["iters"][0] < 10
        for _ in range(rounds):
            f.iterate(1)
            a.iterate(1)
        st = f.state()
        assert a.state()["iters"] == sa["iters"]
    finally:
        a.free()
        f.free()
    print(f"fgmres next to a stopped cg: iters {st['iters']} conv {st['conv']}")
    assert_same_run("fgmres next to a stopped handle", r0, st, *ref[1])


def test_mcg_and_minres_of_different_sizes(two_contexts):
    """bis_mcg (3 columns, 693 rows) created first, then bis_minres on 8379 rows: the context's partial-sum buffer is sized by
    whoever asks for more, while the smaller handle is live."""
    small, wide = make_system(two_contexts[0], (9, 7, 11)), make_system(two_contexts[0], (21, 21, 19))
    small_alone, wide_alone = make_system(two_contexts[1], (9, 7, 11)), make_system(two_contexts[1], (21, 21, 19))
    (B, X), (b, x) = rhs(small["n"], K, 21), rhs(wide["n"], 1, 22)
    rounds, got = drive_together([(small, "mcg", "none", B, X, 1e-8), (wide, "minres", "none", b, x, 1e-8)])
    ref = [drive_alone((small_alone, "mcg", "none", B, X, 1e-8), rounds), drive_alone((wide_alone, "minres", "none", b, x, 1e-8), rounds)]
    for name, (r0, st), (r0_ref, st_ref) in zip(("mcg", "minres"), got, ref):
        print(f"{name} next to the other: iters {st['iters']} conv {st['conv']}; alone: {st_ref['iters']} {st_ref['conv']} ({rounds} rounds)")
        assert all(st_ref["conv"]), f"{name} alone did not converge"
        assert_same_run(f"{name} next to a live handle", r0, st, r0_ref, st_ref)


# ---- C. plain kernels after a stop ---------------------------------------------------------------------------------------

def test_plain_kernels_compute_after_a_handle_has_stopped(ctx, systems):
    """bis_spmv, both sweeps, the SGS apply, bis_spmm and bis_sptrsm into NaN-filled outputs, before any handle exists and with
    converged handles alive (bis_cg + SGS: the SpMV and the sweeps looked at its stop flag; bis_mcg + SGS: the SpMM and the
    multi-vector sweeps): the same bits.  A stop flag left in the context would leave the NaNs in place."""
    e = systems["spd"]
    n = e["n"]
    rng = np.random.default_rng(31)
    v, V = ctx.upload(rng.uniform(-1, 1, n)), ctx.upload(rng.uniform(-1, 1, n * K))
    out, OUT, tmp, work = ctx.alloc(n), ctx.alloc(n * K), ctx.alloc(n), ctx.alloc(n)

    def calls():
        res = {}
        for name, fn, o in (("spmv", lambda: ctx.spmv(e["dA"], v, out), out),
                            ("sptrsv", lambda: ctx.sptrsv(e["Ls"], out, e["D"], v), out),
                            ("bsptrsv", lambda: ctx.bsptrsv(e["Us"], out, e["D"], v), out),
                            ("apply sgs", lambda: ctx.apply_preconditioner("sgs", n, e["Ls"], e["Us"], e["D"], e["Dinv"], e["D"], e["D"],
                                                                             out, v, tmp, work), out),
                            ("spmm", lambda: ctx.spmm(e["dA"], V, OUT, K), OUT),
                            ("sptrsm", lambda: ctx.sptrsm(e["Ls"], OUT, e["D"], V, K), OUT)):
            o.set(np.full(o.n, np.nan))
            tmp.set(np.full(n, np.nan))
            work.set(np.full(n, np.nan))
            fn()
            res[name] = o.to_host()
        return res

    before = calls()
    assert all(np.all(np.isfinite(r)) for r in before.values())
    b, x0 = np.ones((n, 1)), np.zeros((n, 1))
    hs = [Solve(ctx, e, "cg", "sgs", b, x0), Solve(ctx, e, "mcg", "sgs", np.ones((n, K)), np.zeros((n, K)))]
    try:
        for h in hs:
            h.init(1e-8)
            h.iterate(BUDGET)
            st = h.state()
            print(f"{h.kind}: iters {st['iters']} conv {st['conv']}")
            assert all(st["conv"]) and max(st["iters"]) < BUDGET
        after = calls()
    finally:
        for h in hs:
            h.free()
    for u in (v, V, out, OUT, tmp, work):
        u.free()
    for name in before:
        print(f"{name}: {int(np.sum(np.isnan(after[name])))} NaN of {after[name].size} after the stop")
        assert same_bits(after[name], before[name]), f"{name} after a handle has stopped differs from the call before it"


# ---- D. set_preconditioner on an initialised handle ----------------------------------------------------------------------

@pytest.mark.parametrize("kind", [k for k in CONFIGS if k != "stat"])
def test_set_preconditioner_is_refused_after_init(ctx, systems, kind):
    """include/bis_hip.h: every handle family with a set_preconditioner refuses it once init has run (bis_stat has none)."""
    from basic_iterative_solvers_amd import BisError
    e = small_system(systems, kind)
    k = K if kind in LOCKSTEP else 1
    s = Solve(ctx, e, kind, "none", np.ones((e["n"], k)), np.zeros((e["n"], k)))
    try:
        s.init(1e-8)
        with pytest.raises(BisError, match=f"bis_{kind}_set_preconditioner: call it before bis_{kind}_init / bis_{kind}_iterate"):
            s.h.set_preconditioner("sgs", **pc_args(e, "sgs"))
    finally:
        s.free()
