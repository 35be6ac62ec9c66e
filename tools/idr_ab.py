#!/usr/bin/env python3
"""Time the IDR(s) handle (bis_idr_*, the CLI's -idr) against what it is measured by -- per input in ONE process on ONE
allocation of the matrix, the preconditioner's operands and the vectors, the legs alternating round by round, five rounds.
   python tools/idr_ab.py [INPUT ...] [--tol 1e-10] [--budget 600] [--json FILE]
   python tools/idr_ab.py --passes INPUT [--s 4] [--cycles 8] [--json FILE]
INPUT is generator[/rcm]@preconditioner (ilu0, gs or none).  Defaults: unstr:80,80,80@ilu0, unstr:80,80,80/rcm@ilu0,
fem:80,80,81@ilu0, anderson:256,shift=9@gs.
Every leg is bis_*_init + a whole solve from x = 0 to tol r0 (b uniform random, seed 1):
  * idr s=1 / 2 / 4 / 8, fgmres (GMRES(10), right-preconditioned), mbicgstab k=1: the handles, enqueued 8 iterations at a time
    with a status read in between, as the CLI does;
  * gm device scalars: the CLI's -gm, GMRES(10) from the single-vector device-scalar calls with one download of the Hessenberg
    column per iteration (tools/mgmres_ab.py's Single); its history is the PRECONDITIONED residual estimate (left
    preconditioning), so its stop is on another quantity;
  * bi call by call: the CLI's -bi from the single-vector calls with host scalars (tools/mbicgstab_ab.py's Single).
  The two call-by-call legs run the number of iterations a first, untimed solve needed to pass tol r0 (at most --budget).
Reported per input and leg: iterations (= products for IDR, FGMRES and GMRES; BiCGSTAB makes two per iteration), converged,
ms (median and minimum over the rounds) and, for the handles, || b - A x || / r0 recomputed after one more solve (the
call-by-call legs: their last history entry).
--passes: one input under `rocprofv3 --kernel-trace --stats` (a child process that runs `cycles` whole cycles of IDR(s) with
tol 0): per IDR kernel instance the mean duration and the achieved bytes per second against the byte model of DESIGN.md
(vectors moved x 8 n bytes: V 2 nc + 3 or nc + 2, U nc + 2, Q s + 1, W 2 k + 8, T 2, O s + 6).
Each input runs in a child process of its own under a time limit (a GPU step that fails or runs out of time ends the script:
nothing more is started on the device)."""
import csv, glob, json, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mbicgstab_ab import Single as BiSingle  # noqa: E402
from mgmres_ab import Single as GmSingle, generate, timed  # noqa: E402

DEFAULT = ["unstr:80,80,80@ilu0", "unstr:80,80,80/rcm@ilu0", "fem:80,80,81@ilu0", "anderson:256,shift=9@gs"]
STEP_LIMIT = 540  # seconds per input
SS = (1, 2, 4, 8)
RESTART = 10


class Bi(BiSingle):
    """BiSingle with the input's preconditioner instead of ILU(0) only."""

    def __init__(self, ctx, A, pc, ops, b, x):
        super().__init__(ctx, A, ops, b, x)
        self.pc = pc

    def apply(self, out, inp):
        self.ctx.apply_preconditioner(self.pc, self.n, *self.ops, out, inp, self.w["tmp"], self.w["work"])


def operands(ctx, A, pc):
    if pc == "ilu0":
        Ls, LD, Us, UD = ctx.ilu0(A)
        ops = (Ls, Us, LD, LD, LD, UD)
    else:
        Ls, Us, D, Dinv = ctx.split_strict(A)
        ops = (Ls, Us, D, Dinv, D, D)
    return ops, dict(Ls=ops[0], Us=ops[1], A_D=ops[2], A_D_inv=ops[3], L_D=ops[4], U_D=ops[5])


def first_below(hist, tol):
    """(iterations to pass tol hist[0], reached)"""
    for k, v in enumerate(hist):
        if k > 0 and v < tol * hist[0]:
            return k, True
    return len(hist) - 1, False


def run_input(spec, tol, budget):
    import numpy as np
    from basic_iterative_solvers_amd import Context
    ctx = Context(0)
    gen, _, pc = spec.partition("@")
    pc = pc or "none"
    A = generate(ctx, gen)
    n = A.n_rows
    ops, kw = operands(ctx, A, pc)
    b, x, res, tmp = ctx.upload(np.random.default_rng(1).uniform(-1, 1, n)), ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
    handles = {f"idr s={s}": ctx.idr(A, b, x, s) for s in SS}
    handles["fgmres"] = ctx.fgmres(A, b, x, restart=RESTART)
    handles["mbicgstab k=1"] = ctx.mbicgstab(A, b, x, 1)
    if pc != "none":
        for h in handles.values():
            h.set_preconditioner(pc, **kw)
    gm, bi = GmSingle(ctx, A, pc, ops, b, x, RESTART), Bi(ctx, A, pc, ops, b, x)
    got = {}

    def true_residual():
        ctx.compute_residual(A, x, b, res, tmp)
        return ctx.euclidean_vec_norm(res)

    def handle_leg(name, h):
        lockstep = name.startswith("mbicgstab")

        def run():
            ctx.init_vector(x, 0.0)
            r0 = h.init(tol)
            enq = 0
            while enq < budget:
                h.iterate(8)
                enq += 8
                st = h.status(0, hist_cap=1) if lockstep else h.status(hist_cap=1)
                if st[0] < enq:
                    break
            got[name] = dict(iterations=st[0], converged=bool(st[1]), r0=float(np.ravel(r0)[0]))
        return run

    def single_leg(name, single):
        k, reached = first_below(single.solve(budget), tol)  # untimed: the iterations a stop test on the host would allow

        def run():
            hist = single.solve(k)
            got[name] = dict(iterations=k, converged=reached, r0=float(hist[0]), last_entry_over_r0=float(hist[-1] / hist[0]))
        return run

    legs = [(name, handle_leg(name, h)) for name, h in handles.items()]
    legs += [("gm device scalars", single_leg("gm device scalars", gm)), ("bi call by call", single_leg("bi call by call", bi))]
    times = timed(ctx, legs)
    # || b - A x || of the handles' solves, one more (untimed) solve each: x is shared.  (The call-by-call legs rotate their
    # iterate through buffers of their own: their last history entry stands in.)
    for name, f in legs[:len(handles)]:
        f()
        got[name]["true_residual_over_r0"] = true_residual() / got[name]["r0"]
    med = {q: float(np.median(v)) for q, v in times.items()}
    rec = dict(input=gen, preconditioner=pc, rows=n, nnz=A.nnz, tol=tol, budget=budget, restart=RESTART, legs=got, median_ms=med,
               min_ms={q: float(np.min(v)) for q, v in times.items()}, rounds=times, spmv_kernel=A.spmv_kernel(),
               sweep_kernels=[ops[0].sweep_kernel(False), ops[1].sweep_kernel(True)] if pc != "none" else [],
               note="init + a whole solve from x = 0 per call; products per iteration: 1 (idr, fgmres, gm), 2 (bicgstab)")
    print(f"{gen}@{pc} ({n} rows) to {tol:g} r0 [{rec['spmv_kernel']}; {', '.join(rec['sweep_kernels'])}]:", flush=True)
    for q in med:
        g = got[q]
        end = (f"|| b - A x || = {g['true_residual_over_r0']:.2e} r0" if "true_residual_over_r0" in g else
               f"last history entry {g['last_entry_over_r0']:.2e} r0")
        print(f"  {q:18s} {g['iterations']:5d} iterations{'' if g['converged'] else ' NOT CONVERGED'}, {med[q]:10.3f} ms (min "
              f"{rec['min_ms'][q]:.3f}), {end}", flush=True)
    for h in handles.values():
        h.free()
    info = ctx.device_info()
    ctx.close()
    return dict(device=info, records=[rec])


# ---- --passes ---------------------------------------------------------------------------------------------------------
def probe(spec, s, cycles):
    """The child under the profiler: `cycles` whole cycles of IDR(s), nothing stops."""
    import numpy as np
    from basic_iterative_solvers_amd import Context
    ctx = Context(0)
    gen, _, pc = spec.partition("@")
    pc = pc or "none"
    A = generate(ctx, gen)
    n = A.n_rows
    b, x = ctx.upload(np.random.default_rng(1).uniform(-1, 1, n)), ctx.alloc(n)
    ctx.init_vector(x, 0.0)
    h = ctx.idr(A, b, x, s)
    if pc != "none":
        h.set_preconditioner(pc, **operands(ctx, A, pc)[1])
    h.init(0.0)
    h.iterate(cycles * (s + 1))
    it = h.status(hist_cap=1)[0]
    print(json.dumps(dict(rows=n, iterations=it)), flush=True)
    h.free()
    ctx.close()


def vectors_moved(name):
    """n-vectors one launch of this IDR kernel instance reads and writes (None: not an IDR pass)"""
    m = re.search(r"idr_(v|u|dots|w|o)_kernel<(\d+)(?:, (true|false))?>", name)
    if m:
        kind, k = m.group(1), int(m.group(2))
        return {"v": 2 * k + 3 if m.group(3) == "true" else k + 2, "u": k + 2, "dots": k + 1, "w": 2 * k + 8, "o": k + 6}[kind]
    return 2 if "idr_tt_kernel" in name else None


def passes(spec, s, cycles, json_out):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "r",
               "--", sys.executable, os.path.abspath(__file__), "--probe", spec, "--s", str(s), "--cycles", str(cycles)]
        out = subprocess.run(cmd, capture_output=True, text=True)
        if out.returncode != 0:
            print(out.stdout[-2000:] + out.stderr[-2000:])
            print(f"{spec}: the profiled step ended with status {out.returncode}; nothing more is started on the device", flush=True)
            return out.returncode
        info = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                rows += list(csv.DictReader(f))
    n = info["rows"]
    recs = []
    for r in rows:
        vec = vectors_moved(r["Name"])
        if vec is None:
            continue
        short = re.search(r"idr_\w+?_kernel(<[^>]*>)?", r["Name"]).group(0)
        mean_ns = float(r["AverageNs"])
        recs.append(dict(kernel=short, calls=int(r["Calls"]), mean_us=mean_ns / 1e3, vectors=vec, model_bytes=vec * 8 * n,
                         achieved_TB_per_s=vec * 8 * n / mean_ns / 1e3))
    recs.sort(key=lambda r: r["kernel"])
    print(f"{spec}, IDR({s}), {cycles} cycles, {n} rows:")
    if info["iterations"] < cycles * (s + 1):  # launches behind a stop return at once and would count as passes
        print(f"  the solve stopped after {info['iterations']} of {cycles * (s + 1)} iterations: the means below include empty launches; "
              "use fewer cycles", flush=True)
    for r in recs:
        print(f"  {r['kernel']:28s} {r['calls']:4d} calls, {r['mean_us']:9.1f} us, {r['vectors']:2d} vectors = {r['model_bytes'] / 1e6:8.1f} MB, "
              f"{r['achieved_TB_per_s']:.2f} TB/s", flush=True)
    if json_out:
        with open(json_out, "w") as f:
            json.dump(dict(input=spec, s=s, cycles=cycles, rows=n, passes=recs), f, indent=1)
    return 0


def main():
    argv = sys.argv[1:]
    valued = ("--json", "--tol", "--budget", "--s", "--cycles", "--probe", "--passes")

    def opt(name, default):
        return argv[argv.index(name) + 1] if name in argv else default

    json_out = opt("--json", None)
    tol, budget, s, cycles = float(opt("--tol", 1e-10)), int(opt("--budget", 600)), int(opt("--s", 4)), int(opt("--cycles", 8))
    if "--probe" in argv:
        probe(opt("--probe", None), s, cycles)
        return 0
    if "--passes" in argv:
        return passes(opt("--passes", None), s, cycles, json_out)
    taken = {argv[i + 1] for i, a in enumerate(argv[:-1]) if a in valued}
    specs = [a for a in argv if not a.startswith("--") and a not in taken] or DEFAULT
    if "--child" in argv:  # one input, in this process
        out = run_input(specs[0], tol, budget)
        if json_out:
            with open(json_out, "w") as f:
                json.dump(out, f, indent=1)
        return 0
    # one child per input, each GPU step under its own time limit; a failing step ends the script
    merged = dict(device=None, records=[])
    for i, spec in enumerate(specs):
        part = f"{json_out}.{i}.part" if json_out else None
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--child", spec,
               "--tol", repr(tol), "--budget", str(budget)]
        rc = subprocess.call(cmd + (["--json", part] if part else []))
        if rc != 0:
            print(f"{spec}: step ended with status {rc}; stopping, nothing more is started on the device", flush=True)
            return rc
        if part:
            with open(part) as f:
                got = json.load(f)
            os.remove(part)
            merged["device"] = got["device"]
            merged["records"] += got["records"]
    if json_out:
        with open(json_out, "w") as f:
            json.dump(merged, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
