#!/usr/bin/env python3
"""Time the MINRES handle (bis_minres_*, the CLI's -mr) against what it is measured by -- per input in ONE process on ONE
allocation of the matrix and the vectors, the legs alternating round by round, five rounds.
   python tools/minres_ab.py [INPUT ...] [--iters 100] [--json FILE]
INPUT is generator@leg.
  * generator@cg: time per iteration of MINRES against the fused CG (bis_cg_*), both unpreconditioned with tol 0 (nothing
    stops), `iters` iterations enqueued after an untimed init.  By bytes the ratio should be near
    (12 nnz + 120 N) / (12 nnz + 92 N) with 8-byte values; the record carries that figure next to the measured one.
    Defaults: hpcg:256@cg, anderson:256,shift=9@cg.
  * generator@gm: init + `iters` iterations of MINRES on an indefinite matrix against GMRES(10) from the single-vector
    device-scalar calls (the CLI's -gm schedule: tools/mgmres_ab.py's Single) and against bis_fgmres_* with restart 10.
    Iterations are timed, not solves: how many such a system needs at this size is not known.
    Default: anderson:256,shift=6.5@gm.
Each input runs in a child process of its own under a time limit (a GPU step that fails or runs out of time ends the script:
nothing more is started on the device).  Reported per input: ms per leg (median and minimum over the rounds) and the ratios."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mgmres_ab import ROUNDS, Single, generate, timed  # noqa: E402

DEFAULT = ["hpcg:256@cg", "anderson:256,shift=9@cg", "anderson:256,shift=6.5@gm"]
STEP_LIMIT = 420  # seconds per input


class Unpreconditioned(Single):
    """tools/mgmres_ab.py's device-scalar GMRES(m) with M = I: the apply does nothing."""

    def apply(self, v):
        pass


def cg_legs(ctx, A, gen, iters):
    import numpy as np
    n = A.n_rows
    b, x = ctx.upload(np.random.default_rng(1).uniform(-1, 1, n)), ctx.alloc(n)
    solvers = {"minres": ctx.minres(A, b, x), "cg": ctx.cg(A, b, x)}

    def run(s):  # the iterations alone: init is blocking and stays outside
        ctx.init_vector(x, 0.0)
        s.init(0.0)
        ctx.sync()
        t0 = time.perf_counter()
        s.iterate(iters)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / iters

    for s in solvers.values():
        run(s)
    times = {q: [] for q in solvers}
    for _ in range(ROUNDS):
        for q, s in solvers.items():
            times[q].append(run(s))
    med = {q: float(np.median(v)) for q, v in times.items()}
    done = {q: s.status(hist_cap=1)[0] for q, s in solvers.items()}
    model = (12.0 * A.nnz + 120.0 * n) / (12.0 * A.nnz + 92.0 * n)
    rec = dict(input=gen, leg="cg", rows=n, nnz=A.nnz, iters=iters, iters_done=done, spmv_kernel=A.spmv_kernel(),
               spmv_kernel_fused=A.spmv_kernel(fused=True), median_ms_per_iteration=med,
               min_ms_per_iteration={q: float(np.min(v)) for q, v in times.items()}, rounds=times,
               ratio_minres_over_cg=med["minres"] / med["cg"], ratio_by_bytes_8_byte_values=model)
    print(f"{gen}: minres {med['minres']:.4f} ms, fused cg {med['cg']:.4f} ms per iteration over {iters} [{rec['spmv_kernel']} / "
          f"{rec['spmv_kernel_fused']}]; ratio {rec['ratio_minres_over_cg']:.3f}, by bytes with 8-byte values {model:.3f}", flush=True)
    for s in solvers.values():
        s.free()
    return rec


def gm_legs(ctx, A, gen, iters, m=10):
    import numpy as np
    n = A.n_rows
    b, x = ctx.upload(np.random.default_rng(1).uniform(-1, 1, n)), ctx.alloc(n)
    single = Unpreconditioned(ctx, A, "none", (None,) * 6, b, ctx.alloc(n), m)
    mr, fg = ctx.minres(A, b, x), ctx.fgmres(A, b, x, restart=m)
    got = {}

    def handle(s):
        def run():
            ctx.init_vector(x, 0.0)
            s.init(0.0)
            s.iterate(iters)
        return run

    def gm():
        got["hist"] = single.solve(iters)

    times = timed(ctx, [("minres", handle(mr)), ("gm device scalars", gm), ("fgmres", handle(fg))])
    med = {q: float(np.median(v)) for q, v in times.items()}
    it, _, hist = mr.status()
    rec = dict(input=gen, leg="gm", rows=n, nnz=A.nnz, restart=m, iters=iters, minres_iters_done=it,
               minres_residual_reduction=float(hist[-1] / hist[0]), gm_residual_reduction=float(got["hist"][-1] / got["hist"][0]),
               spmv_kernel=A.spmv_kernel(), median_ms=med, min_ms={q: float(np.min(v)) for q, v in times.items()}, rounds=times,
               ratio_gm_over_minres=med["gm device scalars"] / med["minres"], ratio_fgmres_over_minres=med["fgmres"] / med["minres"],
               note="init + `iters` iterations per call; the gm leg downloads one Hessenberg column per iteration")
    print(f"{gen}: init + {iters} iterations: minres {med['minres']:.3f} ms (residual x {rec['minres_residual_reduction']:.3e}), "
          f"gm({m}) with device scalars {med['gm device scalars']:.3f} ms (x {rec['gm_residual_reduction']:.3e}), fgmres({m}) "
          f"{med['fgmres']:.3f} ms; ratios gm / minres {rec['ratio_gm_over_minres']:.2f}, fgmres / minres "
          f"{rec['ratio_fgmres_over_minres']:.2f}", flush=True)
    mr.free(); fg.free()
    return rec


def run_input(spec, iters):
    from basic_iterative_solvers_amd import Context
    ctx = Context(0)
    gen, _, leg = spec.partition("@")
    A = generate(ctx, gen)
    rec = gm_legs(ctx, A, gen, iters) if leg == "gm" else cg_legs(ctx, A, gen, iters)
    info = ctx.device_info()
    ctx.close()
    return dict(device=info, records=[rec])


def main():
    argv = sys.argv[1:]

    def opt(name, default):
        return argv[argv.index(name) + 1] if name in argv else default

    json_out = opt("--json", None)
    iters = int(opt("--iters", 100))
    taken = {argv[i + 1] for i, a in enumerate(argv[:-1]) if a in ("--json", "--iters")}
    specs = [a for a in argv if not a.startswith("--") and a not in taken] or DEFAULT
    if "--child" in argv:  # one input, in this process
        out = run_input(specs[0], iters)
        if json_out:
            with open(json_out, "w") as f:
                json.dump(out, f, indent=1)
        return 0
    # one child per input, each GPU step under its own time limit; a failing step ends the script
    merged = dict(device=None, records=[])
    for i, spec in enumerate(specs):
        part = f"{json_out}.{i}.part" if json_out else None
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--child", spec, "--iters", str(iters)]
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
