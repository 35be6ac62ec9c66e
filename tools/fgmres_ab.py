#!/usr/bin/env python3
"""Time the flexible GMRES handle (bis_fgmres_*, the CLI's -fgm) against what it is measured by -- per input in ONE process on
ONE allocation of the matrix, the preconditioner's operands and the vectors, the legs alternating round by round, five rounds.
   python tools/fgmres_ab.py [INPUT ...] [--iters 20] [--restart 10] [--tol 1e-8] [--json FILE]
INPUT is generator@preconditioner.
  * generator@gs | ilu0 | none: FGMRES(m), init + `iters` iterations with tol 0, against the CLI's -gm with device scalars on
    the same column: GMRES(m) from the single-vector device-scalar calls with one download of the Hessenberg column per
    iteration and the Givens algebra on the host (tools/mgmres_ab.py's Single: host/methods/gmres.hpp's
    orthogonalize_V_dev).  Defaults: anderson:256,shift=9@gs (config 4), unstr:80,80,80@ilu0, hpcg:256@none.
  * generator@mg: whole solves to `tol` with a status read every 8 iterations, as the CLI enqueues them: FGMRES(m) with one
    K-cycle per step against the CG handle (bis_cg_*) with the K-cycle and with the V-cycle of the same hierarchy
    parameters.  Default: hpcg:256@mg.
Each input runs in a child process of its own under a time limit (a GPU step that fails or runs out of time ends the script:
nothing more is started on the device).  Reported per input: ms per leg (median and minimum over the rounds), the ratios,
iteration counts, and the history deviation between the two GMRES legs."""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mgmres_ab import Single, generate, timed  # noqa: E402

DEFAULT = ["anderson:256,shift=9@gs", "unstr:80,80,80@ilu0", "hpcg:256@none", "hpcg:256@mg"]
STEP_LIMIT = 420  # seconds per input


def gmres_legs(ctx, A, gen, pc, iters, m):
    import numpy as np
    n = A.n_rows
    if pc == "ilu0":
        Ls, LD, Us, UD = ctx.ilu0(A)
        ops = (Ls, Us, LD, LD, LD, UD)
    else:
        Ls, Us, D, Dinv = ctx.split_strict(A)
        ops = (Ls, Us, D, Dinv, D, D)
    kw = dict(Ls=ops[0], Us=ops[1], A_D=ops[2], A_D_inv=ops[3], L_D=ops[4], U_D=ops[5])
    b = ctx.upload(np.random.default_rng(1).uniform(-1, 1, n))
    single = Single(ctx, A, pc, ops, b, ctx.alloc(n), m)
    x = ctx.alloc(n)
    s = ctx.fgmres(A, b, x, restart=m)
    if pc != "none":
        s.set_preconditioner(pc, **kw)
    got = {}

    def fgm():
        ctx.init_vector(x, 0.0)
        s.init(0.0)  # tol 0: nothing stops
        s.iterate(iters)

    def gm():
        got["hist"] = single.solve(iters)

    times = timed(ctx, [("fgmres", fgm), ("gm device scalars", gm)])
    med = {q: float(np.median(v)) for q, v in times.items()}
    it, _, hist = s.status()
    # without a preconditioner the two are the same iteration; with one the histories are of different residuals
    dev = float(np.max(np.abs(hist - np.array(got["hist"])[:len(hist)])) / hist[0]) if pc == "none" else None
    rec = dict(input=gen, preconditioner=pc, rows=n, nnz=A.nnz, restart=m, iters=iters, iters_done=it, hist_entries=len(hist),
               hist_dev_vs_gm=dev, spmv_kernel=A.spmv_kernel(), sweep_kernels=[ops[0].sweep_kernel(False), ops[1].sweep_kernel(True)],
               median_ms=med, min_ms={q: float(np.min(v)) for q, v in times.items()},
               ratio_gm_over_fgmres=med["gm device scalars"] / med["fgmres"], rounds=times,
               note="init + `iters` iterations per call; the gm leg downloads one Hessenberg column per iteration")
    print(f"{gen}@{pc}: fgmres {med['fgmres']:.3f} ms, gm with device scalars {med['gm device scalars']:.3f} ms for init + {iters} "
          f"iterations of GMRES({m}) (done {it}) [{rec['spmv_kernel']}; {', '.join(rec['sweep_kernels'])}]; ratio gm / fgmres "
          f"{rec['ratio_gm_over_fgmres']:.2f}" + (f"; history deviation {dev:.2e}" if dev is not None else ""), flush=True)
    s.free()
    return rec


def mg_legs(ctx, A, gen, tol, m, budget=400):
    import numpy as np
    n = A.n_rows
    b, x = ctx.upload(np.ones(n)), ctx.alloc(n)
    mgs = {c: ctx.mg(A, cycle=c) for c in ("k", "v")}
    fg = ctx.fgmres(A, b, x, restart=m)
    fg.set_preconditioner(mgs["k"])
    cgs = {}
    for c in ("k", "v"):
        cgs[c] = ctx.cg(A, b, x)
        cgs[c].set_preconditioner("mg", Ls=mgs[c].operand)
    got = {}

    def solve(name, s):
        def run():
            ctx.init_vector(x, 0.0)
            s.init(tol)
            enq = 0
            while enq < budget:
                s.iterate(8)
                enq += 8
                st = s.status(hist_cap=1)
                if st[0] < enq:
                    break
            got[name] = (st[0], st[1])
        return run

    legs = [("fgmres mg k", solve("fgmres mg k", fg)), ("cg mg k", solve("cg mg k", cgs["k"])), ("cg mg v", solve("cg mg v", cgs["v"]))]
    times = timed(ctx, legs)
    med = {q: float(np.median(v)) for q, v in times.items()}
    rec = dict(input=gen, preconditioner="mg", rows=n, nnz=A.nnz, restart=m, tol=tol, hierarchy_rows=mgs["k"].rows,
               iterations={q: got[q][0] for q in got}, converged={q: got[q][1] for q in got}, median_ms=med,
               min_ms={q: float(np.min(v)) for q, v in times.items()}, rounds=times,
               ratio_cg_k_over_fgmres=med["cg mg k"] / med["fgmres mg k"], ratio_cg_v_over_fgmres=med["cg mg v"] / med["fgmres mg k"],
               note="whole solves from x = 0 to tol, a status read every 8 iterations")
    print(f"{gen}@mg (rows {rec['hierarchy_rows']}), solves to {tol:g}: " +
          ", ".join(f"{q} {med[q]:.3f} ms / {got[q][0]} iterations{'' if got[q][1] else ' NOT CONVERGED'}" for q in med) +
          f"; ratio cg k / fgmres {rec['ratio_cg_k_over_fgmres']:.2f}, cg v / fgmres {rec['ratio_cg_v_over_fgmres']:.2f}", flush=True)
    return rec


def run_input(spec, iters, m, tol):
    from basic_iterative_solvers_amd import Context
    ctx = Context(0)
    gen, _, pc = spec.partition("@")
    pc = pc or "none"
    A = generate(ctx, gen)
    rec = mg_legs(ctx, A, gen, tol, m) if pc == "mg" else gmres_legs(ctx, A, gen, pc, iters, m)
    info = ctx.device_info()
    ctx.close()
    return dict(device=info, records=[rec])


def main():
    argv = sys.argv[1:]

    def opt(name, default):
        return argv[argv.index(name) + 1] if name in argv else default

    json_out = opt("--json", None)
    iters, m, tol = int(opt("--iters", 20)), int(opt("--restart", 10)), float(opt("--tol", 1e-8))
    taken = {argv[i + 1] for i, a in enumerate(argv[:-1]) if a in ("--json", "--iters", "--restart", "--tol")}
    specs = [a for a in argv if not a.startswith("--") and a not in taken] or DEFAULT
    if "--child" in argv:  # one input, in this process
        out = run_input(specs[0], iters, m, tol)
        if json_out:
            with open(json_out, "w") as f:
                json.dump(out, f, indent=1)
        return 0
    # one child per input, each GPU step under its own time limit; a failing step ends the script
    merged = dict(device=None, records=[])
    for i, spec in enumerate(specs):
        part = f"{json_out}.{i}.part" if json_out else None
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--child", spec,
               "--iters", str(iters), "--restart", str(m), "--tol", repr(tol)]
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
