#!/usr/bin/env python3
"""Time the FSAI preconditioner (bis_mat_fsai, "fsai") against the sweep-based ones -- per input in ONE process on ONE
allocation of the matrix, the preconditioners' operands and the vectors, the legs alternating round by round, five rounds.
   python tools/fsai_ab.py [INPUT ...] [--parts a,b,c,d] [--rounds 5] [--max-iters 2000] [--json FILE]
INPUT is generator[/order]: hpcg:256, fem:80,80,81, unstr:80,80,80 and unstr:80,80,80/rcm are the defaults; each runs in a
child process of its own under a time limit (a GPU step that fails or runs out of time ends the script: nothing more is
started on the device).  Reported per input:
  (a) setup: bis_mat_fsai against bis_mat_ilu0, ms per call, with the kernel instance of each;
  (b) one apply of fsai against sgs, ilu0 and ilu0it (inner 3), ms (10 applies per timed call), with the SpMV forms G and Gt
      resolved to (bis_mat_spmv_stream_info's form number and the kernel's name);
  (c) iterations and ms of a solve to 1e-10 r0 (b = A 1, x0 = 0) with each of them: the fused CG, and BiCGSTAB as the
      lock-step solver at k = 1; a status read every 8 iterations, as the CLI does;
  (d) the lock-step CG at k = 4 with fsai against ilu0 (columns A 1 and three random ones).
--json writes the records (meant for profiles/)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT = ["hpcg:256", "fem:80,80,81", "unstr:80,80,80", "unstr:80,80,80/rcm"]
STEP_LIMIT = 540  # seconds per input
TOL = 1e-10
CHUNK = 8
APPLIES = 10
PCS = [("fsai", 0), ("sgs", 0), ("ilu0", 0), ("ilu0it", 3)]


def generate(ctx, spec):
    spec, _, order = spec.partition("/")
    kind, dims = spec.split(":")
    nums = [int(v) for v in dims.split(",") if "=" not in v]
    if kind == "hpcg":
        A = ctx.gen_hpcg(*nums)
    else:
        A = (ctx.gen_unstr if kind == "unstr" else ctx.gen_fem)(*nums)
    if order:
        B = ctx.permute(A, ctx.bfs_order(A, rcm=order == "rcm"))
        A.free()
        A = B
    return A


def timed(ctx, legs, rounds):
    """{name: [ms per call, one entry per round]}, the legs alternating inside every round (one warm-up call each first)."""
    for _, f in legs:
        f()
    ctx.sync()
    times = {name: [] for name, _ in legs}
    for _ in range(rounds):
        for name, f in legs:
            ctx.sync()
            t0 = time.perf_counter()
            f()
            ctx.sync()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return times


def summary(times, per=1):
    import numpy as np
    return dict(median_ms={q: float(np.median(v)) / per for q, v in times.items()}, min_ms={q: float(np.min(v)) / per for q, v in times.items()},
                rounds=times)


def run_input(spec, parts, rounds, max_iters):
    import numpy as np
    from basic_iterative_solvers_amd import Context
    ctx = Context(0)
    A = generate(ctx, spec)
    n = A.n_rows
    rec = dict(input=spec, rows=n, nnz=A.nnz, rounds_per_leg=rounds)
    # the operands of every type, made once
    Ls, Us, D, Dinv = ctx.split_strict(A)
    iLs, iLD, iUs, iUD = ctx.ilu0(A)
    iUinv = ctx.alloc(n)
    ctx.elemwise_div_vectors(iUinv, iLD, iUD)
    G, Gt, n_fallback = ctx.fsai(A)
    rec.update(fsai_kernel=G.fsai_kernel(), ilu0_kernel=iLs.ilu0_kernel(), fallback_rows=n_fallback, nnz_G=G.nnz)
    kw = {"fsai": dict(Ls=G, Us=Gt), "sgs": dict(Ls=Ls, Us=Us, A_D=D, A_D_inv=Dinv, L_D=D, U_D=D),
          "ilu0": dict(Ls=iLs, Us=iUs, A_D=iLD, A_D_inv=iUinv, L_D=iLD, U_D=iUD)}
    kw["ilu0it"] = kw["ilu0"]
    ones = ctx.upload(np.ones(n))
    b, x = ctx.alloc(n), ctx.alloc(n)
    ctx.spmv(A, ones, b)

    if "a" in parts:
        def setup_fsai():
            g, gt, _ = ctx.fsai(A)
            g.free(); gt.free()

        def setup_ilu0():
            l, ld, u, ud = ctx.ilu0(A)
            for v in (l, ld, u, ud):
                v.free()

        rec["setup"] = summary(timed(ctx, [("fsai", setup_fsai), ("ilu0", setup_ilu0)], rounds))
        m = rec["setup"]["median_ms"]
        print(f"{spec} (a) setup: fsai {m['fsai']:.2f} ms [{rec['fsai_kernel']}, {n_fallback} fallback rows], ilu0 {m['ilu0']:.2f} ms "
              f"[{rec['ilu0_kernel']}]", flush=True)

    if "b" in parts:
        out, tmp, work = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)

        def apply_leg(pc, inner):
            o = kw[pc]
            ops = (o.get("Ls"), o.get("Us"), o.get("A_D"), o.get("A_D_inv"), o.get("L_D"), o.get("U_D"))

            def f():
                for _ in range(APPLIES):
                    ctx.apply_preconditioner(pc, n, *ops, out, b, tmp, work, inner=inner)
            return f

        rec["apply"] = summary(timed(ctx, [(pc, apply_leg(pc, inner)) for pc, inner in PCS], rounds), per=APPLIES)
        rec["apply"]["spmv_forms"] = dict(G=[G.spmv_stream_info()[3], G.spmv_kernel()], Gt=[Gt.spmv_stream_info()[3], Gt.spmv_kernel()],
                                          A=[A.spmv_stream_info()[3], A.spmv_kernel()])
        rec["apply"]["sweep_kernels"] = dict(sgs=[Ls.sweep_kernel(False), Us.sweep_kernel(True)], ilu0=[iLs.sweep_kernel(False), iUs.sweep_kernel(True)])
        m = rec["apply"]["median_ms"]
        print(f"{spec} (b) one apply: " + ", ".join(f"{pc} {m[pc]:.3f} ms" for pc, _ in PCS) +
              f"; G form {rec['apply']['spmv_forms']['G']}, Gt form {rec['apply']['spmv_forms']['Gt']}", flush=True)
        for v in (out, tmp, work):
            v.free()

    def solve_leg(s, xs, status, got, key):
        """s: a solver handle on (A, b, xs); runs it from x0 = 0 to TOL or max_iters, a status read every CHUNK iterations."""
        def f():
            ctx.init_vector(xs, 0.0)
            s.init(TOL)
            done = 0
            while done < max_iters:
                s.iterate(CHUNK)
                done += CHUNK
                st = status()
                if all(q[1] for q in st) or all(q[0] < done for q in st):
                    break
            got[key] = dict(iters=[q[0] for q in st], converged=[q[1] for q in st],
                            last_over_r0=[float(q[2][-1] / q[2][0]) if len(q[2]) else 0.0 for q in st])
        return f

    if "c" in parts:
        rec["solve"] = {}
        for solver in ("cg", "bi"):
            handles, legs, got = [], [], {}
            for pc, inner in PCS:
                if solver == "cg":
                    s = ctx.cg(A, b, x)
                    status = lambda s=s: [s.status()]
                else:
                    s = ctx.mbicgstab(A, b, x, 1)
                    status = lambda s=s: [s.status(0)]
                s.set_preconditioner(pc, inner=inner, **kw[pc])
                handles.append(s)
                legs.append((pc, solve_leg(s, x, status, got, pc)))
            r = summary(timed(ctx, legs, rounds))
            r["result"] = got
            rec["solve"][solver] = r
            print(f"{spec} (c) -{solver} to {TOL:g} r0: " + ", ".join(
                f"{pc} {got[pc]['iters'][0]} it {'conv' if got[pc]['converged'][0] else 'NOT conv'} {r['median_ms'][pc]:.1f} ms" for pc, _ in PCS), flush=True)
            for s in handles:
                s.free()

    if "d" in parts:
        k = 4
        rng = np.random.default_rng(1)
        Bk, Xk, col = ctx.alloc(n * k), ctx.alloc(n * k), ctx.alloc(n)
        ctx.mvec_set_col(Bk, n, k, 0, b)
        for j in range(1, k):
            col.set(rng.uniform(-1, 1, n))
            ctx.mvec_set_col(Bk, n, k, j, col)
        handles, legs, got = [], [], {}
        for pc in ("fsai", "ilu0"):
            s = ctx.mcg(A, Bk, Xk, k)
            s.set_preconditioner(pc, **kw[pc])
            handles.append(s)
            legs.append((pc, solve_leg(s, Xk, lambda s=s: [s.status(j) for j in range(k)], got, pc)))
        r = summary(timed(ctx, legs, rounds))
        r["result"] = got
        r["spmm_kernels"] = dict(A=A.spmm_kernel(), G=G.spmm_kernel(), Gt=Gt.spmm_kernel())
        rec["mcg_k4"] = r
        print(f"{spec} (d) MCG k=4 to {TOL:g} r0: " + ", ".join(
            f"{pc} {got[pc]['iters']} it conv {got[pc]['converged']} {r['median_ms'][pc]:.1f} ms" for pc in ("fsai", "ilu0")), flush=True)
        for s in handles:
            s.free()

    info = ctx.device_info()
    ctx.close()
    return dict(device=info, records=[rec])


def main():
    argv = sys.argv[1:]

    def opt(name, default):
        return argv[argv.index(name) + 1] if name in argv else default

    json_out = opt("--json", None)
    parts = opt("--parts", "a,b,c,d")
    rounds = int(opt("--rounds", 5))
    max_iters = int(opt("--max-iters", 2000))
    taken = {argv[argv.index(q) + 1] for q in ("--json", "--parts", "--rounds", "--max-iters") if q in argv}
    child = "--child" in argv
    specs = [a for a in argv if not a.startswith("--") and a not in taken] or DEFAULT
    if child:  # one input, in this process
        out = run_input(specs[0], parts.split(","), rounds, max_iters)
        if json_out:
            with open(json_out, "w") as f:
                json.dump(out, f, indent=1)
        return 0
    # one child per input, each GPU step under its own time limit; a failing step ends the script
    merged = dict(device=None, records=[])
    for i, spec in enumerate(specs):
        part = f"{json_out}.{i}.part" if json_out else None
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--child", spec,
               "--parts", parts, "--rounds", str(rounds), "--max-iters", str(max_iters)]
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
            with open(json_out, "w") as f:  # (kept up to date input by input)
                json.dump(merged, f, indent=1)
    if json_out:
        with open(json_out, "w") as f:
            json.dump(merged, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
