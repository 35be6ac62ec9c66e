#!/usr/bin/env python3
"""Time the 4-byte value stream ("win4", form 8) of preconditioner factors rounded with bis_mat_round_f32 against win8 on
the SAME matrix -- per input in ONE process on ONE allocation of the matrices and the vectors, the legs alternating round by
round, five rounds.
   python tools/f32_ab.py [INPUT ...] [--parts a,b,c] [--rounds 5] [--max-iters 2000] [--json FILE]
INPUT is generator[/order]: fem:80,80,81, unstr:80,80,80/rcm and hpcg:256 are the defaults (all with spmv_valdict 0); each runs
in a child process of its own under a time limit (a GPU step that fails or runs out of time ends the script: nothing more is
started on the device).  Reported per input:
  (a) bis_spmv of the rounded FSAI factors G, Gt and of the rounded ILU(0) triangles L, U: win4 at the default ring depth and
      at spmv_win8_depth 1..6 against win8 (spmv_win4 0) on the same flagged matrix, ms per product (10 per timed call), with the
      streamed bytes of both forms and what the placement search did;
  (b) one "fsai" apply and one "ilu0it" apply (inner 3) on the rounded factors, win4 against win8;
  (c) iterations and ms of a solve to 1e-10 r0 (b = A 1, x0 = 0) under the fused CG ("fsai") and BiCGSTAB ("fsai", "ilu0it"
      inner 3) with the factors as computed (fp64, win8) and rounded (win4).
win4 is always compared with win8 on the same allocation, never with itself.  --json writes the records (meant for profiles/)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT = ["fem:80,80,81", "unstr:80,80,80/rcm", "hpcg:256"]
STEP_LIMIT = 540  # seconds per input
TOL = 1e-10
CHUNK = 8
CALLS = 10
DEPTHS = (1, 2, 3, 4, 5, 6)


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
    ctx.set_option("spmv_valdict", 0)
    A = generate(ctx, spec)
    n = A.n_rows
    rec = dict(input=spec, rows=n, nnz=A.nnz, rounds_per_leg=rounds)
    # the factors twice: as computed (fp64), and rounded and flagged
    facs = {}
    for kind in ("fp64", "fp32"):
        G, Gt, _ = ctx.fsai(A)
        iLs, iLD, iUs, iUD = ctx.ilu0(A)
        iUinv = ctx.alloc(n)
        ctx.elemwise_div_vectors(iUinv, iLD, iUD)
        facs[kind] = dict(G=G, Gt=Gt, L=iLs, U=iUs, LD=iLD, UD=iUD, Uinv=iUinv)
    rec["max_rel_change"] = {q: facs["fp32"][q].round_f32() for q in ("G", "Gt", "L", "U")}
    ones = ctx.upload(np.ones(n))
    b, x, y = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
    ctx.spmv(A, ones, b)

    def with_opts(opts, f):
        def g():
            for k, v in opts.items():
                ctx.set_option(k, v)
            f()
            ctx.sync()
            for k in opts:
                ctx.set_option(k, -1)
        return g

    if "a" in parts:
        rec["spmv"] = {}
        for q in ("G", "Gt", "L", "U"):
            M = facs["fp32"][q]

            def prod(M=M):
                for _ in range(CALLS):
                    ctx.spmv(M, b, y)

            legs = [("win8", with_opts({"spmv_win4": 0}, prod)), ("win4", prod)]
            legs += [(f"win4 depth={d}", with_opts({"spmv_win8_depth": d}, prod)) for d in DEPTHS]
            r = summary(timed(ctx, legs, rounds), per=CALLS)
            r["form"] = [M.spmv_stream_info()[3], M.spmv_kernel()]
            r["bytes_win4"] = M.spmv_streamed_bytes()
            r["layout_win4"] = M.win8_layout()
            r["tuning_win4"] = M.win8_tuning()
            ctx.set_option("spmv_win4", 0)
            r["form_off"] = [M.spmv_stream_info()[3]]
            r["bytes_win8"] = M.spmv_streamed_bytes()
            r["tuning_win8"] = M.win8_tuning()
            ctx.set_option("spmv_win4", -1)
            rec["spmv"][q] = r
            m = r["median_ms"]
            print(f"{spec} (a) {q}: form {r['form']}, win8 {m['win8']:.4f} ms, win4 {m['win4']:.4f} ms (ratio {m['win4'] / m['win8']:.3f}; bytes "
                  f"{r['bytes_win4'] / max(r['bytes_win8'], 1):.3f}); depth " + ", ".join(f"{d}: {m[f'win4 depth={d}']:.4f}" for d in DEPTHS), flush=True)

    def operands(f, pc):
        if pc == "fsai":
            return dict(Ls=f["G"], Us=f["Gt"])
        return dict(Ls=f["L"], Us=f["U"], A_D=f["LD"], A_D_inv=f["Uinv"], L_D=f["LD"], U_D=f["UD"])

    if "b" in parts:
        out, tmp, work = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
        rec["apply"] = {}
        for pc, inner in (("fsai", 0), ("ilu0it", 3)):
            o = operands(facs["fp32"], pc)
            ops = (o.get("Ls"), o.get("Us"), o.get("A_D"), o.get("A_D_inv"), o.get("L_D"), o.get("U_D"))

            def f(pc=pc, ops=ops, inner=inner):
                for _ in range(CALLS):
                    ctx.apply_preconditioner(pc, n, *ops, out, b, tmp, work, inner=inner)

            r = summary(timed(ctx, [("win8", with_opts({"spmv_win4": 0}, f)), ("win4", f)], rounds), per=CALLS)
            rec["apply"][pc] = r
            m = r["median_ms"]
            print(f"{spec} (b) one {pc} apply: win8 {m['win8']:.4f} ms, win4 {m['win4']:.4f} ms (ratio {m['win4'] / m['win8']:.3f})", flush=True)
        for v in (out, tmp, work):
            v.free()

    def solve_leg(s, status, got, key):
        def f():
            ctx.init_vector(x, 0.0)
            s.init(TOL)
            done = 0
            while done < max_iters:
                s.iterate(CHUNK)
                done += CHUNK
                st = status()
                if st[1] or st[0] < done:
                    break
            got[key] = dict(iters=st[0], converged=bool(st[1]), last_over_r0=float(st[2][-1] / st[2][0]) if len(st[2]) else 0.0)
        return f

    if "c" in parts:
        rec["solve"] = {}
        for solver, pc, inner in (("cg", "fsai", 0), ("bi", "fsai", 0), ("bi", "ilu0it", 3)):
            handles, legs, got = [], [], {}
            for kind in ("fp64", "fp32"):
                if solver == "cg":
                    s = ctx.cg(A, b, x)
                    status = lambda s=s: s.status()
                else:
                    s = ctx.mbicgstab(A, b, x, 1)
                    status = lambda s=s: s.status(0)
                s.set_preconditioner(pc, inner=inner, **operands(facs[kind], pc))
                handles.append(s)
                legs.append((kind, solve_leg(s, status, got, kind)))
            r = summary(timed(ctx, legs, rounds))
            r["result"] = got
            rec["solve"][f"{solver} {pc}"] = r
            print(f"{spec} (c) -{solver} -p {pc} to {TOL:g} r0: " + ", ".join(
                f"{kind} {got[kind]['iters']} it {'conv' if got[kind]['converged'] else 'NOT conv'} {r['median_ms'][kind]:.1f} ms" for kind in ("fp64", "fp32")), flush=True)
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
    parts = opt("--parts", "a,b,c")
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
    return 0


if __name__ == "__main__":
    sys.exit(main())
