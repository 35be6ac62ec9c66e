#!/usr/bin/env python3
"""Time the aggregation multigrid preconditioner (bis_mg_create, "mg") against the single-level ones -- per input in ONE
process on ONE allocation of the matrix, the preconditioners' operands and the vectors, the legs alternating round by
round, five rounds.
   python tools/mg_ab.py [INPUT ...] [--parts a,b,c] [--rounds 5] [--max-iters 2000] [--json FILE]
INPUT is a generator string: hpcg:256, anderson:256, fem:80,80,81 and unstr:80,80,80 are the defaults; each runs in a child
process of its own under a time limit (a GPU step that fails or runs out of time ends the script: nothing more is started on
the device).  Reported per input:
  (a) setup: ms of bis_mg_create cut at 1, 2, ... levels (max_levels = k; the time of level k's coarsening is the difference
      of two neighbours), the rows, non-zeros, aggregate kind and SpMV form of every level, the operator complexity;
  (b) one apply (10 per timed call) against the sum of its own SpMVs timed alone -- per level 2 nu of them, coarse_sweeps - 1
      on the coarsest: the difference is what the vector passes cost;
  (c) iterations and ms of the fused CG to 1e-10 r0 (b = A 1, x0 = 0) with mg at coarse_scale 1.0 and 1.5 against none, sgs,
      ilu0it (inner 3) and fsai; a status read every 8 iterations, as the CLI does;
  (d) the cycles (bis_mg_set_cycle) on the same hierarchy, the same CG handle and the same vectors: V, and W, K, K-GCR on the
      first 1, 2, 3 and on all transitions (a count that covers all of them is run once, as "all") -- iterations and ms of
      the fused CG to 1e-10 r0, and one apply against the sum of its own SpMVs timed alone (the K-GCR legs are there for the
      apply's cost: its cycle is not symmetric, CG is not the method for it).  The cycle is set before the clock starts.
  (e) smoothed aggregation (bis_mg_create_smoothed) against the unsmoothed hierarchy: ms of the whole setup of either, the
      rows, non-zeros and SpMV form of every level of both, and of the first transition the two bis_spgemm calls (A P, then
      R (A P)) and the transpose timed alone, with the path each product took;
  (f) iterations and ms of the fused CG to 1e-10 r0 with the smoothed V-cycle against the unsmoothed V, W and K cycles and
      none, sgs, ilu0it (inner 3) and fsai; "best_other" names the fastest leg that is not multigrid.
  (g) the Chebyshev smoother (bis_mg_set_smoother) at equal SpMVs per cycle: l1-Jacobi at nu = m against one polynomial of degree
      m at nu = 1, m = 2, 3, with est_steps 10 and 0, on the plain and the smoothed hierarchy (and Jacobi nu = 1 beside them) --
      iterations and ms of the fused CG to 1e-10 r0, ms of one cycle (median, min and max over the rounds: the spread a
      comparison with another build has to stay inside), lambda_max per level, and ms of bis_mg_set_smoother itself.
(e), (f) and (g) run only when --parts names them.  INPUT@rcm solves the reverse Cuthill-McKee reordering of INPUT.
--json writes the records (meant for profiles/)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT = ["hpcg:256", "anderson:256", "fem:80,80,81", "unstr:80,80,80"]
STEP_LIMIT = 540  # seconds per input
TOL = 1e-10
CHUNK = 8
APPLIES = 10


def generate(ctx, spec):
    spec, _, order = spec.partition("@")
    kind, dims = spec.split(":")
    nums = [int(v) for v in dims.split(",") if "=" not in v]
    A = dict(hpcg=ctx.gen_hpcg, anderson=ctx.gen_anderson, fem=ctx.gen_fem, unstr=ctx.gen_unstr)[kind](*nums)
    if order == "rcm":  # what the CLI's -perm rcm solves: the permuted matrix has no grid hint
        B = ctx.permute(A, ctx.bfs_order(A, rcm=True))
        A.free()
        return B
    return A


def timed(ctx, legs, rounds):
    """{name: [ms per call, one entry per round]}, the legs alternating inside every round (one warm-up call each first).  A leg
    is (name, f) or (name, f, prepare): prepare() runs before the clock starts."""
    legs = [(leg[0], leg[1], leg[2] if len(leg) > 2 else None) for leg in legs]
    for _, f, prepare in legs:
        if prepare:
            prepare()
        f()
    ctx.sync()
    times = {name: [] for name, _, _ in legs}
    for _ in range(rounds):
        for name, f, prepare in legs:
            if prepare:
                prepare()
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


CYCLES = [(1, "W"), (2, "K"), (3, "K-GCR")]


def cycle_spmvs(n_levels, cycle, klev, nu=1, coarse_sweeps=4):
    """SpMVs per level of one apply: a level is visited twice as often as the one above it below a W or K transition, every
    visit costs 2 nu (coarse_sweeps - 1 on the coarsest level), and a W / K transition adds 1 / 2 on its coarse level."""
    visits, extra = [1] * n_levels, [0] * n_levels
    for t in range(n_levels - 1):
        on = cycle != 0 and t < n_levels - 2 and (klev == 0 or t < klev)
        visits[t + 1] = visits[t] * (2 if on else 1)
        if on:
            extra[t + 1] = visits[t] * (1 if cycle == 1 else 2)
    return [visits[l] * (2 * nu if l < n_levels - 1 else coarse_sweeps - 1) + extra[l] for l in range(n_levels)]


def run_input(spec, parts, rounds, max_iters):
    import numpy as np
    from basic_iterative_solvers_amd import Context
    ctx = Context(0)
    A = generate(ctx, spec)
    n = A.n_rows
    rec = dict(input=spec, rows=n, nnz=A.nnz, rounds_per_leg=rounds)
    mg = ctx.mg(A)
    mg15 = ctx.mg(A, coarse_scale=1.5)
    levels = [mg.level_matrix(l) for l in range(mg.levels)]
    rec["hierarchy"] = dict(levels=mg.levels, rows=mg.rows, nnz=mg.nnz, kinds=mg.kinds, operator_complexity=sum(mg.nnz) / max(mg.nnz[0], 1),
                            spmv_forms=[[M.spmv_stream_info()[3], M.spmv_kernel()] for M in levels])
    print(f"{spec}: {mg.levels} levels, rows {mg.rows}, operator complexity {rec['hierarchy']['operator_complexity']:.3f}, kinds {mg.kinds}", flush=True)
    ones = ctx.upload(np.ones(n))
    b, x = ctx.alloc(n), ctx.alloc(n)
    ctx.spmv(A, ones, b)

    if "a" in parts:
        def setup_leg(k):
            def f():
                ctx.mg(A, max_levels=k).free()
            return f

        rec["setup"] = summary(timed(ctx, [(f"levels<={k}", setup_leg(k)) for k in range(1, mg.levels + 1)], rounds))
        m = rec["setup"]["median_ms"]
        print(f"{spec} (a) setup, ms by max_levels: " + ", ".join(f"{k}: {m[f'levels<={k}']:.2f}" for k in range(1, mg.levels + 1)), flush=True)

    if "b" in parts:
        out = ctx.alloc(n)
        xs = [ctx.upload(np.ones(M.n_rows)) for M in levels]
        ys = [ctx.alloc(M.n_rows) for M in levels]
        count = [2 for _ in levels]  # nu = 1: the restriction's and the post-sweep's SpMV
        count[-1] = 3  # the coarsest level: coarse_sweeps - 1

        def apply_leg():
            for _ in range(APPLIES):
                mg.apply(out, b)

        def spmv_leg():
            for _ in range(APPLIES):
                for M, xv, yv, c in zip(levels, xs, ys, count):
                    for _ in range(c):
                        ctx.spmv(M, xv, yv)

        rec["apply"] = summary(timed(ctx, [("apply", apply_leg), ("spmvs_alone", spmv_leg)], rounds), per=APPLIES)
        rec["apply"]["spmvs_per_level"] = count
        m = rec["apply"]["median_ms"]
        print(f"{spec} (b) one apply {m['apply']:.3f} ms, its {sum(count)} SpMVs alone {m['spmvs_alone']:.3f} ms", flush=True)
        for v in [out] + xs + ys:
            v.free()

    if "c" in parts:
        Ls, Us, D, Dinv = ctx.split_strict(A)
        iLs, iLD, iUs, iUD = ctx.ilu0(A)
        iUinv = ctx.alloc(n)
        ctx.elemwise_div_vectors(iUinv, iLD, iUD)
        pcs = [("mg", "mg", 0, dict(Ls=mg.operand)), ("mg_scale1.5", "mg", 0, dict(Ls=mg15.operand)), ("none", None, 0, {}),
               ("sgs", "sgs", 0, dict(Ls=Ls, Us=Us, A_D=D, A_D_inv=Dinv, L_D=D, U_D=D)),
               ("ilu0it", "ilu0it", 3, dict(Ls=iLs, Us=iUs, A_D=iLD, A_D_inv=iUinv, L_D=iLD, U_D=iUD))]
        try:
            G, Gt, _ = ctx.fsai(A)
            pcs.append(("fsai", "fsai", 0, dict(Ls=G, Us=Gt)))
        except Exception as e:  # (rows longer than FSAI's limit)
            rec["fsai_refused"] = str(e)
        handles, legs, got = [], [], {}

        def solve_leg(s, key):
            def f():
                ctx.init_vector(x, 0.0)
                s.init(TOL)
                done = 0
                while done < max_iters:
                    s.iterate(CHUNK)
                    done += CHUNK
                    it, conv, hist = s.status()
                    if conv or it < done:
                        break
                got[key] = dict(iters=it, converged=conv, last_over_r0=float(hist[-1] / hist[0]) if len(hist) else 0.0)
            return f

        for key, pc, inner, kw in pcs:
            s = ctx.cg(A, b, x)
            if pc:
                s.set_preconditioner(pc, inner=inner, **kw)
            handles.append(s)
            legs.append((key, solve_leg(s, key)))
        r = summary(timed(ctx, legs, rounds))
        r["result"] = got
        rec["solve_cg"] = r
        print(f"{spec} (c) -cg to {TOL:g} r0: " + ", ".join(
            f"{k} {got[k]['iters']} it {'conv' if got[k]['converged'] else 'NOT conv'} {r['median_ms'][k]:.1f} ms" for k, *_ in pcs), flush=True)
        for s in handles:
            s.free()

    if "d" in parts:
        settings = [("V", 0, 0)]
        for cyc, cname in CYCLES:
            for klev in (1, 2, 3):
                if klev < mg.levels - 2:
                    settings.append((f"{cname} klev={klev}", cyc, klev))
            if mg.levels > 2:
                settings.append((f"{cname} all", cyc, 0))
        out = ctx.alloc(n)
        xs = [ctx.upload(np.ones(M.n_rows)) for M in levels]
        ys = [ctx.alloc(M.n_rows) for M in levels]
        s = ctx.cg(A, b, x)
        s.set_preconditioner("mg", Ls=mg.operand)
        got, counts = {}, {}

        def setter(cyc, klev):
            return lambda: mg.set_cycle(cyc, klev)

        def solve_leg(key):
            def f():
                ctx.init_vector(x, 0.0)
                s.init(TOL)
                done = 0
                while done < max_iters:
                    s.iterate(CHUNK)
                    done += CHUNK
                    it, conv, hist = s.status()
                    if conv or it < done:
                        break
                got[key] = dict(iters=it, converged=conv, last_over_r0=float(hist[-1] / hist[0]) if len(hist) else 0.0)
            return f

        def apply_leg():
            for _ in range(APPLIES):
                mg.apply(out, b)

        def spmv_leg(count):
            def f():
                for _ in range(APPLIES):
                    for M, xv, yv, c in zip(levels, xs, ys, count):
                        for _ in range(c):
                            ctx.spmv(M, xv, yv)
            return f

        solve_legs, apply_legs = [], []
        for key, cyc, klev in settings:
            counts[key] = cycle_spmvs(mg.levels, cyc, klev)
            solve_legs.append((key, solve_leg(key), setter(cyc, klev)))
            apply_legs.append((key, apply_leg, setter(cyc, klev)))
            apply_legs.append((key + " spmvs_alone", spmv_leg(counts[key])))
        r = summary(timed(ctx, solve_legs, rounds))
        r["result"] = got
        rec["cycles_solve_cg"] = r
        a = summary(timed(ctx, apply_legs, rounds), per=APPLIES)
        a["spmvs_per_level"] = counts
        rec["cycles_apply"] = a
        mg.set_cycle(0)
        for key, _, _ in settings:
            print(f"{spec} (d) {key}: -cg {got[key]['iters']} it {'conv' if got[key]['converged'] else 'NOT conv'} "
                  f"{r['median_ms'][key]:.1f} ms; one apply {a['median_ms'][key]:.3f} ms, its {sum(counts[key])} SpMVs alone "
                  f"{a['median_ms'][key + ' spmvs_alone']:.3f} ms", flush=True)
        s.free()
        for v in [out] + xs + ys:
            v.free()

    if "e" in parts or "f" in parts:
        sm = ctx.mg(A, smooth=True)
        sm_levels = [sm.level_matrix(l) for l in range(sm.levels)]
        rec["smoothed_hierarchy"] = dict(levels=sm.levels, rows=sm.rows, nnz=sm.nnz, kinds=sm.kinds,
                                         operator_complexity=sum(sm.nnz) / max(sm.nnz[0], 1),
                                         prolong_omega=[sm.prolong_omega(l) for l in range(sm.levels - 1)],
                                         nnz_P=[sm.prolongator(l).nnz for l in range(sm.levels - 1)],
                                         spmv_forms=[[M.spmv_stream_info()[3], M.spmv_kernel()] for M in sm_levels])
        print(f"{spec}: smoothed: {sm.levels} levels, rows {sm.rows}, nnz {sm.nnz}, operator complexity "
              f"{rec['smoothed_hierarchy']['operator_complexity']:.3f}", flush=True)

    if "e" in parts:
        legs = [("unsmoothed", lambda: ctx.mg(A).free()), ("smoothed", lambda: ctx.mg(A, smooth=True).free())]
        paths = {}
        if sm.levels > 1:
            P, R = sm.prolongator(0), sm.restrictor(0)
            AP = ctx.spgemm(A, P)
            paths["A P"] = AP.spgemm_kernel()

            def ap_leg():
                ctx.spgemm(A, P).free()

            def rap_leg():
                C_ = ctx.spgemm(R, AP)
                paths["R (A P)"] = C_.spgemm_kernel()
                C_.free()

            legs += [("spgemm A P", ap_leg), ("spgemm R (A P)", rap_leg), ("transpose P", lambda: P.transpose().free())]
        r = summary(timed(ctx, legs, rounds))
        r["paths"] = paths
        rec["smoothed_setup"] = r
        print(f"{spec} (e) setup ms: " + ", ".join(f"{k} {v:.2f}" for k, v in r["median_ms"].items()) + f"; paths {paths}", flush=True)
        if sm.levels > 1:
            AP.free()

    if "f" in parts:
        Ls, Us, D, Dinv = ctx.split_strict(A)
        iLs, iLD, iUs, iUD = ctx.ilu0(A)
        iUinv = ctx.alloc(n)
        ctx.elemwise_div_vectors(iUinv, iLD, iUD)
        mgw, mgk = ctx.mg(A, cycle="w"), ctx.mg(A, cycle="k")
        pcs = [("mg smoothed V", "mg", 0, dict(Ls=sm.operand)), ("mg V", "mg", 0, dict(Ls=mg.operand)), ("mg W", "mg", 0, dict(Ls=mgw.operand)),
               ("mg K", "mg", 0, dict(Ls=mgk.operand)), ("none", None, 0, {}),
               ("sgs", "sgs", 0, dict(Ls=Ls, Us=Us, A_D=D, A_D_inv=Dinv, L_D=D, U_D=D)),
               ("ilu0it", "ilu0it", 3, dict(Ls=iLs, Us=iUs, A_D=iLD, A_D_inv=iUinv, L_D=iLD, U_D=iUD))]
        try:
            G, Gt, _ = ctx.fsai(A)
            pcs.append(("fsai", "fsai", 0, dict(Ls=G, Us=Gt)))
        except Exception as e:  # (rows longer than FSAI's limit)
            rec["fsai_refused"] = str(e)
        handles, legs, got = [], [], {}

        def solve_leg_f(s, key):
            def f():
                ctx.init_vector(x, 0.0)
                s.init(TOL)
                done = 0
                while done < max_iters:
                    s.iterate(CHUNK)
                    done += CHUNK
                    it, conv, hist = s.status()
                    if conv or it < done:
                        break
                got[key] = dict(iters=it, converged=conv, last_over_r0=float(hist[-1] / hist[0]) if len(hist) else 0.0)
            return f

        for key, pc, inner, kw in pcs:
            s = ctx.cg(A, b, x)
            if pc:
                s.set_preconditioner(pc, inner=inner, **kw)
            handles.append(s)
            legs.append((key, solve_leg_f(s, key)))
        r = summary(timed(ctx, legs, rounds))
        r["result"] = got
        others = [k for k, *_ in pcs if not k.startswith("mg") and got[k]["converged"]]
        r["best_other"] = min(others, key=lambda k: r["median_ms"][k]) if others else None
        rec["smoothed_solve_cg"] = r
        print(f"{spec} (f) -cg to {TOL:g} r0: " + ", ".join(
            f"{k} {got[k]['iters']} it {'conv' if got[k]['converged'] else 'NOT conv'} {r['median_ms'][k]:.1f} ms" for k, *_ in pcs) +
            f"; best non-mg: {r['best_other']}", flush=True)
        for s in handles:
            s.free()
        mgw.free()
        mgk.free()

    if "g" in parts:
        rec["chebyshev"] = {}
        out = ctx.alloc(n)
        for hier, smooth in (("plain", False), ("smoothed", True)):
            # one hierarchy per nu; the nu = 1 one carries every Chebyshev setting in turn (set before the clock starts)
            hs = {nu: ctx.mg(A, smooth=smooth, nu=nu) for nu in (1, 2, 3)}
            solvers = {}
            for nu, h in hs.items():
                solvers[nu] = ctx.cg(A, b, x)
                solvers[nu].set_preconditioner("mg", Ls=h.operand)
            got, lmax = {}, {}

            def set_jacobi():
                if hs[1].smoother()["kind"]:
                    hs[1].set_smoother("jacobi")

            def set_cheb(m, est):
                def f():
                    hs[1].set_smoother("cheb", degree=m, est_steps=est)
                    lmax[f"cheb degree={m} est={est}"] = [hs[1].spectrum(l)["lambda_max"] for l in range(hs[1].levels)]
                return f

            def solve_leg_g(s, key):
                def f():
                    ctx.init_vector(x, 0.0)
                    s.init(TOL)
                    done = 0
                    while done < max_iters:
                        s.iterate(CHUNK)
                        done += CHUNK
                        it, conv, hist = s.status()
                        if conv or it < done:
                            break
                    got[key] = dict(iters=it, converged=conv, last_over_r0=float(hist[-1] / hist[0]) if len(hist) else 0.0)
                return f

            def apply_leg_g(h):
                def f():
                    for _ in range(APPLIES):
                        h.apply(out, b)
                return f

            settings = [("jacobi nu=1", 1, set_jacobi)]
            for m in (2, 3):
                settings.append((f"jacobi nu={m}", m, None))
                for est in (10, 0):
                    settings.append((f"cheb degree={m} est={est}", 1, set_cheb(m, est)))
            r = summary(timed(ctx, [(k, solve_leg_g(solvers[nu], k), prep) for k, nu, prep in settings], rounds))
            a = summary(timed(ctx, [(k, apply_leg_g(hs[nu]), prep) for k, nu, prep in settings], rounds), per=APPLIES)
            setup = summary(timed(ctx, [("set_smoother est=10", lambda: hs[1].set_smoother("cheb", degree=2, est_steps=10)),
                                        ("set_smoother est=0", lambda: hs[1].set_smoother("cheb", degree=2, est_steps=0))], rounds))
            rec["chebyshev"][hier] = dict(rows=hs[1].rows, nnz=hs[1].nnz, solve_cg=dict(r, result=got), apply=a, lambda_max=lmax,
                                          set_smoother=setup)
            for k, _, _ in settings:
                print(f"{spec} (g) {hier} {k}: -cg {got[k]['iters']} it {'conv' if got[k]['converged'] else 'NOT conv'} "
                      f"{r['median_ms'][k]:.2f} ms (min {r['min_ms'][k]:.2f}); one cycle {a['median_ms'][k]:.3f} ms (min {a['min_ms'][k]:.3f}, max "
                      f"{max(a['rounds'][k]) / APPLIES:.3f})" + (f"; lambda_max {['%.4f' % v for v in lmax[k]]}" if k in lmax else ""), flush=True)
            print(f"{spec} (g) {hier} set_smoother ms: " + ", ".join(f"{k} {v:.2f}" for k, v in setup["median_ms"].items()), flush=True)
            for s in solvers.values():
                s.free()
            for h in hs.values():
                h.free()
        out.free()

    if "e" in parts or "f" in parts:
        sm.free()
    info = ctx.device_info()
    mg.free()
    mg15.free()
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
    return 0


if __name__ == "__main__":
    sys.exit(main())
