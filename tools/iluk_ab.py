#!/usr/bin/env python3
"""Time ILU(K) with level-of-fill (bis_mat_iluk, the CLI's -fill K) for K = 0..3 -- per input in ONE process on ONE
allocation of the matrix and the vectors, the legs alternating round by round.
   python tools/iluk_ab.py [INPUT ...] [--levels 0,1,2,3] [--rounds 3] [--inner 3] [--max-iters 2000] [--limit 420] [--json FILE]
INPUT is a generator, "/rcm" appended for the RCM-ordered matrix; defaults: fem:80,80,81, unstr:80,80,80, unstr:80,80,80/rcm
and hpcg:128.  Per input and level:
  (a) setup: the symbolic phase alone (bis_mat_iluk_symbolic) and the whole factorisation (bis_mat_iluk), ms; numeric = the
      difference.  Level 0 is bis_mat_ilu0 and has no symbolic phase.
  (b) fill: entries added to A's pattern, and L + U + D entries over A's.
  (c) one apply of "ilu0" (two exact sweeps) and of "ilu0it" (--inner Jacobi-Richardson steps per triangle, fp64 values and
      values rounded to fp32), 10 applies per timed call.
  (d) fused CG to 1e-8 r0 (a status read every 25 iterations) with each of the three: iterations and ms per solve.
Each input runs in a child process of its own under a time limit (a GPU step that fails or runs out of time ends the script:
nothing more is started on the device)."""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fsai_ab import generate, summary, timed  # noqa: E402

DEFAULT = ["fem:80,80,81", "unstr:80,80,80", "unstr:80,80,80/rcm", "hpcg:128"]
STEP_LIMIT = 420  # seconds per input (--limit)
APPLIES = 10
CHUNK = 25
TOL = 1e-8


def run_input(spec, levels, rounds, inner, max_iters):
    import numpy as np
    from basic_iterative_solvers_amd import Context
    ctx = Context(0)
    A = generate(ctx, spec)
    n = A.n_rows
    rec = dict(input=spec, rows=n, nnz=A.nnz, rounds_per_leg=rounds, inner=inner, levels={})
    b, x = ctx.upload(np.random.default_rng(1).uniform(-1, 1, n)), ctx.alloc(n)  # (A 1 is an eigenvector of the fem operators)
    out, tmp, work = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
    from basic_iterative_solvers_amd import BisError
    for k in levels:
        r = dict()
        try:  # a level the library refuses for this input (a row beyond the search table, no memory) is named and left out
            for v in ctx.iluk(A, k)[:4]:
                v.free()
        except BisError as e:
            rec["levels"][str(k)] = dict(not_built=str(e))
            print(f"{spec} K={k}: not built ({e}); the level is left out", flush=True)
            continue

        def whole():
            for v in ctx.iluk(A, k)[:4]:
                v.free()

        def symbolic():
            ctx.iluk_symbolic(A, k)[0].free()

        legs = [("iluk", whole)] + ([("symbolic", symbolic)] if k > 0 else [])
        r["setup"] = summary(timed(ctx, legs, rounds))
        m = r["setup"]["median_ms"]
        Ls, L_D, Us, U_D, n_fill = ctx.iluk(A, k)
        Uinv = ctx.alloc(n)
        ctx.elemwise_div_vectors(Uinv, L_D, U_D)
        # the same factors rounded to fp32 for the SpMV-shaped solves
        Ls32, L_D32, Us32, U_D32, _ = ctx.iluk(A, k)
        r["round_f32_change"] = max(Ls32.round_f32(), Us32.round_f32())
        entries = Ls.nnz + Us.nnz + n
        r.update(n_fill=n_fill, entries=entries, over_A=entries / A.nnz, numeric_kernel=Ls.ilu0_kernel(), symbolic_kernel=Ls.iluk_kernel())
        print(f"{spec} K={k} (a) setup {m['iluk']:.1f} ms" + (f" (symbolic {m['symbolic']:.1f}, numeric {m['iluk'] - m['symbolic']:.1f})" if k else "") +
              f"; (b) {n_fill} fill entries, L+U+D = {entries} ({r['over_A']:.2f} x A); {r['numeric_kernel']}", flush=True)
        kw = dict(ilu0=("ilu0", dict(Ls=Ls, Us=Us, A_D=L_D, A_D_inv=Uinv, L_D=L_D, U_D=U_D)),
                  ilu0it=("ilu0it", dict(Ls=Ls, Us=Us, A_D=L_D, A_D_inv=Uinv, L_D=L_D, U_D=U_D, inner=inner)),
                  ilu0it_f32=("ilu0it", dict(Ls=Ls32, Us=Us32, A_D=L_D, A_D_inv=Uinv, L_D=L_D, U_D=U_D, inner=inner)))

        def apply_leg(pc, a):
            def f():
                for _ in range(APPLIES):
                    ctx.apply_preconditioner(pc, n, a["Ls"], a["Us"], a["A_D"], a["A_D_inv"], a["L_D"], a["U_D"], out, b, tmp, work,
                                             inner=a.get("inner", 0))
            return f

        r["apply"] = summary(timed(ctx, [(q, apply_leg(*kw[q])) for q in kw], rounds), per=APPLIES)
        r["forward_sweep"] = Ls.sweep_kernel()
        print(f"{spec} K={k} (c) one apply: " + ", ".join(f"{q} {r['apply']['median_ms'][q]:.3f} ms" for q in kw), flush=True)
        got, handles, legs = {}, [], []

        def solve_leg(s, key):
            def f():
                ctx.init_vector(x, 0.0)
                s.init(TOL)
                done = 0
                while done < max_iters:
                    s.iterate(CHUNK)
                    done += CHUNK
                    iters, conv, hist = s.status()
                    if conv or iters < done:
                        break
                got[key] = dict(iters=iters, converged=conv, last_over_r0=float(hist[-1] / hist[0]))
            return f

        for q, (pc, a) in kw.items():
            s = ctx.cg(A, b, x)
            s.set_preconditioner(pc, **a)
            handles.append(s)
            legs.append((q, solve_leg(s, q)))
        r["solve_cg"] = summary(timed(ctx, legs, rounds))
        r["solve_cg"]["result"] = got
        print(f"{spec} K={k} (d) -cg to {TOL:g} r0: " + ", ".join(
            f"{q} {got[q]['iters']} it {'conv' if got[q]['converged'] else 'NOT conv'} {r['solve_cg']['median_ms'][q]:.1f} ms" for q in kw), flush=True)
        for h in handles + [Ls, L_D, Us, U_D, Uinv, Ls32, L_D32, Us32, U_D32]:
            h.free()
        rec["levels"][str(k)] = r
    info = ctx.device_info()
    ctx.close()
    return dict(device=info, records=[rec])


def main():
    argv = sys.argv[1:]

    def opt(name, default):
        return argv[argv.index(name) + 1] if name in argv else default

    json_out = opt("--json", None)
    levels, rounds, inner, max_iters = opt("--levels", "0,1,2,3"), int(opt("--rounds", 3)), int(opt("--inner", 3)), int(opt("--max-iters", 2000))
    limit = int(opt("--limit", STEP_LIMIT))
    taken = {argv[i + 1] for i, a in enumerate(argv[:-1]) if a in ("--json", "--levels", "--rounds", "--inner", "--max-iters", "--limit")}
    specs = [a for a in argv if not a.startswith("--") and a not in taken] or DEFAULT
    if "--child" in argv:  # one input, in this process
        out = run_input(specs[0], [int(v) for v in levels.split(",")], rounds, inner, max_iters)
        if json_out:
            with open(json_out, "w") as f:
                json.dump(out, f, indent=1)
        return 0
    # one child per input, each GPU step under its own time limit; a failing step ends the script
    merged = dict(device=None, records=[])
    for i, spec in enumerate(specs):
        part = f"{json_out}.{i}.part" if json_out else None
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", spec, "--levels", levels,
               "--rounds", str(rounds), "--inner", str(inner), "--max-iters", str(max_iters)]
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
            with open(json_out, "w") as f:
                json.dump(merged, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
