#!/usr/bin/env python3
"""Time block Jacobi (bis_bj_*, the CLI's -p bj) -- per input in ONE process on ONE allocation of the matrix and the vectors,
the legs alternating round by round, five rounds.
   python tools/bj_ab.py [INPUT ...] [--bs 3] [--parts abc] [--max-iters 2000] [--json FILE]
INPUT is generator[@parts]; defaults: fem:80,80,81 and unstr:80,80,80 (three unknowns a node, 3 x 3 diagonal blocks), and
fem:128,128,128@ab, whose vectors are long enough that a launch does not weigh in part (b).
  (a) setup: bis_bj_create (gather, invert, symmetrise) against bis_mat_fsai and bis_mat_ilu0, ms.
  (b) one apply against its byte model 8 sum m_b^2 + 16 n, and bis_sum_vectors on the same allocation in the same run against
      its 24 n bytes (50 calls per timed call): achieved GB/s of both and their ratio -- what the apply reaches of the device's
      streaming rate.  Also the multi-vector apply at k = 4 against 8 sum m_b^2 + 16 n k.
  (c) fused CG to 1e-8 r0 (a status read every 25 iterations) with bj (symmetrised) against j, fsai and ilu0it (inner 3):
      iterations and ms per solve.
Each input runs in a child process of its own under a time limit (a GPU step that fails or runs out of time ends the script:
nothing more is started on the device)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fsai_ab import generate, summary, timed  # noqa: E402

DEFAULT = ["fem:80,80,81", "unstr:80,80,80", "fem:128,128,128@ab"]
STEP_LIMIT = 420  # seconds per input
ROUNDS = 5
APPLIES = 50
CHUNK = 25
TOL = 1e-8


def run_input(spec, bs, parts, max_iters):
    import numpy as np
    from basic_iterative_solvers_amd import Context
    ctx = Context(0)
    gen, _, own = spec.partition("@")
    parts = own or parts
    A = generate(ctx, gen)
    n = A.n_rows
    rec = dict(input=spec, rows=n, nnz=A.nnz, block_size=bs, rounds_per_leg=ROUNDS)
    bj = ctx.bjacobi(A, block_size=bs, symmetrize=True)
    n_blocks, max_block, values = bj.info()
    rec.update(n_blocks=n_blocks, max_block=max_block, stored_values=values)
    # the operands of the other types, made once; a type the library does not build for this input is left out and named
    from basic_iterative_solvers_amd import BisError
    others, rec["not_built"] = {}, {}
    if "a" in parts or "c" in parts:
        for pc, make in (("fsai", lambda: ctx.fsai(A)), ("ilu0", lambda: ctx.ilu0(A))):
            try:
                others[pc] = make()
            except BisError as e:
                rec["not_built"][pc] = str(e)
                print(f"{spec}: {pc} is not built for this input ({e}): its legs are left out", flush=True)
    ones = ctx.upload(np.ones(n))
    b, x = ctx.upload(np.random.default_rng(1).uniform(-1, 1, n)), ctx.alloc(n)  # (A 1 is an eigenvector of the fem operators)

    if "a" in parts:
        def setup_bj():
            ctx.bjacobi(A, block_size=bs, symmetrize=True).free()

        def setup_fsai():
            g, gt, _ = ctx.fsai(A)
            g.free(); gt.free()

        def setup_ilu0():
            for v in ctx.ilu0(A):
                v.free()

        legs = [("bj", setup_bj)] + [(pc, f) for pc, f in (("fsai", setup_fsai), ("ilu0", setup_ilu0)) if pc in others]
        rec["setup"] = summary(timed(ctx, legs, ROUNDS))
        m = rec["setup"]["median_ms"]
        print(f"{spec} (a) setup: " + ", ".join(f"{pc}{f'({bs})' if pc == 'bj' else ''} {m[pc]:.2f} ms" for pc, _ in legs), flush=True)

    if "b" in parts:
        k = 4
        out, Xk, Yk = ctx.alloc(n), ctx.alloc(n * k), ctx.alloc(n * k)
        ctx.init_vector(Xk, 1.0)

        def apply_leg():
            for _ in range(APPLIES):
                bj.apply(out, b)

        def mapply_leg():
            for _ in range(APPLIES):
                bj.mapply(Yk, Xk, k)

        def sum_leg():
            for _ in range(APPLIES):
                ctx.sum_vectors(out, b, ones, 1.0)

        r = summary(timed(ctx, [("bj_apply", apply_leg), ("bj_mapply_k4", mapply_leg), ("sum_vectors", sum_leg)], ROUNDS), per=APPLIES)
        model = dict(bj_apply=8.0 * values + 16.0 * n, bj_mapply_k4=8.0 * values + 16.0 * n * k, sum_vectors=24.0 * n)
        r["model_bytes"] = model
        r["gb_per_s"] = {q: model[q] / (r["median_ms"][q] * 1e-3) / 1e9 for q in model}
        r["apply_over_sum_vectors"] = r["gb_per_s"]["bj_apply"] / r["gb_per_s"]["sum_vectors"]
        r["mapply_over_sum_vectors"] = r["gb_per_s"]["bj_mapply_k4"] / r["gb_per_s"]["sum_vectors"]
        rec["apply"] = r
        g = r["gb_per_s"]
        print(f"{spec} (b) one apply: bj({bs}) {r['median_ms']['bj_apply'] * 1e3:.1f} us = {g['bj_apply']:.0f} GB/s on {model['bj_apply'] / 1e6:.1f} MB, "
              f"k = 4 {r['median_ms']['bj_mapply_k4'] * 1e3:.1f} us = {g['bj_mapply_k4']:.0f} GB/s, sum_vectors {r['median_ms']['sum_vectors'] * 1e3:.1f} us = "
              f"{g['sum_vectors']:.0f} GB/s; apply / sum_vectors {r['apply_over_sum_vectors']:.2f}, k = 4 {r['mapply_over_sum_vectors']:.2f}", flush=True)
        for v in (out, Xk, Yk):
            v.free()

    if "c" in parts:
        D, Dinv = ctx.mat_diag(A)
        if "ilu0" in others:
            iLs, iLD, iUs, iUD = others["ilu0"]
            iUinv = ctx.alloc(n)
            ctx.elemwise_div_vectors(iUinv, iLD, iUD)
        if "fsai" in others:
            G, Gt, _ = others["fsai"]
        handles, legs, got = [], [], {}

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

        for pc in ("bj", "j") + (("fsai",) if "fsai" in others else ()) + (("ilu0it",) if "ilu0" in others else ()):
            s = ctx.cg(A, b, x, A_D=D if pc == "j" else None)
            if pc == "bj":
                s.set_preconditioner(bj)
            elif pc == "fsai":
                s.set_preconditioner("fsai", Ls=G, Us=Gt)
            elif pc == "ilu0it":
                s.set_preconditioner("ilu0it", Ls=iLs, Us=iUs, A_D=iLD, A_D_inv=iUinv, L_D=iLD, U_D=iUD, inner=3)
            handles.append(s)
            legs.append((pc, solve_leg(s, pc)))
        r = summary(timed(ctx, legs, ROUNDS))
        r["result"] = got
        rec["solve_cg"] = r
        print(f"{spec} (c) -cg to {TOL:g} r0: " + ", ".join(
            f"{pc} {got[pc]['iters']} it {'conv' if got[pc]['converged'] else 'NOT conv'} {r['median_ms'][pc]:.1f} ms" for pc, _ in legs), flush=True)
        for s in handles:
            s.free()

    info = ctx.device_info()
    bj.free()
    ctx.close()
    return dict(device=info, records=[rec])


def main():
    argv = sys.argv[1:]

    def opt(name, default):
        return argv[argv.index(name) + 1] if name in argv else default

    json_out = opt("--json", None)
    bs, parts, max_iters = int(opt("--bs", 3)), opt("--parts", "abc"), int(opt("--max-iters", 2000))
    taken = {argv[i + 1] for i, a in enumerate(argv[:-1]) if a in ("--json", "--bs", "--parts", "--max-iters")}
    specs = [a for a in argv if not a.startswith("--") and a not in taken] or DEFAULT
    if "--child" in argv:  # one input, in this process
        out = run_input(specs[0], bs, parts, max_iters)
        if json_out:
            with open(json_out, "w") as f:
                json.dump(out, f, indent=1)
        return 0
    # one child per input, each GPU step under its own time limit; a failing step ends the script
    merged = dict(device=None, records=[])
    for i, spec in enumerate(specs):
        part = f"{json_out}.{i}.part" if json_out else None
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--child", spec, "--bs", str(bs),
               "--parts", parts, "--max-iters", str(max_iters)]
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
