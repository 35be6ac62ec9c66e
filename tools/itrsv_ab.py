#!/usr/bin/env python3
"""Time the step of bis_itrsv against the three-launch composition it replaces (bis_spmv + bis_subtract_vectors +
bis_elemwise_mult_vectors), on the ILU(0) L factor of an input, in one process, on one set of vectors, the variants
interleaved round by round; the results are compared bit for bit.
   python tools/itrsv_ab.py fem:80,80,81 unstr:80,80,80 unstr:80,80,80/rcm [--json FILE]
Per input two configurations of the SAME factor (bis_mat_retune between them): the default SpMV form, and the CRS-value
row-block kernel forced (spmv_win8 = 0, spmv_colslab = 0, spmv_valdict = 0) -- the one form whose step is fused.  Variants:
   itrsv      bis_itrsv, STEPS steps (plus x_0 = D_inv b)
   3-launch   x_0, then STEPS x (bis_spmv, bis_subtract_vectors, bis_elemwise_mult_vectors)
   spmv+sub   x_0, then STEPS x (bis_spmv, bis_subtract_vectors in place): a LOWER bound on SpMV + epilogue kernel (it moves
              24 B per row where the epilogue moves 40) -- what the fused step has to beat on a form-0 triangle
   x0         x_0 alone (subtracted from the others for the per-step figures)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from basic_iterative_solvers_amd import Context

STEPS, REPS, ROUNDS = 8, 3, 7
args = [a for a in sys.argv[1:] if not a.startswith("--")]
json_out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
if json_out:
    args.remove(json_out)
ctx = Context(0)
records = []


def generate(spec):
    spec, _, order = spec.partition("/")
    kind, dims = spec.split(":")
    A = (ctx.gen_unstr if kind == "unstr" else ctx.gen_fem)(*[int(v) for v in dims.split(",")])
    if order:
        B = ctx.permute(A, ctx.bfs_order(A, rcm=order == "rcm"))
        A.free()
        A = B
    return A


for spec in args:
    A = generate(spec)
    n = A.n_rows
    t0 = time.perf_counter()
    L, L_D, U, U_D = ctx.ilu0(A)
    ctx.sync()
    t_ilu = time.perf_counter() - t0
    A.free(); U.free()
    b, x, work, tmp, y = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
    b.set(np.random.default_rng(1).uniform(-1, 1, n))
    dinv = L_D  # the vector of ones: its own reciprocal

    def itrsv():
        ctx.itrsv(L, dinv, b, x, work, STEPS)

    def x0():
        ctx.elemwise_mult_vectors(y, dinv, b)

    def three():
        cur, nxt = y, work
        ctx.elemwise_mult_vectors(cur, dinv, b)
        for _ in range(STEPS):
            ctx.spmv(L, cur, tmp)
            ctx.subtract_vectors(tmp, b, tmp)
            ctx.elemwise_mult_vectors(nxt, tmp, dinv)
            cur, nxt = nxt, cur
        return cur

    def spmv_sub():
        cur, nxt = y, work
        ctx.elemwise_mult_vectors(cur, dinv, b)
        for _ in range(STEPS):
            ctx.spmv(L, cur, nxt)
            ctx.subtract_vectors(nxt, b, nxt)
            cur, nxt = nxt, cur

    variants = [("itrsv", itrsv), ("3-launch", three), ("spmv+sub", spmv_sub), ("x0", x0)]
    for cfg in (dict(), dict(spmv_win8=0, spmv_colslab=0, spmv_valdict=0)):
        for k, v in cfg.items():
            ctx.set_option(k, v)
        L.retune()
        itrsv(); got = x.to_host()
        ref = three().to_host()
        same = bool(np.array_equal(got, ref))
        for _, f in variants:  # warm
            f()
        ctx.sync()
        times = {name: [] for name, _ in variants}
        for _ in range(ROUNDS):
            for name, f in variants:
                ctx.sync()
                t0 = time.perf_counter()
                for _ in range(REPS):
                    f()
                ctx.sync()
                times[name].append((time.perf_counter() - t0) / REPS * 1e3)
        med = {k: float(np.median(v)) for k, v in times.items()}
        lo = {k: float(np.min(v)) for k, v in times.items()}
        step = {k: (med[k] - med["x0"]) / STEPS for k in ("itrsv", "3-launch", "spmv+sub")}
        rec = dict(input=spec, rows=n, nnz_L=L.nnz, options=cfg, spmv_kernel=L.spmv_kernel(), spmv_form=L.spmv_stream_info()[3],
                   itrsv_kernel=L.itrsv_kernel(), bit_identical=same, steps=STEPS, median_ms=med, min_ms=lo, per_step_ms=step,
                   rounds=times, ilu0_s=t_ilu)
        records.append(rec)
        print(f"{spec} {cfg or 'default'}: L {n} rows {L.nnz} nnz, SpMV {rec['spmv_kernel']} (form {rec['spmv_form']}), "
              f"{rec['itrsv_kernel']}; per step: itrsv {step['itrsv']:.3f} ms, 3-launch {step['3-launch']:.3f} ms, "
              f"spmv+sub {step['spmv+sub']:.3f} ms (x0 {med['x0']:.3f} ms); bit-identical {same}", flush=True)
        for k in cfg:
            ctx.set_option(k, -1)
    for v in (b, x, work, tmp, y, L_D, U_D):
        v.free()
    L.free()
if json_out:
    with open(json_out, "w") as f:
        json.dump(dict(device=ctx.device_info(), records=records), f, indent=1)
ctx.close()
