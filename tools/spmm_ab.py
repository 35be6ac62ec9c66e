#!/usr/bin/env python3
"""Time bis_spmm at k = 2, 4, 8 against k launches of bis_spmv, and MCG at k = 4 against four sequential CG solves, in one
process, on one allocation of the matrix and the vectors, the legs alternating round by round.
   python tools/spmm_ab.py fem:80,80,81 unstr:80,80,80 unstr:80,80,80/rcm anderson:256,shift=9 hpcg:256 [--json FILE]
Legs per input and k:
   spmm k       one bis_spmm on the interleaved n x k block
   k x spmv     k bis_spmv launches in the matrix' default SpMV form, on k plain vectors
   k x spmv crs (matrices with a value dictionary only) the same with spmv_valdict = 0
and, once per input, CG_ITERS iterations (tol 0: nothing stops) of
   mcg k=4      bis_mcg_iterate on four columns
   4 x cg       bis_cg_iterate on the same four systems, one after the other
Reported: ms per call (median and minimum over the rounds), ms per right-hand side, and spmm_streamed_bytes / time as a
fraction of 8 TB/s."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from basic_iterative_solvers_amd import Context

REPS, ROUNDS, CG_ITERS, PEAK = 5, 5, 10, 8e12
KS = (2, 4, 8)
args = [a for a in sys.argv[1:] if not a.startswith("--")]
json_out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
if json_out:
    args.remove(json_out)
ctx = Context(0)
records = []


def generate(spec):
    spec, _, order = spec.partition("/")
    kind, dims = spec.split(":")
    parts = dims.split(",")
    nums = [int(v) for v in parts if "=" not in v]
    kw = {k: float(v) for k, v in (p.split("=") for p in parts if "=" in p)}
    if kind == "hpcg":
        A = ctx.gen_hpcg(*nums)
    elif kind == "anderson":
        A = ctx.gen_anderson(nums[0], shift=kw.get("shift", 0.0))
    else:
        A = (ctx.gen_unstr if kind == "unstr" else ctx.gen_fem)(*nums)
    if order:
        B = ctx.permute(A, ctx.bfs_order(A, rcm=order == "rcm"))
        A.free()
        A = B
    return A


def timed(legs):
    """{name: [ms per call, one entry per round]}, the legs alternating inside every round."""
    for _, f in legs:
        f()
    ctx.sync()
    times = {name: [] for name, _ in legs}
    for _ in range(ROUNDS):
        for name, f in legs:
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(REPS):
                f()
            ctx.sync()
            times[name].append((time.perf_counter() - t0) / REPS * 1e3)
    return times


for spec in args:
    A = generate(spec)
    n = A.n_rows
    rng = np.random.default_rng(1)
    kmax = max(KS)
    X, Y = ctx.alloc(n * kmax), ctx.alloc(n * kmax)
    xs, ys = [ctx.alloc(n) for _ in range(kmax)], [ctx.alloc(n) for _ in range(kmax)]
    for j in range(kmax):
        xs[j].set(rng.uniform(-1, 1, n))
    form = A.spmv_stream_info()[3]
    dictionary = 1 <= form <= 5
    for k in KS:
        for j in range(k):
            ctx.mvec_set_col(X, n, k, j, xs[j])

        def spmm():
            ctx.spmm(A, X, Y, k)

        def spmvs():
            for j in range(k):
                ctx.spmv(A, xs[j], ys[j])

        def spmvs_crs():
            ctx.set_option("spmv_valdict", 0)
            for j in range(k):
                ctx.spmv(A, xs[j], ys[j])
            ctx.set_option("spmv_valdict", -1)

        spmm(); spmvs()
        tmp = ctx.alloc(n)
        same = True
        for j in range(k):
            ctx.mvec_get_col(tmp, Y, n, k, j)
            same = same and bool(np.array_equal(tmp.to_host(), ys[j].to_host()))
        tmp.free()
        legs = [("spmm", spmm), ("k x spmv", spmvs)] + ([("k x spmv crs", spmvs_crs)] if dictionary else [])
        times = timed(legs)
        med = {q: float(np.median(v)) for q, v in times.items()}
        nbytes = A.spmm_streamed_bytes(k)
        rec = dict(input=spec, rows=n, nnz=A.nnz, k=k, spmv_kernel=A.spmv_kernel(), spmv_form=form, spmm_kernel=A.spmm_kernel(),
                   bit_identical=same, median_ms=med, min_ms={q: float(np.min(v)) for q, v in times.items()},
                   ms_per_rhs={q: v / k for q, v in med.items()}, spmm_streamed_bytes=nbytes,
                   spmm_fraction_of_8TBs=nbytes / (med["spmm"] * 1e-3) / PEAK, speedup_vs_k_spmv=med["k x spmv"] / med["spmm"], rounds=times)
        records.append(rec)
        print(f"{spec} k={k}: {rec['spmm_kernel']} {med['spmm']:.3f} ms ({med['spmm'] / k:.3f} per rhs, {rec['spmm_fraction_of_8TBs']:.2f} of 8 TB/s on "
              f"{nbytes} B); k x spmv [{rec['spmv_kernel']}, form {form}] {med['k x spmv']:.3f} ms ({med['k x spmv'] / k:.3f} per rhs)"
              + (f"; k x spmv crs {med['k x spmv crs']:.3f} ms" if dictionary else "") + f"; speed-up {rec['speedup_vs_k_spmv']:.2f}; bit-identical {same}", flush=True)
    # MCG at k = 4 against four CG solves (no preconditioner, tol 0, x0 = 0)
    k = 4
    B, X0 = ctx.alloc(n * k), ctx.alloc(n * k)
    for j in range(k):
        ctx.mvec_set_col(B, n, k, j, xs[j])
    m = ctx.mcg(A, B, X0, k)
    x0s = [ctx.alloc(n) for _ in range(k)]
    cgs = [ctx.cg(A, xs[j], x0s[j]) for j in range(k)]

    def mcg():
        ctx.init_vector(X0, 0.0)
        m.init(0.0)
        m.iterate(CG_ITERS)

    def four_cg():
        for j in range(k):
            ctx.init_vector(x0s[j], 0.0)
            cgs[j].init(0.0)
            cgs[j].iterate(CG_ITERS)

    saved = REPS
    REPS = 1
    times = timed([("mcg k=4", mcg), ("4 x cg", four_cg)])
    REPS = saved
    med = {q: float(np.median(v)) for q, v in times.items()}
    rec = dict(input=spec, rows=n, nnz=A.nnz, k=k, cg_iters=CG_ITERS, mcg_iters_done=[m.status(j)[0] for j in range(k)],
               cg_iters_done=[c.status()[0] for c in cgs], median_ms=med, min_ms={q: float(np.min(v)) for q, v in times.items()},
               speedup_vs_4_cg=med["4 x cg"] / med["mcg k=4"], rounds=times, note="init + CG_ITERS iterations per call")
    records.append(rec)
    print(f"{spec} mcg k=4: {med['mcg k=4']:.3f} ms, 4 x cg {med['4 x cg']:.3f} ms for init + {CG_ITERS} iterations "
          f"(done {rec['mcg_iters_done']} / {rec['cg_iters_done']}); speed-up {rec['speedup_vs_4_cg']:.2f}", flush=True)
    m.free()
    for c in cgs:
        c.free()
    for v in [X, Y, B, X0] + xs + ys + x0s:
        v.free()
    A.free()
if json_out:
    with open(json_out, "w") as f:
        json.dump(dict(device=ctx.device_info(), records=records), f, indent=1)
ctx.close()
