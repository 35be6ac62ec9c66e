#!/usr/bin/env python3
"""Time one bis_sptrsm / bis_bsptrsm at k = 2, 4, 8 against k bis_sptrsv / bis_bsptrsv calls, and a preconditioned MCG solve of
k = 4 columns (ILU(0), SGS) against four bis_cg solves with the same preconditioner -- per input in ONE process on ONE
allocation of the matrix and the vectors, the legs alternating round by round.
   python tools/sptrsm_ab.py [hpcg:64 fem:40,40,40 unstr:40,40,40 unstr:40,40,40/rcm] [--json FILE]
Without arguments the four default inputs run, each in a child process of its own under a time limit (a GPU step that fails
or runs out of time ends the script: nothing more is started on the device).  Reported per input, side and k: ms per call
(median and minimum over the rounds), the kernels' names, and the byte model 12 nnz + rp + 8 (1 + 3 k) n."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT = ["hpcg:64", "fem:40,40,40", "unstr:40,40,40", "unstr:40,40,40/rcm"]
STEP_LIMIT = 300  # seconds per input
REPS, ROUNDS, CG_ITERS = 5, 5, 10
KS = (2, 4, 8)


def generate(ctx, spec):
    spec, _, order = spec.partition("/")
    kind, dims = spec.split(":")
    nums = [int(v) for v in dims.split(",")]
    if kind == "hpcg":
        A = ctx.gen_hpcg(*nums)
    else:
        A = (ctx.gen_unstr if kind == "unstr" else ctx.gen_fem)(*nums)
    if order:
        B = ctx.permute(A, ctx.bfs_order(A, rcm=order == "rcm"))
        A.free()
        A = B
    return A


def timed(ctx, legs, reps):
    """{name: [ms per call, one entry per round]}, the legs alternating inside every round."""
    for _, f in legs:
        f()
    ctx.sync()
    times = {name: [] for name, _ in legs}
    for _ in range(ROUNDS):
        for name, f in legs:
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            ctx.sync()
            times[name].append((time.perf_counter() - t0) / reps * 1e3)
    return times


def run_input(spec):
    import numpy as np
    from basic_iterative_solvers_amd import Context
    ctx = Context(0)
    records = []
    A = generate(ctx, spec)
    n = A.n_rows
    Ls, Us, D, Dinv = ctx.split_strict(A)
    rng = np.random.default_rng(1)
    kmax = max(KS)
    bs, xs = [ctx.upload(rng.uniform(-1, 1, n)) for _ in range(kmax)], [ctx.alloc(n) for _ in range(kmax)]
    B, X, tmp = ctx.alloc(n * kmax), ctx.alloc(n * kmax), ctx.alloc(n)
    for backward, T in ((False, Ls), (True, Us)):
        multi = ctx.bsptrsm if backward else ctx.sptrsm
        one = ctx.bsptrsv if backward else ctx.sptrsv
        for k in KS:
            for j in range(k):
                ctx.mvec_set_col(B, n, k, j, bs[j])

            def sweepm():
                multi(T, X, D, B, k)

            def sweeps():
                for j in range(k):
                    one(T, xs[j], D, bs[j])

            sweepm(); sweeps()
            same = True
            for j in range(k):
                ctx.mvec_get_col(tmp, X, n, k, j)
                same = same and bool(np.array_equal(tmp.to_host().view(np.uint64), xs[j].to_host().view(np.uint64)))
            times = timed(ctx, [("sptrsm", sweepm), ("k x sptrsv", sweeps)], REPS)
            med = {q: float(np.median(v)) for q, v in times.items()}
            nbytes = 12 * T.nnz + T.rp_width * (n + 1) + 8 * (1 + 3 * k) * n
            rec = dict(input=spec, side="backward" if backward else "forward", rows=n, nnz=T.nnz, k=k,
                       sptrsm_kernel=T.sweepm_kernel(backward), sptrsv_kernel=T.sweep_kernel(backward), bit_identical=same,
                       median_ms=med, min_ms={q: float(np.min(v)) for q, v in times.items()}, model_bytes=nbytes,
                       speedup_vs_k_sptrsv=med["k x sptrsv"] / med["sptrsm"], rounds=times)
            records.append(rec)
            print(f"{spec} {rec['side']} k={k}: {rec['sptrsm_kernel']} {med['sptrsm']:.3f} ms ({med['sptrsm'] / k:.3f} per rhs, model "
                  f"{nbytes} B); k x [{rec['sptrsv_kernel']}] {med['k x sptrsv']:.3f} ms; speed-up {rec['speedup_vs_k_sptrsv']:.2f}; "
                  f"bit-identical {same}", flush=True)
    # MCG at k = 4 against four CG solves, ILU(0) and SGS (tol 0: nothing stops, x0 = 0)
    k = 4
    iLs, iLD, iUs, iUD = ctx.ilu0(A)
    Bk, X0 = ctx.alloc(n * k), ctx.alloc(n * k)
    for j in range(k):
        ctx.mvec_set_col(Bk, n, k, j, bs[j])
    x0s = [ctx.alloc(n) for _ in range(k)]
    for pc, kw in (("ilu0", dict(Ls=iLs, Us=iUs, A_D=iLD, A_D_inv=iLD, L_D=iLD, U_D=iUD)),
                   ("sgs", dict(Ls=Ls, Us=Us, A_D=D, A_D_inv=Dinv, L_D=D, U_D=D))):
        m = ctx.mcg(A, Bk, X0, k)
        m.set_preconditioner(pc, **kw)
        cgs = [ctx.cg(A, bs[j], x0s[j]) for j in range(k)]
        for c in cgs:
            c.set_preconditioner(pc, **kw)

        def mcg():
            ctx.init_vector(X0, 0.0)
            m.init(0.0)
            m.iterate(CG_ITERS)

        def four_cg():
            for j in range(k):
                ctx.init_vector(x0s[j], 0.0)
                cgs[j].init(0.0)
                cgs[j].iterate(CG_ITERS)

        times = timed(ctx, [("mcg k=4", mcg), ("4 x cg", four_cg)], 1)
        med = {q: float(np.median(v)) for q, v in times.items()}
        rec = dict(input=spec, preconditioner=pc, rows=n, nnz=A.nnz, k=k, cg_iters=CG_ITERS,
                   mcg_iters_done=[m.status(j)[0] for j in range(k)], cg_iters_done=[c.status()[0] for c in cgs],
                   sweepm_kernels=[(iLs if pc == "ilu0" else Ls).sweepm_kernel(False), (iUs if pc == "ilu0" else Us).sweepm_kernel(True)],
                   median_ms=med, min_ms={q: float(np.min(v)) for q, v in times.items()},
                   speedup_vs_4_cg=med["4 x cg"] / med["mcg k=4"], rounds=times, note="init + CG_ITERS iterations per call")
        records.append(rec)
        print(f"{spec} mcg+{pc} k=4: {med['mcg k=4']:.3f} ms [{', '.join(rec['sweepm_kernels'])}], 4 x cg {med['4 x cg']:.3f} ms for init + "
              f"{CG_ITERS} iterations (done {rec['mcg_iters_done']} / {rec['cg_iters_done']}); speed-up {rec['speedup_vs_4_cg']:.2f}", flush=True)
        m.free()
        for c in cgs:
            c.free()
    info = ctx.device_info()
    ctx.close()
    return dict(device=info, records=records)


def main():
    argv = sys.argv[1:]
    json_out = argv[argv.index("--json") + 1] if "--json" in argv else None
    child = "--child" in argv
    specs = [a for a in argv if not a.startswith("--") and a != json_out] or DEFAULT
    if child:  # one input, in this process
        out = run_input(specs[0])
        if json_out:
            with open(json_out, "w") as f:
                json.dump(out, f, indent=1)
        return 0
    # one child per input, each GPU step under its own time limit; a failing step ends the script
    merged = dict(device=None, records=[])
    for i, spec in enumerate(specs):
        part = f"{json_out}.{i}.part" if json_out else None
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--child", spec]
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
