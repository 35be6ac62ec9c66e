#!/usr/bin/env python3
"""Time a lock-step BiCGSTAB solve of k = 2, 4, 8 columns (MBiCGSTAB, ILU(0), init + 10 iterations) against k single-column
BiCGSTAB solves made of the single-vector calls (apply_preconditioner, spmv, dot, subtract_vectors, sum_vectors,
euclidean_vec_norm with host scalars: the way k systems are solved without bis_mbicgstab_*) -- per input in ONE process on
ONE allocation of the matrix, the factors and the vectors, the legs alternating round by round, five rounds.
   python tools/mbicgstab_ab.py [unstr:80,80,80 unstr:80,80,80/rcm fem:80,80,81] [--iters 10] [--ks 2,4,8] [--json FILE]
Without arguments the three default inputs run, each in a child process of its own under a time limit (a GPU step that fails
or runs out of time ends the script: nothing more is started on the device).  Reported per input and k: ms per solve (median
and minimum over the rounds), the ratio, and the kernels' names (bis_mat_sweep_kernel / bis_mat_sweepm_kernel, SpMV / SpMM)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT = ["unstr:80,80,80", "unstr:80,80,80/rcm", "fem:80,80,81"]
STEP_LIMIT = 300  # seconds per input
ROUNDS = 5


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


def timed(ctx, legs):
    """{name: [ms per call, one entry per round]}, the legs alternating inside every round (one warm-up call each first)."""
    for _, f in legs:
        f()
    ctx.sync()
    times = {name: [] for name, _ in legs}
    for _ in range(ROUNDS):
        for name, f in legs:
            ctx.sync()
            t0 = time.perf_counter()
            f()
            ctx.sync()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return times


class Single:
    """One column's BiCGSTAB from the single-vector calls, host scalars (bicgstab_separate_iteration, bicgstab.hpp:8-83)."""

    def __init__(self, ctx, A, ops, b, x):
        self.ctx, self.A, self.ops, self.b, self.x, self.n = ctx, A, ops, b, x, A.n_rows
        self.w = {q: ctx.alloc(self.n) for q in ("xn", "h", "r", "rn", "r0", "p", "pn", "v", "s", "st", "y", "z", "t", "tmp", "work")}

    def apply(self, out, inp):
        self.ctx.apply_preconditioner("ilu0", self.n, *self.ops, out, inp, self.w["tmp"], self.w["work"])

    def solve(self, iters):
        import numpy as np
        ctx, A, w, f = self.ctx, self.A, dict(self.w), np.float64
        x = self.x
        ctx.init_vector(x, 0.0)
        ctx.spmv(A, x, w["t"])
        ctx.subtract_vectors(w["r"], self.b, w["t"], 1.0)
        hist = [ctx.euclidean_vec_norm(w["r"])]
        self.apply(w["p"], w["r"])
        ctx.copy_vector(w["r0"], w["p"])
        rho = f(ctx.dot(w["r"], w["p"]))
        with np.errstate(all="ignore"):
            for _ in range(iters):
                self.apply(w["y"], w["p"])
                ctx.spmv(A, w["y"], w["v"])
                alpha = rho / f(ctx.dot(w["r0"], w["v"]))
                ctx.subtract_vectors(w["s"], w["r"], w["v"], float(alpha))
                self.apply(w["st"], w["s"])
                ctx.spmv(A, w["st"], w["z"])
                omega = f(ctx.dot(w["z"], w["s"])) / f(ctx.dot(w["z"], w["z"]))
                ctx.sum_vectors(w["h"], x, w["y"], float(alpha))
                ctx.sum_vectors(w["xn"], w["h"], w["st"], float(omega))
                ctx.subtract_vectors(w["rn"], w["s"], w["z"], float(omega))
                rho_new = f(ctx.dot(w["r0"], w["rn"]))
                beta = (rho_new / rho) * (alpha / omega)
                ctx.subtract_vectors(w["t"], w["p"], w["v"], float(omega))
                ctx.sum_vectors(w["pn"], w["rn"], w["t"], float(beta))
                hist.append(ctx.euclidean_vec_norm(w["rn"]))
                w["p"], w["pn"] = w["pn"], w["p"]
                w["r"], w["rn"] = w["rn"], w["r"]
                x, w["xn"] = w["xn"], x
                rho = rho_new
        return hist


def run_input(spec, iters, ks):
    import numpy as np
    from basic_iterative_solvers_amd import Context
    ctx = Context(0)
    records = []
    A = generate(ctx, spec)
    n = A.n_rows
    iLs, iLD, iUs, iUD = ctx.ilu0(A)
    ops = (iLs, iUs, iLD, iLD, iLD, iUD)
    kw = dict(Ls=iLs, Us=iUs, A_D=iLD, A_D_inv=iLD, L_D=iLD, U_D=iUD)
    rng = np.random.default_rng(1)
    kmax = max(ks)
    bs = [ctx.upload(rng.uniform(-1, 1, n)) for _ in range(kmax)]
    singles = [Single(ctx, A, ops, bs[j], ctx.alloc(n)) for j in range(kmax)]
    Bk, Xk = ctx.alloc(n * kmax), ctx.alloc(n * kmax)
    for k in ks:
        for j in range(k):
            ctx.mvec_set_col(Bk, n, k, j, bs[j])
        m = ctx.mbicgstab(A, Bk, Xk, k)
        m.set_preconditioner("ilu0", **kw)
        got = {}

        def lockstep():
            ctx.init_vector(Xk, 0.0, n * k)
            m.init(0.0)  # tol 0: nothing stops
            m.iterate(iters)

        def k_singles():
            got["hist"] = [singles[j].solve(iters) for j in range(k)]

        times = timed(ctx, [("mbicgstab", lockstep), ("k x single", k_singles)])
        med = {q: float(np.median(v)) for q, v in times.items()}
        st = [m.status(j) for j in range(k)]
        dev = [float(np.max(np.abs(st[j][2] - np.array(got["hist"][j])[:len(st[j][2])])) / st[j][2][0]) for j in range(k)]
        rec = dict(input=spec, preconditioner="ilu0", rows=n, nnz=A.nnz, k=k, iters=iters, iters_done=[s[0] for s in st],
                   hist_dev_vs_single=dev, spmm_kernel=A.spmm_kernel(), spmv_kernel=A.spmv_kernel(),
                   sweepm_kernels=[iLs.sweepm_kernel(False), iUs.sweepm_kernel(True)],
                   sweep_kernels=[iLs.sweep_kernel(False), iUs.sweep_kernel(True)],
                   median_ms=med, min_ms={q: float(np.min(v)) for q, v in times.items()},
                   ratio_k_singles_over_lockstep=med["k x single"] / med["mbicgstab"], rounds=times,
                   note="init + `iters` iterations per call; the k-singles leg reads 5 scalars per iteration and column on the host")
        records.append(rec)
        print(f"{spec} k={k}: mbicgstab {med['mbicgstab']:.3f} ms [{rec['spmm_kernel']}; {', '.join(rec['sweepm_kernels'])}], "
              f"k x single {med['k x single']:.3f} ms [{rec['spmv_kernel']}; {', '.join(rec['sweep_kernels'])}] for init + {iters} "
              f"iterations (done {rec['iters_done']}); ratio {rec['ratio_k_singles_over_lockstep']:.2f}; "
              f"history deviation {max(dev):.2e}", flush=True)
        m.free()
    info = ctx.device_info()
    ctx.close()
    return dict(device=info, records=records)


def main():
    argv = sys.argv[1:]

    def opt(name, default):
        return argv[argv.index(name) + 1] if name in argv else default

    json_out = opt("--json", None)
    iters = int(opt("--iters", 10))
    ks_arg = opt("--ks", "2,4,8")
    ks = tuple(int(v) for v in ks_arg.split(","))
    taken = {json_out, str(iters) if "--iters" in argv else None, ks_arg if "--ks" in argv else None}
    child = "--child" in argv
    specs = [a for a in argv if not a.startswith("--") and a not in taken] or DEFAULT
    if child:  # one input, in this process
        out = run_input(specs[0], iters, ks)
        if json_out:
            with open(json_out, "w") as f:
                json.dump(out, f, indent=1)
        return 0
    # one child per input, each GPU step under its own time limit; a failing step ends the script
    merged = dict(device=None, records=[])
    for i, spec in enumerate(specs):
        part = f"{json_out}.{i}.part" if json_out else None
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--child", spec,
               "--iters", str(iters), "--ks", ks_arg]
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
