#!/usr/bin/env python3
"""Time a lock-step GMRES(10) solve of k = 2, 4, 8 columns (MGMRES, init + 20 iterations) against k single-column GMRES(10)
solves made of the single-vector device-scalar calls (spmv, apply_preconditioner, bis_dot_dev, bis_axpy_dot_dev,
bis_scalar_sqrt_inv, bis_scale_dev, one download of the Hessenberg column per iteration, the Givens algebra on the host,
multi_axpy and sum_vectors at a restart: host/methods/gmres.hpp's orthogonalize_V_dev, the way k systems are solved without
bis_mgmres_*) -- per input in ONE process on ONE allocation of the matrix, the preconditioner's operands and the vectors, the
legs alternating round by round, five rounds.
   python tools/mgmres_ab.py [INPUT ...] [--iters 20] [--ks 2,4,8] [--restart 10] [--json FILE]
INPUT is generator[/order]@preconditioner: anderson:256,shift=9@gs (config 4), unstr:80,80,80@ilu0, unstr:80,80,80/rcm@ilu0,
fem:80,80,81@ilu0 are the defaults; each runs in a child process of its own under a time limit (a GPU step that fails or runs
out of time ends the script: nothing more is started on the device).  Reported per input and k: ms per solve (median and
minimum over the rounds), the ratio, and the kernels' names (bis_mat_sweep_kernel / bis_mat_sweepm_kernel, SpMV / SpMM)."""
import ctypes as C
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT = ["anderson:256,shift=9@gs", "unstr:80,80,80@ilu0", "unstr:80,80,80/rcm@ilu0", "fem:80,80,81@ilu0"]
STEP_LIMIT = 420  # seconds per input
ROUNDS = 5


def generate(ctx, spec):
    spec, _, order = spec.partition("/")
    kind, dims = spec.split(":")
    nums = [int(v) for v in dims.split(",") if "=" not in v]
    kw = {k: float(v) for k, v in (p.split("=") for p in dims.split(",") if "=" in p)}
    if kind == "anderson":
        A = ctx.gen_anderson(nums[0], shift=kw.get("shift", 0.0))
    elif kind == "hpcg":
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
    """One column's GMRES(m) from the single-vector calls with device scalars (GMRESSolver with orthogonalize_V_dev,
    host/methods/gmres.hpp): n + 2 stream-ordered reductions per iteration, one download of the Hessenberg column, the Givens
    algebra on the host."""

    def __init__(self, ctx, A, pc, ops, b, x, m):
        self.ctx, self.A, self.pc, self.ops, self.b, self.x, self.n, self.m = ctx, A, pc, ops, b, x, A.n_rows, m
        self.w = {q: ctx.alloc(self.n) for q in ("r", "w", "t", "vy", "tmp", "work")}
        self.V = ctx.alloc(self.n * (m + 1))
        self.hcol = ctx.alloc(m + 4)

    def apply(self, v):
        self.ctx.apply_preconditioner(self.pc, self.n, *self.ops, v, v, self.w["tmp"], self.w["work"])

    def start_cycle(self):
        ctx, w, n = self.ctx, self.w, self.n
        ctx.spmv(self.A, self.x, w["t"])
        ctx.subtract_vectors(w["r"], self.b, w["t"], 1.0)
        unpre = ctx.euclidean_vec_norm(w["r"])
        self.apply(w["r"])
        beta = ctx.euclidean_vec_norm(w["r"])
        ctx.scale(self.V.offset(0, n), w["r"], 1.0 / beta)
        return unpre, beta

    def solve(self, iters):
        import numpy as np
        ctx, lib, h, n, m, w, V, hc = self.ctx, self.ctx.lib, self.ctx.h, self.n, self.m, self.w, self.V, self.hcol
        p = lambda v, off=0: C.c_void_p(v.ptr + 8 * off)
        n64 = C.c_int64(n)
        ctx.init_vector(self.x, 0.0)
        r0, beta = self.start_cycle()
        hist = [r0]
        R, cs, sn, g = np.zeros((m + 1, m)), np.zeros(m), np.zeros(m), np.zeros(m + 1)
        g[0] = beta
        pos = 0
        for _ in range(iters):
            ctx.spmv(self.A, V.offset(pos * n, n), w["w"])
            self.apply(w["w"])
            ctx.check(lib.bis_dot_dev(h, p(w["w"]), p(V), n64, p(hc)))
            for i in range(pos):
                ctx.check(lib.bis_axpy_dot_dev(h, p(w["w"]), p(V, i * n), p(hc, i), p(V, (i + 1) * n), n64, p(hc, i + 1)))
            ctx.check(lib.bis_axpy_dot_dev(h, p(w["w"]), p(V, pos * n), p(hc, pos), C.c_void_p(), n64, p(hc, pos + 1)))
            ctx.check(lib.bis_scalar_sqrt_inv(h, p(hc, pos + 1), p(hc, pos + 2), p(hc, pos + 1)))
            ctx.check(lib.bis_scale_dev(h, p(V, (pos + 1) * n), p(w["w"]), p(hc, pos + 2), n64))
            col = hc.to_host()[:pos + 2]  # the per-iteration round trip
            for i in range(pos):
                a, b = col[i], col[i + 1]
                col[i], col[i + 1] = cs[i] * a + sn[i] * b, cs[i] * b - sn[i] * a
            a, b = col[pos], col[pos + 1]
            den = np.sqrt(a * a + b * b)
            cs[pos], sn[pos] = a / den, b / den
            R[:pos, pos] = col[:pos]
            R[pos, pos] = cs[pos] * a + sn[pos] * b
            g[pos + 1] = -sn[pos] * g[pos]
            g[pos] = cs[pos] * g[pos]
            hist.append(abs(g[pos + 1]))
            pos += 1
            if pos == m:  # check_restart (tol 0: nothing stops)
                y = np.zeros(m)
                for r in range(m - 1, -1, -1):
                    y[r] = (g[r] - np.dot(R[r, r + 1:m], y[r + 1:m])) / R[r, r]
                ctx.multi_axpy(V, n, y, m, w["vy"], n)
                ctx.sum_vectors(self.x, self.x, w["vy"], 1.0)
                _, beta = self.start_cycle()
                hist.append(beta)
                g[:] = 0.0
                g[0] = beta
                pos = 0
        return hist


def run_input(spec, iters, ks, m):
    import numpy as np
    from basic_iterative_solvers_amd import Context
    ctx = Context(0)
    records = []
    gen, _, pc = spec.partition("@")
    pc = pc or "ilu0"
    A = generate(ctx, gen)
    n = A.n_rows
    if pc == "ilu0":
        Ls, LD, Us, UD = ctx.ilu0(A)
        ops = (Ls, Us, LD, LD, LD, UD)
    else:
        Ls, Us, D, Dinv = ctx.split_strict(A)
        ops = (Ls, Us, D, Dinv, D, D)
    kw = dict(Ls=ops[0], Us=ops[1], A_D=ops[2], A_D_inv=ops[3], L_D=ops[4], U_D=ops[5])
    rng = np.random.default_rng(1)
    kmax = max(ks)
    bs = [ctx.upload(rng.uniform(-1, 1, n)) for _ in range(kmax)]
    singles = [Single(ctx, A, pc, ops, bs[j], ctx.alloc(n), m) for j in range(kmax)]
    Bk, Xk = ctx.alloc(n * kmax), ctx.alloc(n * kmax)
    for k in ks:
        for j in range(k):
            ctx.mvec_set_col(Bk, n, k, j, bs[j])
        s = ctx.mgmres(A, Bk, Xk, k, restart=m)
        s.set_preconditioner(pc, **kw)
        got = {}

        def lockstep():
            ctx.init_vector(Xk, 0.0, n * k)
            s.init(0.0)  # tol 0: nothing stops
            s.iterate(iters)

        def k_singles():
            got["hist"] = [singles[j].solve(iters) for j in range(k)]

        times = timed(ctx, [("mgmres", lockstep), ("k x single", k_singles)])
        med = {q: float(np.median(v)) for q, v in times.items()}
        st = [s.status(j) for j in range(k)]
        dev = [float(np.max(np.abs(st[j][2] - np.array(got["hist"][j])[:len(st[j][2])])) / st[j][2][0]) for j in range(k)]
        rec = dict(input=gen, preconditioner=pc, rows=n, nnz=A.nnz, k=k, restart=m, iters=iters, iters_done=[q[0] for q in st],
                   hist_entries=[len(q[2]) for q in st], hist_dev_vs_single=dev, spmm_kernel=A.spmm_kernel(),
                   spmv_kernel=A.spmv_kernel(), sweepm_kernels=[ops[0].sweepm_kernel(False), ops[1].sweepm_kernel(True)],
                   sweep_kernels=[ops[0].sweep_kernel(False), ops[1].sweep_kernel(True)],
                   median_ms=med, min_ms={q: float(np.min(v)) for q, v in times.items()},
                   ratio_k_singles_over_lockstep=med["k x single"] / med["mgmres"], rounds=times,
                   note="init + `iters` iterations per call; the k-singles leg downloads one Hessenberg column per iteration and column")
        records.append(rec)
        print(f"{spec} k={k}: mgmres {med['mgmres']:.3f} ms [{rec['spmm_kernel']}; {', '.join(rec['sweepm_kernels'])}], "
              f"k x single {med['k x single']:.3f} ms [{rec['spmv_kernel']}; {', '.join(rec['sweep_kernels'])}] for init + {iters} "
              f"iterations of GMRES({m}) (done {rec['iters_done']}); ratio {rec['ratio_k_singles_over_lockstep']:.2f}; "
              f"history deviation {max(dev):.2e}", flush=True)
        s.free()
    info = ctx.device_info()
    ctx.close()
    return dict(device=info, records=records)


def main():
    argv = sys.argv[1:]

    def opt(name, default):
        return argv[argv.index(name) + 1] if name in argv else default

    json_out = opt("--json", None)
    iters = int(opt("--iters", 20))
    m = int(opt("--restart", 10))
    ks_arg = opt("--ks", "2,4,8")
    ks = tuple(int(v) for v in ks_arg.split(","))
    taken = {json_out, str(iters) if "--iters" in argv else None, ks_arg if "--ks" in argv else None,
             str(m) if "--restart" in argv else None}
    child = "--child" in argv
    specs = [a for a in argv if not a.startswith("--") and a not in taken] or DEFAULT
    if child:  # one input, in this process
        out = run_input(specs[0], iters, ks, m)
        if json_out:
            with open(json_out, "w") as f:
                json.dump(out, f, indent=1)
        return 0
    # one child per input, each GPU step under its own time limit; a failing step ends the script
    merged = dict(device=None, records=[])
    for i, spec in enumerate(specs):
        part = f"{json_out}.{i}.part" if json_out else None
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--child", spec,
               "--iters", str(iters), "--ks", ks_arg, "--restart", str(m)]
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
