#!/usr/bin/env python3
"""Time one iteration of the LSMR handle (bis_lsmr_*, the CLI's -lsmr) against the same iteration made of the library's
single-vector calls (spmv, subtract_vectors / sum_vectors, dot, scale, elemwise_mult_vectors; the scalar algebra on the
host, tests/lsmr_ref.py's Scalars) -- per input in ONE process on ONE allocation of A, At and the vectors, the legs
alternating round by round, five rounds.
   python tools/lsmr_ab.py [INPUT ...] [--iters 50] [--json FILE]
INPUT is a generator string, optionally followed by @tall: the first 60 % of the columns of the generated matrix (cut on the
host from the downloaded matrix, uploaded again), an over-determined system.  Defaults: unstr:80,80,80 (square),
unstr:80,80,80@tall, hpcg:128.
Per input: ms per iteration of both legs without and with the column scaling d = 1 / column norms (median and minimum
over the rounds, tol 0: nothing stops, the blocking init stays outside), the ratio, the bytes the passes move beside the two
products (24 m + 88 n per iteration, 24 m + 112 n scaled; the call-by-call loop: 40 m + 144 n, 40 m + 216 n), and one solve
to tol 1e-8 from x0 = 0 (b uniform(-1, 1) from default_rng(1)) with its iteration count, stop reason and time.
Each input runs in a child process of its own under a time limit (a GPU step that fails or runs out of time ends the script:
nothing more is started on the device)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mgmres_ab import ROUNDS, generate  # noqa: E402

DEFAULT = ["unstr:80,80,80", "unstr:80,80,80@tall", "hpcg:128"]
STEP_LIMIT = 560  # seconds per input
SOLVE_TOL, SOLVE_MAX = 1e-8, 2000


def tall_slice(ctx, A, share=0.6):
    """The first `share` of A's columns as a new matrix (host cut of the downloaded CRS)."""
    import numpy as np
    from oracle.pyoracle import CRS
    rp, col, val = A.download()
    nc = int(A.n_cols * share)
    keep = col < nc
    kept_before = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])
    B = ctx.matrix(CRS(A.n_rows, kept_before[rp], col[keep], val[keep], n_cols=nc))
    A.free()
    return B


class Loop:
    """The iteration of include/bis_hip.h call by call: every dot returns to the host, the scalars live in numpy."""

    def __init__(self, ctx, A, At, b, d):
        self.ctx, self.A, self.At, self.b, self.d, self.m, self.n = ctx, A, At, b, d, A.n_rows, A.n_cols
        m, n = self.m, self.n
        self.x, self.u, self.tm = ctx.alloc(n), ctx.alloc(m), ctx.alloc(m)
        self.v, self.h, self.hbar, self.tn, self.w = (ctx.alloc(n) for _ in range(5))

    def init(self):
        import numpy as np
        from lsmr_ref import Scalars, div0
        c, m, n = self.ctx, self.m, self.n
        c.init_vector(self.x, 0.0)
        c.init_vector(self.hbar, 0.0)
        c.compute_residual(self.A, self.x, self.b, self.u, self.tm)
        beta = np.sqrt(np.float64(c.dot(self.u, self.u, m)))
        c.spmv(self.At, self.u, self.tn)
        c.scale(self.tn, self.tn, float(div0(1.0, beta)), n)
        if self.d is not None:
            c.elemwise_mult_vectors(self.tn, self.tn, self.d, n=n)
        alpha = np.sqrt(np.float64(c.dot(self.tn, self.tn, n)))
        self.S = Scalars(beta, alpha, 0.0, 0.0)
        c.scale(self.v, self.tn, float(self.S.ia), n)
        c.copy_vector(self.h, self.v, n)

    def iterate(self, iters):
        import numpy as np
        c, S, m, n, d = self.ctx, self.S, self.m, self.n, self.d
        for _ in range(iters):
            if d is not None:
                c.elemwise_mult_vectors(self.w, self.v, d, n=n)
            c.spmv(self.A, self.w if d is not None else self.v, self.tm)
            c.subtract_vectors(self.u, self.tm, self.u, float(S.cu), m)
            S.set_beta(np.sqrt(np.float64(c.dot(self.u, self.u, m))))
            c.spmv(self.At, self.u, self.tn)
            c.scale(self.tn, self.tn, float(S.ib), n)
            if d is not None:
                c.elemwise_mult_vectors(self.tn, self.tn, d, n=n)
            c.subtract_vectors(self.tn, self.tn, self.v, float(S.beta), n)
            c_hbar, c_x, c_h = S.step(np.sqrt(np.float64(c.dot(self.tn, self.tn, n))))
            c.scale(self.v, self.tn, float(S.ia), n)
            c.subtract_vectors(self.hbar, self.h, self.hbar, float(c_hbar), n)
            if d is not None:
                c.elemwise_mult_vectors(self.w, d, self.hbar, n=n)
            c.sum_vectors(self.x, self.x, self.w if d is not None else self.hbar, float(c_x), n)
            c.subtract_vectors(self.h, self.v, self.h, float(c_h), n)


def legs(ctx, A, At, gen, iters):
    import numpy as np
    m, n = A.n_rows, A.n_cols
    b, x = ctx.upload(np.random.default_rng(1).uniform(-1, 1, m)), ctx.alloc(n)
    rec = dict(input=gen, rows=m, cols=n, nnz=A.nnz, iters=iters)
    for scaled in (False, True):
        tag = "scaled" if scaled else "plain"
        s = ctx.lsmr(A, b, x, At=At, col_scaling="norm" if scaled else None)
        loop = Loop(ctx, A, At, b, s.col_scaling)

        def run_handle():
            ctx.init_vector(x, 0.0)
            s.init(0.0)
            ctx.sync()
            t0 = time.perf_counter()
            s.iterate(iters)
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3 / iters

        def run_loop():
            loop.init()
            ctx.sync()
            t0 = time.perf_counter()
            loop.iterate(iters)
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3 / iters

        runs = {"handle": run_handle, "calls": run_loop}
        for f in runs.values():
            f()
        times = {q: [] for q in runs}
        for _ in range(ROUNDS):
            for q, f in runs.items():
                times[q].append(f())
        med = {q: float(np.median(v)) for q, v in times.items()}
        st = s.status()
        agree = float(np.max(np.abs(st["hist"] - np.array(loop.S.hist)[:len(st["hist"])])) / st["hist"][0])
        bytes_handle = 24.0 * m + (112.0 if scaled else 88.0) * n
        bytes_calls = 40.0 * m + (216.0 if scaled else 144.0) * n
        rec[tag] = dict(median_ms_per_iteration=med, min_ms_per_iteration={q: float(np.min(v)) for q, v in times.items()}, rounds=times,
                        ratio_calls_over_handle=med["calls"] / med["handle"], pass_bytes_handle=bytes_handle, pass_bytes_calls=bytes_calls,
                        histories_apart=agree)
        print(f"{gen} {tag}: handle {med['handle']:.4f} ms, call by call {med['calls']:.4f} ms per iteration over {iters}; ratio "
              f"{med['calls'] / med['handle']:.3f}; pass bytes {bytes_handle / 1e6:.1f} / {bytes_calls / 1e6:.1f} MB; histories apart "
              f"{agree:.1e} [{A.spmv_kernel()} / {At.spmv_kernel()}]", flush=True)
        # one solve
        ctx.init_vector(x, 0.0)
        ctx.sync()
        t0 = time.perf_counter()
        s.init(SOLVE_TOL)
        done = 0
        while done < SOLVE_MAX:
            s.iterate(100)
            done += 100
            st = s.status(hist_cap=SOLVE_MAX + 1)
            if st["iters"] < done:
                break
        rec[tag]["solve"] = dict(tol=SOLVE_TOL, iters=st["iters"], converged=st["converged"], reason=st["reason"],
                                 ms=(time.perf_counter() - t0) * 1e3, ar_reduction=float(st["hist"][-1] / st["hist"][0]),
                                 r_reduction=float(st["hist_r"][-1] / st["hist_r"][0]))
        print(f"{gen} {tag}: solve to {SOLVE_TOL:g}: {st['iters']} iterations, reason {st['reason']}, {rec[tag]['solve']['ms']:.1f} ms, "
              f"ar x {rec[tag]['solve']['ar_reduction']:.2e}, r x {rec[tag]['solve']['r_reduction']:.2e}", flush=True)
        s.free()
    rec.update(spmv_kernel=A.spmv_kernel(), spmv_kernel_At=At.spmv_kernel())
    return rec


def run_input(spec, iters):
    from basic_iterative_solvers_amd import Context
    ctx = Context(0)
    gen, _, cut = spec.partition("@")
    A = generate(ctx, gen)
    if cut == "tall":
        A = tall_slice(ctx, A)
    At = A.transpose()
    rec = legs(ctx, A, At, spec, iters)
    info = ctx.device_info()
    ctx.close()
    return dict(device=info, records=[rec])


def main():
    argv = sys.argv[1:]

    def opt(name, default):
        return argv[argv.index(name) + 1] if name in argv else default

    json_out = opt("--json", None)
    iters = int(opt("--iters", 50))
    taken = {argv[i + 1] for i, a in enumerate(argv[:-1]) if a in ("--json", "--iters")}
    specs = [a for a in argv if not a.startswith("--") and a not in taken] or DEFAULT
    if "--child" in argv:  # one input, in this process
        out = run_input(specs[0], iters)
        if json_out:
            with open(json_out, "w") as f:
                json.dump(out, f, indent=1)
        return 0
    # one child per input, each GPU step under its own time limit; a failing step ends the script
    merged = dict(device=None, records=[])
    for i, spec in enumerate(specs):
        part = f"{json_out}.{i}.part" if json_out else None
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--child", spec, "--iters", str(iters)]
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
