#!/usr/bin/env python3
"""Time the singular-value handle (bis_svds_*, the CLI's -svd K) against the only route there was before it: the eigensolver
handle (bis_eigs_*) in the caller-applied mode on A^T A, two bis_spmv per product.
   python tools/svds_ab.py [INPUT ...] [--json FILE]
INPUT is a generator string, or banded:ROWS,COLS[,PER_ROW[,SEED]] (tests/lsmr_ref.banded, made on the host and uploaded).
Defaults: banded:1500000,800000 (about 1.5 M x 0.8 M) and unstr:80,80,80 (square, non-symmetric).  Per input, k = 4, the
largest values, ncv 20 and 64 for the handle and as many basis blocks for the eigensolver (its ncv = 2 ncv - 1, at most 64:
2 ncv + 1 blocks against ncv + 2), in ONE process on ONE allocation of A and A^T, the two legs alternating round by round,
five rounds (median and minimum), host clock around work that ends in a device synchronise, round 0 a warm-up:
  svds       init + solve to tol 1e-10 (batches of 4 cycles with a status poll): products, restarts, reason, ms, and the
             attained residuals max_i ||A v - sigma u|| + ||A^T u - sigma v|| of the returned vectors, over sigma_max
  eigs       the same for bis_eigs_* on A^T A, which = LA: sigma = sqrt(lambda), v the Ritz vector, u = A v / sigma; its
             test is relative to lambda = sigma^2
  cycle      the second cycle of the handle with tol -1 (nothing stops), bis_svds_iterate(1) after init and one cycle
  close      the closing half step of that cycle driven through op_begin / bis_spmv / op_end minus the half step before
             it: the one-wave SVD kernel and the two compressions, and their share of the cycle
  svd_kernel the same difference at the first restart on a 150 x 130 matrix, where every vector pass is launch latency: the
             one-wave kernel on a bidiagonal B (at ncv = 64 it is the figure the choice of the round-robin order asks for)
Each input runs in a child process of its own under a time limit (a GPU step that fails or runs out of time ends the script:
nothing more is started on the device)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mgmres_ab import ROUNDS, generate  # noqa: E402

DEFAULT = ["banded:1500000,800000", "unstr:80,80,80"]
STEP_LIMIT = 560  # seconds per input
K, TOL, MAX_CYCLES = 4, 1e-10, 200


def keep_count(k, m):
    return min(k + (m - k) // 2, m - 1)


def timed(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    out = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, out


def make(ctx, spec):
    if spec.startswith("banded:"):
        from lsmr_ref import banded
        a = [int(x) for x in spec.split(":")[1].split(",")]
        return ctx.matrix(banded(a[0], a[1], a[2] if len(a) > 2 else 5, a[3] if len(a) > 3 else 1))
    return generate(ctx, spec)


def residuals(ctx, A, At, sigma, U, V):
    """max_i ||A v_i - sigma_i u_i|| + ||A^T u_i - sigma_i v_i|| with the library's products, the rest on the host."""
    import numpy as np
    worst = 0.0
    tm, tn = ctx.alloc(A.n_rows), ctx.alloc(A.n_cols)
    for i, s in enumerate(sigma):
        u, v = ctx.upload(np.ascontiguousarray(U[:, i])), ctx.upload(np.ascontiguousarray(V[:, i]))
        ctx.spmv(A, v, tm)
        ctx.spmv(At, u, tn)
        worst = max(worst, float(np.linalg.norm(tm.to_host() - s * U[:, i]) + np.linalg.norm(tn.to_host() - s * V[:, i])))
        u.free()
        v.free()
    tm.free()
    tn.free()
    return worst


def solve_svds(ctx, A, At, ncv):
    s = ctx.svds(A, k=K, which="LM", ncv=ncv, tol=TOL, At=At)
    ms, st = timed(ctx, lambda: s.solve(max_cycles=MAX_CYCLES, batch=4))
    U, V = s.vectors()
    s.free()
    return dict(ms=ms, st=st, U=U, V=V)


def solve_eigs(ctx, A, At, ncv, work):
    """bis_eigs_* on A^T A in the caller-applied mode: a product is two bis_spmv through `work` (at least A's rows)."""
    import numpy as np
    n = A.n_cols
    s = ctx.eigs(None, k=K, which="LA", ncv=ncv, tol=TOL, n=n)
    l = keep_count(K, ncv)

    def run():
        s.init()
        st = s.status()
        for cycle in range(MAX_CYCLES):
            for _ in range(ncv if cycle == 0 else ncv - l):
                inp, out = s.op_begin()
                ctx.spmv(A, inp, work)
                ctx.spmv(At, work, out)
                s.op_end()
            if cycle % 4 == 3 or cycle == 0:  # the handle's poll: every 4 cycles
                st = s.status()
                if st["stopped"]:
                    break
        return s.status()

    ms, st = timed(ctx, run)
    X = s.vectors() if st["restarts"] else np.zeros((n, K))
    s.free()
    return dict(ms=ms, st=st, X=X)


def cycle_pieces(ctx, A, At, ncv, first=False):
    """ms of the second cycle (first: of nothing) and of what the close of the second (first: the first) cycle adds.  The
    handle runs with tol -1, which no estimate meets (with tol 0 an estimate that has underflowed to 0 does), and every round
    starts from init, so every round times the same restart."""
    import numpy as np
    halves = 2 * ncv if first else 2 * (ncv - keep_count(K, ncv))
    s = ctx.svds(A, k=K, which="LM", ncv=ncv, tol=-1.0, At=At)

    def driven(count):
        for _ in range(count):
            inp, out, tr = s.op_begin()
            ctx.spmv(At if tr else A, inp, out)
            s.op_end()

    rec = dict(cycle=[], close=[])
    live = True
    for r in range(ROUNDS + 1):
        t_cycle = 0.0
        if not first:
            s.init()
            s.iterate(1)
            t_cycle, _ = timed(ctx, lambda: s.iterate(1))  # the second cycle: ncv - l steps
        s.init()
        if not first:
            s.iterate(1)
        driven(halves - 2)
        t_before, _ = timed(ctx, lambda: driven(1))  # the left half of the last step: an ordinary half step with as many blocks
        t_last, _ = timed(ctx, lambda: driven(1))    # the right half: the cycle closes
        st = s.status()
        live = live and not st["stopped"] and st["restarts"] == (1 if first else 2)
        if r:  # round 0 warms up
            rec["cycle"].append(t_cycle)
            rec["close"].append(t_last - t_before)
    s.free()
    out = {q: dict(median=float(np.median(v)), min=float(np.min(v))) for q, v in rec.items()}
    out.update(halves=halves, live=live, finite=bool(np.all(np.isfinite(st["hist"]))))
    return out


def run_input(spec):
    import numpy as np
    from basic_iterative_solvers_amd import Context
    from lsmr_ref import banded
    ctx = Context(0)
    A = make(ctx, spec)
    At = A.transpose()
    tiny = ctx.matrix(banded(150, 130, 5, 1))
    tiny_t = tiny.transpose()
    work = ctx.alloc(max(A.n_rows, A.n_cols))
    rec = dict(input=spec, rows=A.n_rows, cols=A.n_cols, nnz=A.nnz, spmv_kernel=A.spmv_kernel(), spmv_kernel_t=At.spmv_kernel(), k=K)
    tall = A.n_rows >= A.n_cols
    for ncv in (20, 64):
        ncv_e = min(2 * ncv - 1, 64)
        legs = dict(svds=[], eigs=[])
        last = {}
        for r in range(ROUNDS + 1):  # the legs alternate; round 0 warms up
            a = solve_svds(ctx, A, At, ncv)
            # A^T A has the short side's size only when A is tall; a wide A is handed over transposed
            b = solve_eigs(ctx, A, At, ncv_e, work) if tall else solve_eigs(ctx, At, A, ncv_e, work)
            if r:
                legs["svds"].append(a["ms"])
                legs["eigs"].append(b["ms"])
            last = dict(svds=a, eigs=b)
        a, b = last["svds"], last["eigs"]
        smax = float(a["st"]["sigma_ref"]) or 1.0
        res_a = residuals(ctx, A, At, a["st"]["values"], a["U"], a["V"]) / smax
        lam = np.maximum(b["st"]["values"], 0.0)
        sig_b = np.sqrt(lam)
        Vb = b["X"]
        Am, Amt = (A, At) if tall else (At, A)
        Ub = np.zeros((Am.n_rows, K))
        tmp = ctx.alloc(Am.n_rows)
        for i in range(K):
            x = ctx.upload(np.ascontiguousarray(Vb[:, i]))
            ctx.spmv(Am, x, tmp)
            Ub[:, i] = tmp.to_host() / (sig_b[i] if sig_b[i] > 0 else 1.0)
            x.free()
        tmp.free()
        res_b = residuals(ctx, Am, Amt, sig_b, Ub, Vb) / smax
        p = cycle_pieces(ctx, A, At, ncv)
        t = cycle_pieces(ctx, tiny, tiny_t, ncv, first=True)
        out = dict(ncv=ncv, eigs_ncv=ncv_e,
                   svds=dict(ms_median=float(np.median(legs["svds"])), ms_min=float(np.min(legs["svds"])), products=a["st"]["products"],
                             restarts=a["st"]["restarts"], reason=a["st"]["reason"], converged=a["st"]["converged"],
                             values=[float(v) for v in a["st"]["values"]], residual_over_sigma_max=res_a),
                   eigs=dict(ms_median=float(np.median(legs["eigs"])), ms_min=float(np.min(legs["eigs"])), products=b["st"]["products"],
                             spmvs=2 * b["st"]["products"], restarts=b["st"]["restarts"], reason=b["st"]["reason"],
                             converged=b["st"]["converged"], values=[float(v) for v in sig_b], residual_over_sigma_max=res_b),
                   cycle=p, svd_kernel=t["close"], close_share_of_cycle=p["close"]["median"] / p["cycle"]["median"],
                   svd_kernel_share_of_cycle=t["close"]["median"] / p["cycle"]["median"])
        rec[f"ncv{ncv}"] = out
        print(f"{spec} ncv {ncv}: svds {out['svds']['products']} products, {out['svds']['restarts']} restarts, reason {out['svds']['reason']}, "
              f"{out['svds']['ms_median']:.1f} ms (min {out['svds']['ms_min']:.1f}), residual / sigma_max {res_a:.2e}; eigs on A^T A (ncv "
              f"{ncv_e}) {out['eigs']['products']} products = {out['eigs']['spmvs']} SpMV, {out['eigs']['restarts']} restarts, reason "
              f"{out['eigs']['reason']}, {out['eigs']['ms_median']:.1f} ms (min {out['eigs']['ms_min']:.1f}), residual / sigma_max {res_b:.2e}",
              flush=True)
        print(f"{spec} ncv {ncv} (live {p['live']}, {t['live']}): the second cycle ({p['halves']} products) {p['cycle']['median']:.3f} ms; its close (SVD kernel + two "
              f"compressions) {p['close']['median']:.3f} ms = {100 * out['close_share_of_cycle']:.1f} %; the one-wave SVD kernel alone "
              f"(150 x 130) {t['close']['median']:.3f} ms (min {t['close']['min']:.3f}) = {100 * out['svd_kernel_share_of_cycle']:.1f} % of the cycle; "
              f"max |sigma_svds - sigma_eigs| / sigma_max {float(np.max(np.abs(np.array(out['svds']['values']) - sig_b))) / smax:.2e}", flush=True)
    info = ctx.device_info()
    ctx.close()
    return dict(device=info, records=[rec])


def main():
    argv = sys.argv[1:]
    json_out = argv[argv.index("--json") + 1] if "--json" in argv else None
    specs = [a for a in argv if not a.startswith("--") and a != json_out] or DEFAULT
    if "--child" in argv:  # one input, in this process
        out = run_input(specs[0])
        if json_out:
            with open(json_out, "w") as f:
                json.dump(out, f, indent=1)
        return 0
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
