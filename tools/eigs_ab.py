#!/usr/bin/env python3
"""Time the pieces of one cycle of the thick-restart Lanczos handle (bis_eigs_*, the CLI's -eig K) and whole solves.
   python tools/eigs_ab.py [INPUT ...] [--json FILE]
INPUT is a generator string; defaults: anderson:256, hpcg:256.  Per input, k = 4, which = SA, ncv 20 and 64, in ONE process on
ONE allocation of A, five rounds each (median and minimum):
  cycle      one later cycle of the handle (ncv - l steps), bis_eigs_iterate(1)
  products   as many products alone (bis_spmv on the handle's own vectors)
  passes     a cycle's steps driven through op_begin / bis_spmv / op_end, minus the products: multi-dots, updates, scalings and
             the Ritz and compression launches that return at once (per step the mean over the middle steps, times the steps)
  close      the closing step driven the same way minus a product and an ordinary step's passes: the Ritz kernel and the
             compression
  ritz       the same difference on a 125-row matrix (anderson:5), where every vector pass is launch latency: the one-wave
             Ritz kernel (the compression of 125 rows is one workgroup)
  one_pass   one Gram-Schmidt pass instead of two cannot be selected in the handle; its cost is reported as passes / 2, which
             is exact for the traffic (two basis reads and about three passes over W of the seven)
  solve      init + cycles in batches of 4 with a status poll, tol 1e-10, at most 60 cycles: products, restarts, reason, ms
Each input runs in a child process of its own under a time limit (a GPU step that fails or runs out of time ends the script:
nothing more is started on the device)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mgmres_ab import ROUNDS, generate  # noqa: E402

DEFAULT = ["anderson:256", "hpcg:256"]
STEP_LIMIT = 560  # seconds per input
K, WHICH, TOL, MAX_CYCLES = 4, "SA", 1e-10, 60


def keep_count(k, m):
    return min(k + (m - k) // 2, m - 1)


def timed(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def cycle_pieces(ctx, A, ncv):
    """ms of the pieces of one later cycle (ncv - l steps); the handle runs with tol 0: nothing stops."""
    import numpy as np
    l = keep_count(K, ncv)
    steps = ncv - l
    s = ctx.eigs(A, k=K, which=WHICH, ncv=ncv, tol=0.0)
    s.init()
    s.iterate(1)  # the first cycle: from here on every cycle has ncv - l steps

    def driven(count):
        for _ in range(count):
            inp, out = s.op_begin()
            ctx.spmv(A, inp, out)
            s.op_end()

    rec = dict(products=[], passes=[], close=[], cycle=[])
    for r in range(ROUNDS + 1):
        t_cycle = timed(ctx, lambda: s.iterate(1))  # a whole cycle of the handle
        # the next cycle by hand: its first product `steps` times alone, then the steps
        inp, out = s.op_begin()
        t_prod = timed(ctx, lambda: [ctx.spmv(A, inp, out) for _ in range(steps)])
        s.op_end()
        t_mid = timed(ctx, lambda: driven(steps - 2))
        t_last = timed(ctx, lambda: driven(1))
        if r:  # round 0 warms up
            one_product = t_prod / steps
            per_step = t_mid / (steps - 2) - one_product
            rec["cycle"].append(t_cycle)
            rec["products"].append(t_prod)
            rec["passes"].append(per_step * steps)
            rec["close"].append(t_last - one_product - per_step)
    st = s.status()
    s.free()
    out = {q: dict(median=float(np.median(v)), min=float(np.min(v))) for q, v in rec.items()}
    out.update(steps=steps, l=l, live=not st["stopped"], finite=bool(np.all(np.isfinite(st["hist"]))))
    return out


def solve(ctx, A, ncv):
    s = ctx.eigs(A, k=K, which=WHICH, ncv=ncv, tol=TOL)
    ctx.sync()
    t0 = time.perf_counter()
    st = s.solve(max_cycles=MAX_CYCLES, batch=4)
    ms = (time.perf_counter() - t0) * 1e3
    s.free()
    return dict(ms=ms, products=st["products"], restarts=st["restarts"], converged=st["converged"], reason=st["reason"],
                nconv=st["nconv"], values=[float(v) for v in st["values"]], est=[float(v) for v in st["est"]])


def run_input(spec):
    from basic_iterative_solvers_amd import Context
    ctx = Context(0)
    A = generate(ctx, spec)
    tiny = ctx.gen_anderson(5)  # 125 rows: more than ncv = 64, or the first cycle would end on the invariant subspace
    rec = dict(input=spec, rows=A.n_rows, nnz=A.nnz, spmv_kernel=A.spmv_kernel(), k=K, which=WHICH)
    for ncv in (20, 64):
        p = cycle_pieces(ctx, A, ncv)
        t = cycle_pieces(ctx, tiny, ncv)
        p["ritz"] = t["close"]
        p["one_pass_saving"] = dict(median=p["passes"]["median"] / 2)
        p["ritz_share_of_cycle"] = t["close"]["median"] / p["cycle"]["median"]
        p["solve"] = solve(ctx, A, ncv)
        rec[f"ncv{ncv}"] = p
        print(f"{spec} ncv {ncv} ({p['steps']} steps per cycle, l = {p['l']}): cycle {p['cycle']['median']:.3f} ms = products "
              f"{p['products']['median']:.3f} + passes {p['passes']['median']:.3f} + close {p['close']['median']:.3f} (medians of {ROUNDS}); "
              f"Ritz kernel {t['close']['median']:.3f} ms = {100 * p['ritz_share_of_cycle']:.1f} % of the cycle; the second pass costs "
              f"{p['one_pass_saving']['median']:.3f} ms", flush=True)
        sv = p["solve"]
        print(f"{spec} ncv {ncv}: solve k = {K} {WHICH} tol {TOL:g}: {sv['products']} products, {sv['restarts']} restarts, reason "
              f"{sv['reason']}, {sv['nconv']} converged, {sv['ms']:.1f} ms; values {sv['values']}", flush=True)
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
