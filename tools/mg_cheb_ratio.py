#!/usr/bin/env python3
"""CPU only: CG iteration counts with the restated multigrid cycle (tests/mg_cheb_ref.py) under the Chebyshev smoother, for
the choice of its default `ratio` (lambda_max / lambda_min) -- the table of docs/EXPERIMENTS.md.

HPCG 16^3 and 32^3 and the unstructured 8^3 input at coarse_limit 64, plain and smoothed aggregation, degree 2 and 3 at nu = 1,
est_steps 10, safety 1.1, b = A 1, tolerance 1e-10; beside them l1-Jacobi at nu = degree (the same number of SpMVs a cycle).

    python tools/mg_cheb_ratio.py [--ratios 4,10,20,30] [--est 10]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import mg_cheb_ref as cheb  # noqa: E402
import spgemm_ref as ref  # noqa: E402
import test_gpu_mg as base  # noqa: E402
from oracle.pyoracle import Oracle  # noqa: E402


def scipy_product(A, B):
    C = (A.to_scipy() @ B.to_scipy()).tocsr()
    C.sort_indices()
    return ref.crs(A.n_rows, B.n_cols, C.indptr, C.indices, C.data)


def iterations(A, levels, b, cfg):
    hist, _ = base.numpy_pcg(A, lambda r: cheb.cycle(levels, r, cfg), b, 1e-10, 300)
    return len(hist) - 1 if hist[-1] < 1e-10 * hist[0] else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ratios", default="4,10,20,30")
    ap.add_argument("--est", type=int, default=10)
    ap.add_argument("--degrees", default="2,3")
    a = ap.parse_args()
    ratios = [float(r) for r in a.ratios.split(",")]
    degrees = [int(d) for d in a.degrees.split(",")]
    o = Oracle()
    inputs = [("hpcg16", o.gen_hpcg(16), (16, 16, 16, 1)), ("hpcg32", o.gen_hpcg(32), (32, 32, 32, 1)), ("unstr8", o.gen_unstr(8, 8, 8), None)]
    total = {r: 0 for r in ratios}
    print("| input | hierarchy | degree | Jacobi nu=degree | " + " | ".join(f"ratio {r:g}" for r in ratios) + " |")
    print("|---|---|---|---|" + "---|" * len(ratios))
    for name, A0, grid in inputs:
        A = ref.crs(A0.n_rows, A0.n_rows, A0.row_ptr, A0.col, A0.val)
        b = base.host_spmv(A, np.ones(A.n_rows))
        for kind in ("plain", "smoothed"):
            levels = base.hierarchy_reference(A, grid, coarse_limit=64) if kind == "plain" else \
                ref.hierarchy(A, grid, coarse_limit=64, product=scipy_product)
            spec = [cheb.spectrum(L["A"], L["w"], 2.0, a.est, 1.1) for L in levels]
            print(f"<!-- {name} {kind}: rows {[L['A'].n_rows for L in levels]}, bound {[float(s['bound']) for s in spec]}, "
                  f"estimate {[float(s['estimate']) for s in spec]} -->", flush=True)
            for m in degrees:
                row = [iterations(A, levels, b, cheb.config(nu=m))]
                for r in ratios:
                    sm = cheb.smoother(levels, degree=m, ratio=r, est_steps=a.est, safety=1.1)
                    it = iterations(A, levels, b, cheb.config(cheb=sm))
                    row.append(it)
                    total[r] += it if it is not None else 300
                print(f"| {name} | {kind} | {m} | " + " | ".join("-" if v is None else str(v) for v in row) + " |", flush=True)
    print("| total | | | | " + " | ".join(str(total[r]) for r in ratios) + " |")


if __name__ == "__main__":
    main()
