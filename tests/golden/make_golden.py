#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ FROM THE REFERENCE ITSELF.

Runs only in the build container (needs /root/reference compiled into
oracle/_ref by `make -C oracle ref`).  Outputs are data only: inputs and the
reference's outputs.  OMP_NUM_THREADS is forced to 1 (the reference's
multi-thread reductions are not run-to-run reproducible, SURVEY.md section 5
defect 4).

  FDM-2d-16.mtx, matrix_band_klein.mtx  -- data files shipped with the
      reference (data/matrices/), copied verbatim as input fixtures
  golden_<name>.npz   -- CRS after the reference's reader, split_LU / peel_diag
      outputs, kernel in/out vectors, ILU(0) factors
  histories.json      -- residual histories of the reference's solvers

Inputs that do not exist as files (HPCG-n, Anderson-L) are produced by the
oracle's generators (oracle/bis_oracle.c: orc_gen_hpcg / orc_gen_anderson) and
fed to the reference as CRS arrays; the generator definitions are this repo's
own, the solver outputs are the reference's.
"""
import json
import os
import sys

os.environ["OMP_NUM_THREADS"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

from oracle.pyoracle import CRS, Oracle, Ref  # noqa: E402


def pack(prefix, M, d):
    d[prefix + "_rp"] = M.row_ptr.astype(np.int64)
    d[prefix + "_col"] = M.col.copy()
    d[prefix + "_val"] = M.val.copy()


def kernel_vectors(ref, A, name):
    d = {}
    n = A.n_rows
    rng = np.random.default_rng(12345)
    x = rng.uniform(-1, 1, n)
    y = rng.uniform(-1, 1, n)
    pack("A", A, d)
    d["x"], d["y"] = x, y
    d["spmv"] = ref.spmv(A, x)
    L, Ls, U, Us = ref.split_LU(A)
    for k, M in zip(("L", "Ls", "U", "Us"), (L, Ls, U, Us)):
        pack(k, M, d)
    D, Dinv = ref.peel_diag(L)
    ref.peel_diag(U)
    pack("Lpeeled", L, d)
    pack("Upeeled", U, d)
    d["A_D"], d["A_D_inv"] = D, Dinv
    d["scale"] = ref.extract_scale(A)
    d["sptrsv"] = ref.sptrsv(Ls, D, y)
    d["bsptrsv"] = ref.sptrsv(Us, D, y, backward=True)
    inpl = y.copy()
    d["sptrsv_inplace"] = ref.sptrsv(Ls, D, inpl, x=inpl)
    d["sub"] = ref.subtract_vectors(x, y, 0.37)
    d["sum"] = ref.sum_vectors(x, y, -1.25)
    d["mul"] = ref.elemwise_mult_vectors(x, y, -1.0)
    d["div"] = ref.elemwise_div_vectors(x, D, 1.0)
    d["dot"] = np.array([ref.dot(x, y)])
    d["norm"] = np.array([ref.norm(x)])
    d["scale_vec"] = ref.scale(x, 1.0 / 3.0)
    d["residual"] = ref.compute_residual(A, x, y)
    d["normalize_x"] = ref.normalize_x(d["spmv"], x, D, y)
    ones = np.ones(n)
    for pc in ("none", "j", "gs", "bgs", "sgs", "2st", "s2st"):
        d["pc_" + pc] = ref.apply_preconditioner(pc, Ls, Us, D, Dinv, ones,
                                                 ones, y)
    d["pc_gs_inplace"] = ref.apply_preconditioner("gs", Ls, Us, D, Dinv, ones,
                                                  ones, y, inplace=True)
    # second build configuration: PRECOND_INNER_ITERS=2, PRECOND_OUTER_ITERS=2
    ref2 = Ref("_i2o2")
    for pc in ("j", "gs", "sgs", "2st", "s2st"):
        d["pc22_" + pc] = ref2.apply_preconditioner(pc, Ls, Us, D, Dinv, ones,
                                                    ones, y)
    # real ILU(0) factors (factor_ILU0_old) and their application
    iLs, iLD, iUs, iUD = ref.factor_ilu0(A)
    pack("iluLs", iLs, d)
    pack("iluUs", iUs, d)
    d["iluLD"], d["iluUD"] = iLD, iUD
    d["pc_ilu0"] = ref.apply_preconditioner("ilu0", iLs, iUs, D, Dinv, iLD,
                                            iUD, y)
    # multi-axpy (dgemm_transpose1 as gmres.hpp:358 uses it), in-bounds n_vec
    V = rng.uniform(-1, 1, (6, n))
    yy = rng.uniform(-1, 1, 6)
    d["V"], d["yy"] = V, yy
    d["multi_axpy5"] = ref.dgemm_transpose1(V, yy, 5)
    np.savez_compressed(os.path.join(HERE, f"golden_{name}.npz"), **d)


RUNS = [  # (solver, precond, extra kwargs)
    ("cg", "none", {}), ("cg", "j", {}), ("cg", "gs", {}), ("cg", "bgs", {}),
    ("cg", "sgs", {}), ("cg", "2st", {}), ("cg", "s2st", {}),
    ("cg", "ilu0", dict(ilu_real=True)), ("cg", "j", dict(num_scale=True)),
    ("bi", "none", {}), ("bi", "j", {}), ("bi", "gs", {}), ("bi", "sgs", {}),
    ("bi", "ilu0", dict(ilu_real=True)),
    ("gm", "none", dict(restart_len=50)), ("gm", "j", dict(restart_len=50)),
    ("gm", "gs", dict(restart_len=50)), ("gm", "sgs", dict(restart_len=50)),
    ("gm", "ilu0", dict(restart_len=50, ilu_real=True)),
    ("gm", "gs", dict(restart_len=10)), ("gm", "none", dict(restart_len=10)),
    ("j", "none", {}), ("gs", "none", {}), ("sgs", "none", {}),
]


def histories(ref, orc, mats):
    out = {}
    for name, A in mats.items():
        for solver, pc, kw in RUNS:
            r = ref.solve(A, solver, pc, **kw)
            key = f"{name}|{solver}|{pc}|" + ",".join(
                f"{k}={v}" for k, v in sorted(kw.items()))
            entry = dict(iters=r["iters"], converged=r["converged"],
                         stopping=r["stopping"],
                         final_true_residual=r["final_true_residual"],
                         hist=[float(v) for v in r["hist"]])
            # How far is this history independent of rounding?  The oracle is the same
            # algorithm with different rounding (fma row sums vs the reference's
            # re-associated SIMD sums): the first index where the two part by more
            # than 1e-9 r0 bounds what any other implementation can be compared on.
            o_all = orc.solve(A, solver, pc, **kw)
            n_all = min(len(o_all["hist"]), len(r["hist"]))
            d_all = np.abs(o_all["hist"][:n_all] - r["hist"][:n_all]) / r["hist"][0]
            bad = np.nonzero(~(d_all <= 1e-9))[0]
            entry["stable_len"] = int(bad[0]) if len(bad) else int(n_all)
            if solver == "gm":
                # GMRES restarts read one word past `y` in the reference
                # (SURVEY.md section 5 defect 1).  Keep a restarted history
                # only if it agrees with the defined semantics (y[m] = 0,
                # oracle) -- i.e. the stray word happened to be 0.0; else keep
                # the part before the first restart.
                o = orc.solve(A, solver, pc, **kw)
                m = kw.get("restart_len", 10)
                n = min(len(o["hist"]), len(r["hist"]))
                dev = np.max(np.abs(o["hist"][:n] - r["hist"][:n])) / r["hist"][0]
                finite = bool(np.all(np.isfinite(r["hist"])))
                same_len = len(o["hist"]) == len(r["hist"])
                clean = dev < 1e-12 and finite and same_len
                entry["restart_clean"] = bool(clean)
                if not clean:
                    # agreeing prefix if the two only stop at different rounding-level
                    # iterations, else the part before the first restart
                    keep = n if dev < 1e-12 else min(m + 1, n)
                    entry["hist"] = entry["hist"][:keep]
                    entry["stable_len"] = min(entry["stable_len"], keep)
                    entry["iters"] = None
                    entry["converged"] = None
                    entry["final_true_residual"] = None
            out[key] = entry
    with open(os.path.join(HERE, "histories.json"), "w") as f:
        json.dump(out, f, indent=0)
    return out


# Mid-size inputs: full residual histories of the real reference at sizes where blocks, windows,
# tiles and levels are many -- the HIP path is run on the same generator inputs (device generators, bit-identical to
# the oracle's: tests/test_gpu_kernels.py) to convergence against them.  histories_mid.json, data only.
MID_RUNS = [
    ("hpcg48", "hpcg:48", lambda o: o.gen_hpcg(48), [("cg", "none", {}), ("cg", "j", {}), ("cg", "sgs", {})]),
    ("hpcg32", "hpcg:32", lambda o: o.gen_hpcg(32), [("gs", "none", {}), ("sgs", "none", {}), ("j", "none", {})]),
    ("anderson32_shift9", "anderson:32,shift=9", lambda o: o.gen_anderson(32, shift=9.0),
     # (restart length 50: no restart before convergence -- a restart reads y[m] out of bounds in the reference,
     # SURVEY.md section 5 defect 1, and the history behind it is not defined)
     [("gm", "gs", dict(restart_len=50)), ("j", "none", {}), ("cg", "sgs", {})]),
    ("fem_12x11x10", "fem:12,11,10", lambda o: o.gen_fem(12, 11, 10),
     [("bi", "ilu0", dict(ilu_real=True)), ("cg", "j", {})]),
]


def histories_mid(ref, orc):
    out = {}
    for name, cli_arg, gen, runs in MID_RUNS:
        A = gen(orc)
        for solver, pc, kw in runs:
            r = ref.solve(A, solver, pc, **kw)
            o = orc.solve(A, solver, pc, **kw)
            n = min(len(o["hist"]), len(r["hist"]))
            d = np.abs(o["hist"][:n] - r["hist"][:n]) / r["hist"][0]
            bad = np.nonzero(~(d <= 1e-9))[0]
            key = f"{name}|{solver}|{pc}|" + ",".join(f"{k}={v}" for k, v in sorted(kw.items()))
            out[key] = dict(cli=cli_arg, rows=A.n_rows, nnz=A.nnz, iters=r["iters"], converged=r["converged"],
                            stopping=r["stopping"], final_true_residual=r["final_true_residual"],
                            hist=[float(v) for v in r["hist"]], stable_len=int(bad[0]) if len(bad) else int(n),
                            oracle_max_dev_over_r0=float(np.max(d)))
            print(key, r["iters"], r["converged"], f"oracle dev {np.max(d):.2e}", flush=True)
    with open(os.path.join(HERE, "histories_mid.json"), "w") as f:
        json.dump(out, f, indent=0)
    return out


# Round 4: (i) raw (indefinite) Anderson, the operator of BASELINE configs 2-3 as named: the first 100 CG iterations
# (SURVEY 8d parity gate item ii; cg.hpp:6-54 call order) -- CG need not converge there, the window is what is compared;
# (ii) the unstructured config-5 input (`unstr:`: no grid, no node blocks) with the solver / preconditioner pairs of configs
# 5 and 4.  histories_r4.json, data only.
R4_RUNS = [
    ("anderson16_raw", "anderson:16", lambda o: o.gen_anderson(16), [("cg", "none", dict(max_iters=100))]),
    ("anderson32_raw", "anderson:32", lambda o: o.gen_anderson(32), [("cg", "none", dict(max_iters=100)),
                                                                      ("cg", "j", dict(max_iters=100))]),
    ("unstr_12x11x10", "unstr:12,11,10", lambda o: o.gen_unstr(12, 11, 10),
     [("bi", "ilu0", dict(ilu_real=True)), ("gm", "gs", dict(restart_len=50)), ("cg", "sgs", {}), ("gs", "none", {}),
      # (added later in round 4: the other solver / preconditioner pairs on the matrix without a grid)
      ("gm", "ilu0", dict(ilu_real=True, restart_len=50)), ("cg", "ilu0", dict(ilu_real=True)), ("bi", "sgs", {}), ("cg", "j", {}),
      ("sgs", "none", {}), ("bi", "2st", {}), ("gm", "s2st", dict(restart_len=50))]),
    ("unstr_20x20x20", "unstr:20,20,20", lambda o: o.gen_unstr(20, 20, 20),
     [("bi", "ilu0", dict(ilu_real=True)), ("gm", "gs", dict(restart_len=50)), ("cg", "sgs", {}), ("gm", "ilu0", dict(ilu_real=True, restart_len=50))]),
]


def histories_r4(ref, orc):
    out = {}
    for name, cli_arg, gen, runs in R4_RUNS:
        A = gen(orc)
        for solver, pc, kw in runs:
            r = ref.solve(A, solver, pc, **kw)
            o = orc.solve(A, solver, pc, **kw)
            n = min(len(o["hist"]), len(r["hist"]))
            d = np.abs(o["hist"][:n] - r["hist"][:n]) / r["hist"][0]
            bad = np.nonzero(~(d <= 1e-9))[0]
            key = f"{name}|{solver}|{pc}|" + ",".join(f"{k}={v}" for k, v in sorted(kw.items()))
            out[key] = dict(cli=cli_arg, rows=A.n_rows, nnz=A.nnz, iters=r["iters"], converged=r["converged"],
                            stopping=r["stopping"], final_true_residual=r["final_true_residual"],
                            hist=[float(v) for v in r["hist"]], stable_len=int(bad[0]) if len(bad) else int(n),
                            oracle_max_dev_over_r0=float(np.max(d)))
            print(key, r["iters"], r["converged"], f"oracle dev {np.max(d):.2e} stable {out[key]['stable_len']}", flush=True)
    with open(os.path.join(HERE, "histories_r4.json"), "w") as f:
        json.dump(out, f, indent=0)
    return out


# ILU(0) on adversarial patterns (--ilu-edges-only): the reference's factor_ILU0_old on inputs the solver matrices never
# are -- missing, zero, -0.0 and near-tolerance diagonals, empty rows, entries that cancel to 0, unsorted and unsymmetric
# rows, long rows, rows at the wave kernel's 1024-entry limit, repeated columns, a long dependency chain.  Values are
# dyadic where the pattern allows (power-of-two pivots, small integers), so that every operation is exact and any correctly
# rounded implementation -- fma or not -- gives the same bits; `exact` records, per case, whether that held (checked op by
# op below).  golden_ilu_edges.npz, data only: input CRS, the reference's factors and its ILU(0) apply of a fixed vector.
ILU_EDGES_MTX = "ilu_dups.mtx"


def _rows_crs(rows, n=None):
    """CRS from rows given as lists of (column, value) in stored order."""
    n = len(rows) if n is None else n
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    val = np.array([v for r in rows for _, v in r], dtype=np.float64)
    return CRS(n, rp, col, val)


def _band_rows(n, half, diag=8.0):
    return [[(j, diag if j == i else (-1.0 if (i + j) % 2 else 0.5)) for j in range(max(0, i - half), min(n, i + half + 1))]
            for i in range(n)]


def _two_level(rng, n_src, n_dep, dep_len, src_ulen, extra=None):
    """Rows 0..n_src-1 ("sources") have no L entries, a power-of-two diagonal and U entries to later columns; the dependent
    rows after them eliminate against sources only -- every pivot is a power of two and every update exact.  dep_len /
    src_ulen: row index -> number of L entries / of U entries."""
    n = n_src + n_dep
    rows = []
    for i in range(n_src):
        k = min(src_ulen(i), n - i - 1)
        cols = np.sort(rng.choice(np.arange(i + 1, n), size=k, replace=False)) if k else []
        rows.append([(i, float(2.0 ** int(rng.integers(1, 4))))] + [(int(c), float(rng.integers(-3, 4))) for c in cols])
    for i in range(n_src, n):
        k = min(dep_len(i), n_src)
        cols = np.sort(rng.choice(n_src, size=k, replace=False)) if k else []
        r = [(int(c), float(rng.integers(-4, 5))) for c in cols] + [(i, 64.0)]
        if i + 1 < n:
            r.append((i + 1, 1.0))
        rows.append(r)
    return rows


def _q(x):
    """Random values on a grid of 2^-10: as irregular as uniform ones for the factorisation, but they compress."""
    return np.round(np.asarray(x) * 1024.0) / 1024.0


def _random_pattern(rng, n, band, p_far, max_len, p_dup, p_zero, p_tiny):
    """Unsymmetric, unsorted: a band plus far entries, some repeated columns, explicit zeros, tiny or missing diagonals."""
    rows = []
    for i in range(n):
        k = int(rng.integers(1, max_len + 1))
        c = set(int(v) for v in rng.integers(max(0, i - band), min(n, i + band + 1), size=k))
        if rng.random() < p_far:
            c.add(int(rng.integers(0, n)))
        c.add(i)
        r = [(j, float(_q(rng.uniform(-1, 1)))) for j in c]
        for t, (j, v) in enumerate(r):
            if j == i:
                u = rng.random()
                r[t] = (j, 6.0 + v if u > p_tiny else [1e-9, -1e-9, 0.0, -0.0, 1e-17][int(rng.integers(0, 5))])
            elif rng.random() < p_zero:
                r[t] = (j, 0.0)
        if rng.random() < p_tiny / 2:
            r = [e for e in r if e[0] != i]  # no diagonal
        if r and rng.random() < p_dup:
            r.append((r[int(rng.integers(0, len(r)))][0], float(_q(rng.uniform(-1, 1)))))
        order = rng.permutation(len(r))
        rows.append([r[t] for t in order])
    return rows


def ilu_edge_cases():
    """[(name, CRS)] -- the catalogue, deterministic."""
    rng = np.random.default_rng(20261016)
    tol = 1e-8
    below = float(np.nextafter(tol, 0.0))
    cases = []
    add = lambda name, rows, n=None: cases.append((name, _rows_crs(rows, n)))  # noqa: E731
    # -- pivots: |u_ii| < tol -> sign(u_ii) * repl; the rows that meet them are eliminated against power-of-two pivots
    add("no_diag", [[(0, 4.0), (1, 1.0)], [(0, 2.0), (2, 1.0)], [(1, 2.0), (2, 8.0)], [(3, 2.0)]])
    add("zero_diag", [[(0, 4.0), (2, 1.0)], [(1, 0.0), (2, 2.0)], [(0, 1.0), (1, 2.0), (2, 4.0)]])
    add("negzero_diag", [[(0, 4.0), (1, 2.0)], [(0, 1.0), (1, -0.0)], [(1, 2.0), (2, -0.0)], [(3, 8.0)]])
    add("tol_diag", [[(0, tol)], [(1, -tol)], [(2, below)], [(3, -below)], [(4, 2.0 * tol)], [(5, -2.0 * tol)],
                     [(6, 4.0), (7, 2.0)], [(6, 2.0), (7, 1.0)], [(8, 4.0), (9, -2.0)], [(8, 2.0), (9, -1.0)],
                     [(10, 4.0), (11, 1.0)], [(10, -1.0), (11, -0.25)]])
    # (row 7: 1 - 0.5 * 2 = +0 -> +repl; row 9: -1 - 0.5 * -2 = +0; row 11: -0.25 + 0.25 * 1 = +0 -- and -0.0 above)
    add("tiny_diag", [[(0, 1e-17), (1, 1.0)], [(0, 2.0), (1, 4.0)], [(0, -1e-20), (1, 1.0), (2, -1e-300)],
                      [(2, 4.0), (3, 8.0)]])
    # -- empty rows: the first, one inside, the last
    add("empty_rows", [[], [(1, 4.0), (2, 1.0)], [(1, 2.0), (2, 8.0), (4, 1.0)], [], [(2, 1.0), (3, 2.0), (4, 4.0)], []])
    # -- cancellation: row 3's column 4 becomes exactly 0 after the elimination with row 0, so row 1's update skips it;
    #    explicit zeros in L and U positions
    add("cancel_to_zero", [[(0, 4.0), (4, 2.0)], [(1, 2.0), (4, 1.0)], [(2, 8.0), (3, 0.0)],
                           [(0, 2.0), (1, 2.0), (3, 8.0), (4, 1.0)], [(0, 0.0), (2, 0.0), (4, 16.0)]])
    # -- unsorted rows: reversed, shuffled (a band of half-width 3; 8 on the diagonal)
    band = _band_rows(40, 3)
    add("unsorted_reverse", [list(reversed(r)) for r in band])
    add("unsorted_shuffled", [[r[t] for t in rng.permutation(len(r))] for r in band])
    # -- structurally unsymmetric: U rows with columns the dependent row lacks, L entries whose U row is empty
    add("unsymmetric", [[(0, 4.0), (2, 1.0), (3, 2.0), (5, 1.0)], [(1, 2.0)], [(0, 2.0), (1, 1.0), (2, 8.0)],
                        [(3, 4.0)], [(1, 4.0), (3, 1.0), (4, 2.0)], [(0, 1.0), (4, 1.0), (5, 4.0)]])
    # -- long rows: L parts of 63, 64, 65, 128, 129 entries, U rows longer than 64 (multi-chunk sort and wave paths)
    lens = {200: 63, 201: 64, 202: 65, 203: 128, 204: 129}
    rows = _two_level(rng, 150, 60, lambda i: lens.get(i, 3), lambda i: 70 if i % 10 == 0 else 2)
    for i in lens:
        rows[i] = [rows[i][t] for t in rng.permutation(len(rows[i]))]
    add("long_rows", rows)
    # -- the wave kernels' limit: a row of exactly 1024 entries stays on the wave path, 1025 falls to the lane kernel
    for name, m in (("row_1024", 1024), ("row_1025", 1025)):
        rows = _two_level(rng, 1100, 20, lambda i: 2, lambda i: 1)
        rows[1110] = [(int(c), 1.0) for c in range(m - 2)] + [(1110, 64.0), (1111, 1.0)]
        add(name, rows)
    # -- repeated columns, each kind in a matrix of its own
    add("dup_k", [[(0, 4.0), (1, 1.0)], [(0, 2.0), (0, 1.0), (1, 8.0)]])
    add("dup_diag", [[(0, 4.0), (1, 1.0)], [(0, 2.0), (1, 8.0), (1, 2.0)]])
    add("dup_diag_via_u", [[(0, 4.0), (2, 1.0)], [(1, 4.0)], [(0, 2.0), (2, 8.0), (2, 1.0)]])
    add("dup_u", [[(0, 4.0), (2, 1.0), (2, 2.0), (3, 1.0)], [(1, 8.0)], [(2, 8.0), (3, 2.0)],
                  [(0, 2.0), (2, 4.0), (3, 16.0)]])
    add("dup_three", [[(0, 2.0), (1, 1.0)], [(1, 4.0), (2, 2.0)], [(0, 1.0), (1, 2.0), (2, 8.0), (1, 4.0), (1, 1.0)],
                      [(3, 2.0), (1, 1.0), (3, 4.0), (3, 8.0)]])
    add("dup_nonadjacent", [[(0, 4.0), (2, 4.0)], [(1, 8.0), (3, 1.0)], [(2, 3.25), (0, 2.0), (1, 4.0), (0, 1.0), (3, 0.5)],
                            [(3, 8.0), (1, 2.0), (2, 4.0), (1, -2.0)]])
    rows = _two_level(rng, 100, 30, lambda i: 80 if i == 110 else 3, lambda i: 2)
    rows[110] = rows[110] + [(rows[110][5][0], 2.0), (rows[110][40][0], -1.0)]
    rows[110] = [rows[110][t] for t in rng.permutation(len(rows[110]))]
    add("dup_long_row", rows)
    # -- a long dependency chain: bidiagonal plus random earlier columns (the persistent kernel waits on its flags)
    n = 2500
    rows = []
    for i in range(n):
        r = {i: 8.0}
        if i:
            r[i - 1] = -1.0
        for c in rng.integers(0, i, size=min(i, 1)) if i else []:
            r[int(c)] = 0.5
        if i + 1 < n:
            r[i + 1] = -1.0
        rows.append(list(r.items()))
    add("chain_2500", rows)
    # -- random-valued versions at a few thousand rows
    add("rand_unsorted_dups", _random_pattern(rng, 1200, 6, 0.1, 4, 0.05, 0.05, 0.02))
    add("rand_unsymmetric", _random_pattern(rng, 1200, 40, 0.3, 3, 0.0, 0.02, 0.01))
    rows = _random_pattern(rng, 1000, 4, 0.0, 3, 0.02, 0.02, 0.01)
    for i in range(250, 1000, 250):
        extra = [(int(c), float(_q(rng.uniform(-1, 1)))) for c in rng.choice(i, size=70 + i // 100, replace=False)]
        rows[i] = rows[i] + extra
        rows[i - 150] = rows[i - 150] + [(int(c), float(_q(rng.uniform(-1, 1)))) for c in
                                         rng.choice(np.arange(i - 149, 1000), size=80, replace=False)]
    add("rand_long_rows", rows)
    return cases


def ilu0_exact(A, pivot_tol=1e-8, pivot_repl=1e-4):
    """factor_ILU0_old in Python floats, checking every operation for exactness: True if no operation rounded (then
    fma and mul-then-subtract agree and the factors are the same bits on any correctly rounded implementation)."""
    from fractions import Fraction as F
    n = A.n_rows
    U_rows, U_D = [None] * n, [0.0] * n
    for i in range(n):
        w, idx = {}, []
        for p in range(A.row_ptr[i], A.row_ptr[i + 1]):
            w[int(A.col[p])] = float(A.val[p])
            idx.append(int(A.col[p]))
        idx.sort()
        for k in idx:
            if k >= i:
                break
            pivot = U_D[k]
            if abs(pivot) < 1e-16:
                continue
            f = w[k] / pivot
            if F(f) * F(pivot) != F(w[k]):
                return False
            w[k] = f
            for j, u in U_rows[k]:
                if w.get(j, 0.0) != 0.0:
                    r = w[j] - f * u
                    if F(r) != F(w[j]) - F(f) * F(u):
                        return False
                    w[j] = r
        u_diag = w[i] if i in w else 0.0
        if abs(u_diag) < pivot_tol:
            u_diag = (1.0 if u_diag >= 0 else -1.0) * pivot_repl
        U_D[i] = u_diag
        U_rows[i] = [(j, w[j]) for j in idx if j > i]
    return True


def ilu_edges(ref, orc):
    cases = ilu_edge_cases()
    # the host-CLI fixture: a diagonally dominant matrix whose .mtx splits some entries over two lines
    cases.append(("mtx_dups", ref.read_mtx(os.path.join(HERE, ILU_EDGES_MTX))))
    d = {"names": np.array([c[0] for c in cases]), "exact": np.zeros(len(cases), dtype=np.int8)}
    for t, (name, A) in enumerate(cases):
        n = A.n_rows
        pack(name + "__A", A, d)
        Ls, L_D, Us, U_D = ref.factor_ilu0(A)
        pack(name + "__Ls", Ls, d)
        pack(name + "__Us", Us, d)
        d[name + "__LD"], d[name + "__UD"] = L_D, U_D
        y = _q(np.random.default_rng(1000 + t).uniform(-1, 1, n))
        d[name + "__y"] = y
        d[name + "__pc_ilu0"] = ref.apply_preconditioner("ilu0", Ls, Us, None, None, L_D, U_D, y)
        d["exact"][t] = ilu0_exact(A)
        # the oracle is the spec the GPU tests use where the reference is absent: it must be the reference
        oLs, oL_D, oUs, oU_D = orc.factor_ilu0(A)
        same = all(np.array_equal(a, b) for a, b in ((oLs.row_ptr, Ls.row_ptr), (oLs.col, Ls.col), (oLs.val, Ls.val),
                                                     (oUs.row_ptr, Us.row_ptr), (oUs.col, Us.col), (oUs.val, Us.val),
                                                     (oL_D, L_D), (oU_D, U_D)))
        lens = np.diff(A.row_ptr)
        print(f"{name}: {n} rows, {A.nnz} nnz, longest row {lens.max(initial=0)}, exact {bool(d['exact'][t])}, "
              f"oracle == reference {same}", flush=True)
        assert same, name
    np.savez_compressed(os.path.join(HERE, "golden_ilu_edges.npz"), **d)
    return cases


def main():
    ref, orc = Ref(), Oracle()
    if "--r4-only" in sys.argv:  # leaves the earlier fixtures as they are
        h = histories_r4(ref, orc)
        print(f"wrote {len(h)} round-4 histories")
        return
    if "--ilu-edges-only" in sys.argv:  # leaves the other fixtures as they are
        c = ilu_edges(ref, orc)
        print(f"wrote {len(c)} ILU(0) edge cases")
        return
    if "--mid-only" in sys.argv:  # leaves the small fixtures as they are
        h = histories_mid(ref, orc)
        print(f"wrote {len(h)} mid-size histories")
        return
    mats = {}
    for name in ("FDM-2d-16", "matrix_band_klein"):
        A = ref.read_mtx(os.path.join(HERE, name + ".mtx"))
        mats[name] = A
    mats["hpcg8"] = orc.gen_hpcg(8)
    mats["hpcg_4x6x5"] = orc.gen_hpcg(4, 6, 5)
    mats["anderson8_shift9"] = orc.gen_anderson(8, shift=9.0)
    for name, A in mats.items():
        kernel_vectors(ref, A, name)
    # raw Anderson (indefinite): kernel vectors only + first CG iterations
    kernel_vectors(ref, orc.gen_anderson(6), "anderson6_raw")
    h = histories(ref, orc, mats)
    n_clean = sum(1 for k, v in h.items() if v.get("restart_clean", True))
    print(f"wrote {len(h)} histories ({n_clean} complete) and "
          f"{len(mats) + 1} kernel fixture files")
    histories_mid(ref, orc)
    histories_r4(ref, orc)


if __name__ == "__main__":
    main()
