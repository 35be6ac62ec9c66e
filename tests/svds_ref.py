"""The thick-restart Lanczos bidiagonalisation of include/bis_hip.h (bis_svds_*) restated in numpy, line by line, with the
order of the sums as an argument (eigs_ref.DOTS: np, long, blocks), and the inputs the singular-value tests share.  Not a
test file.

The header's "one fma per element and block" lines use lsmr_ref.fma (the product kept exactly); the one-wave lines (the
Jacobi rotations and their three sums, the norms of the columns, the estimates, the test) round every operation
separately and add in row order, as the device's lanes do.  The pairs of one round of the round-robin schedule are
disjoint, so the restatement rotates them at once, as the lanes do.

TABLE records, per row of the issue's table, the arguments chosen so that the restatement's deciding ratio
max est / (tol sigma_ref) sits at most at 0.5 at the last restart and at least at 2 at the restart before it
(tests/test_svds_ref_cpu.py asserts both): equal restart counts are then a fair demand on the device."""
import numpy as np

from eigs_ref import DOTS, dots_np  # noqa: F401  (re-exported for the tests)
from idr_ref import hashed_shadow
from lsmr_ref import banded, dense_of, fma, host_spmv, table_matrix, transposed  # noqa: F401

EPS = np.finfo(np.float64).eps
MAX_SWEEPS = 30
REASONS = {0: "live", 1: "converged", 2: "invariant", 3: "jacobi", 4: "bad_start"}
LIVE, CONVERGED, INVARIANT, JACOBI, BAD_START = range(5)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def default_ncv(ns, k):
    return min(ns, 64, max(2 * k + 1, 20))


def keep_count(k, m):
    return min(k + (m - k) // 2, m - 1)


# name -> (generator, arguments, which, k, ncv): the issue's table and its 3 x 2 row.  One row moved: S SM from ncv = 24 to
# 36.  At 24 the restatement stops after 20 restarts with the ratios 0.115 and 1.49, as the issue's prototype did: the
# restart before the last is within a factor 1.5 of the threshold.  Of ncv = 20 .. 40 the values 28 (2.53 / 0.278), 36
# (2.73 / 0.0206) and 40 (17.3 / 0.435) meet both margins; 36 has the most room on the side that 24 missed by the most and
# walks more than four groups of basis blocks.
TABLE = {
    "T-LM": ("table", "T", "LM", 4, 20),
    "T-SM": ("table", "T", "SM", 3, 24),
    "W-LM": ("table", "W", "LM", 4, 20),
    "W-SM": ("table", "W", "SM", 3, 24),
    "S-LM": ("table", "S", "LM", 4, 20),
    "S-SM": ("table", "S", "SM", 3, 36),
    "B2100-LM": ("banded", (2100, 1500, 6, 7), "LM", 6, 64),
    "B2100-SM": ("banded", (2100, 1500, 6, 7), "SM", 2, 40),
    "B7x40-LM": ("banded", (7, 40, 3, 6), "LM", 2, 6),
    "B40x7-LM": ("banded", (40, 7, 3, 5), "LM", 2, 7),
    "B3x2-LM": ("banded", (3, 2, 2, 1), "LM", 1, 2),
}
ROWS = list(TABLE)


def make_input(name):
    """The host CRS of a table row."""
    kind, args = TABLE[name][:2]
    return table_matrix(args) if kind == "table" else banded(*args)


def diag_rect(rows, cols, d):
    """The rectangular "diagonal" matrix a_ii = d_i (every entry stored, zeros too)."""
    from oracle.pyoracle import CRS
    n = min(rows, cols)
    row_ptr = np.minimum(np.arange(rows + 1, dtype=np.int64), n)
    return CRS(rows, row_ptr, np.arange(n, dtype=np.int32), np.asarray(d, dtype=np.float64), n_cols=cols)


# ---- the restart's dense SVD ---------------------------------------------------------------------------------------------
def round_pairs(me, r):
    """The pairs (p < q) of round r of the round-robin schedule of me columns; the bye of an odd me is left out."""
    n2 = (me + 1) & ~1
    n1 = n2 - 1
    out = []
    for lane in range(n2 // 2):
        x, y = (n1, r) if lane == 0 else ((r + lane) % n1, (r - lane) % n1)
        p, q = min(x, y), max(x, y)
        if q < me:
            out.append((p, q))
    return out


def seq_sum(M):
    """Column sums of M, added in row order from 0."""
    return np.add.accumulate(M, axis=0)[-1]


def jacobi_svd(B):
    """One-sided Jacobi as the header states it: (sigma, X, Y, sweeps, ok) with B = X diag(sigma) Y^T, sigma unsorted;
    sweeps counts the last one, which rotated nothing."""
    G = np.array(B, dtype=np.float64)
    me = G.shape[0]
    Y = np.eye(me)
    n2 = (me + 1) & ~1
    thr = np.sqrt(np.float64(me)) * EPS
    sweeps, ok = 0, False
    with np.errstate(all="ignore"):
        floor = EPS * np.sqrt(np.add.accumulate(seq_sum(G * G))[-1])  # eps ||B||_F: column sums in row order, added in column order
        while sweeps < MAX_SWEEPS and not ok:
            rotated = False
            for r in range(n2 - 1):
                pairs = round_pairs(me, r)
                if not pairs:
                    continue
                p = np.array([x[0] for x in pairs])
                q = np.array([x[1] for x in pairs])
                gp, gq = G[:, p], G[:, q]
                a, b, c = seq_sum(gp * gp), seq_sum(gq * gq), seq_sum(gp * gq)
                act = (c != 0.0) & (np.abs(c) > thr * np.sqrt(a) * np.sqrt(b)) & (np.sqrt(a) > floor) & (np.sqrt(b) > floor)
                if not np.any(act):
                    continue
                rotated = True
                p, q, a, b, c = p[act], q[act], a[act], b[act], c[act]
                zeta = (b - a) / (2.0 * c)
                root = np.sqrt(1.0 + zeta * zeta)
                t = 1.0 / np.where(zeta >= 0.0, zeta + root, zeta - root)
                cs = 1.0 / np.sqrt(1.0 + t * t)
                sn = t * cs
                for M in (G, Y):
                    u, v = M[:, p].copy(), M[:, q].copy()
                    M[:, p] = cs * u - sn * v
                    M[:, q] = sn * u + cs * v
            sweeps += 1
            ok = not rotated
        sigma = np.sqrt(seq_sum(G * G))
        sigma = np.where(sigma > floor, sigma, 0.0)  # the rounding noise of a zero singular value is a zero column
        X = np.where(sigma != 0.0, G / np.where(sigma != 0.0, sigma, 1.0), 0.0)
    return sigma, X, Y, sweeps, ok


def rank_order(sigma, which):
    """The columns in rank order: ascending (stable), then SM as sorted, LM descending (stable on the sorted list)."""
    asc = np.argsort(sigma, kind="stable")
    if which == "SM":
        return asc
    return asc[np.argsort(-sigma[asc], kind="stable")]


def assemble_B(sigma, s, alpha, beta, l, me):
    B = np.zeros((me, me))
    for i in range(l):
        B[i, i] = sigma[i]
        B[i, l] = s[i]
    for j in range(l, me):
        B[j, j] = alpha[j]
        if j + 1 < me:
            B[j, j + 1] = beta[j]
    return B


# ---- the method ----------------------------------------------------------------------------------------------------------
def svds(A, At, k, ncv=None, which="LM", tol=1e-10, v0=None, max_cycles=200, dots=dots_np, spmv=host_spmv):
    """bis_svds_init + bis_svds_iterate(max_cycles) + bis_svds_status + bis_svds_vectors.  A, At: host CRS (At = A^T).
    Returns dict(products, restarts, stopped, converged, reason, nconv, sigma_ref, values, est, hist, hist_nconv, U (rows x k),
    V (cols x k), ratios (per restart max_i est_i / (tol sigma_ref)), sweeps (per restart))."""
    rows, cols = A.n_rows, A.n_cols
    flip = rows < cols
    F, Ft = (At, A) if flip else (A, At)
    ns, nl = min(rows, cols), max(rows, cols)
    m = default_ncv(ns, k) if ncv is None else ncv
    assert 1 <= k < m <= min(ns, 64) and ns >= 2
    l_keep = keep_count(k, m)
    out = dict(products=0, restarts=0, stopped=False, converged=False, reason=LIVE, nconv=0, sigma_ref=0.0, values=np.zeros(k),
               est=np.zeros(k), hist=[], hist_nconv=[], ratios=[], sweeps=[], U=None, V=None)
    v0 = hashed_shadow(ns, 1)[:, 0] if v0 is None else np.asarray(v0, dtype=np.float64)
    with np.errstate(all="ignore"):
        nrm = np.sqrt(dots(v0[None, :], v0)[0])
    if not (nrm > 0.0) or not np.isfinite(nrm):
        out.update(stopped=True, reason=BAD_START, hist=np.zeros(0), hist_nconv=np.zeros(0, dtype=np.int64))
        return out
    P, Q = np.zeros((m + 1, ns)), np.zeros((m, nl))
    P[0] = v0 / nrm
    alpha, beta, sigma, s = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m)
    l = 0

    def compress(V, C, me, l_out):
        a = np.zeros((l_out, V.shape[1]))
        for b in range(me):  # one fma per block from 0, ascending
            a = fma(C[b][:, None], V[b][None, :], a)
        return a

    def restart(me, broke):
        nonlocal l
        sg, X, Y, sweeps, ok = jacobi_svd(assemble_B(sigma, s, alpha, beta, l, me))
        order = rank_order(sg, which)
        nr = min(k, me)
        beta_last = beta[me - 1]
        out["sigma_ref"] = sref = max(out["sigma_ref"], float(np.max(sg)))
        vals = sg[order[:nr]]
        est = np.abs(beta_last * X[me - 1, order[:nr]])
        nconv = int(np.sum(est <= tol * sref))
        out["values"][:nr], out["est"][:nr] = vals, est
        out["hist"].append(float(np.max(est)))
        out["hist_nconv"].append(nconv)
        out["ratios"].append(float(np.max(est) / (tol * sref)) if sref > 0 else 0.0)
        out["sweeps"].append(sweeps)
        out["restarts"] += 1
        out["nconv"] = nconv
        reason = LIVE
        if broke:
            reason, out["converged"], out["nconv"] = INVARIANT, me >= k, nr
        elif not ok:
            reason = JACOBI
        elif nconv == k:
            reason, out["converged"] = CONVERGED, True
        l_out = nr if reason != LIVE else l_keep
        keep = order[:l_out]
        tail = P[me].copy()
        P[:l_out] = compress(P, Y[:me, keep], me, l_out)
        Q[:l_out] = compress(Q, X[:me, keep], me, l_out)
        if reason != LIVE:
            out.update(stopped=True, reason=reason)
            return
        P[l_out] = tail
        sigma[:l_out] = sg[keep]
        s[:l_out] = beta_last * X[me - 1, keep]
        l = l_out

    def orthogonalise(w, Bs):
        """(the vector after two passes, its norm, the norm before)"""
        if len(Bs) == 0:
            nrm = np.sqrt(dots(w[None, :], w)[0])
            return w, nrm, nrm
        before = np.sqrt(dots(w[None, :], w)[0])  # summed with the first group of the first pass
        for _ in range(2):
            h = dots(Bs, w)
            for b in range(len(Bs)):
                w = fma(-h[b], Bs[b], w)
        return w, np.sqrt(dots(w[None, :], w)[0]), before

    cycles = 0
    old_err = np.seterr(all="ignore")
    while not out["stopped"] and cycles < max_cycles:
        for j in range(l, m):
            w, alpha[j], before = orthogonalise(np.asarray(spmv(F, P[j]), dtype=np.float64).copy(), Q[:j])
            out["products"] += 1
            if alpha[j] <= EPS * before:  # F maps span(P_0..P_j) into span(Q_0..Q_{j-1})
                alpha[j] = beta[j] = 0.0
                Q[j] = 0.0
                restart(j + 1, True)
                break
            Q[j] = w / alpha[j]
            w, beta[j], before = orthogonalise(np.asarray(spmv(Ft, Q[j]), dtype=np.float64).copy(), P[:j + 1])
            out["products"] += 1
            if beta[j] <= EPS * before:  # an invariant subspace
                beta[j] = 0.0
                restart(j + 1, True)
                break
            P[j + 1] = w / beta[j]
        else:
            restart(m, False)
        cycles += 1
    np.seterr(**old_err)
    out["hist"] = np.array(out["hist"])
    out["hist_nconv"] = np.array(out["hist_nconv"], dtype=np.int64)
    left, right = (P, Q) if flip else (Q, P)
    out["U"], out["V"] = left[:k].T.copy(), right[:k].T.copy()
    return out


# ---- what the tests measure ----------------------------------------------------------------------------------------------
def wanted(sv, k, which):
    """The k wanted singular values of numpy's (descending, min(rows, cols) of them) in rank order."""
    return sv[:k] if which == "LM" else sv[::-1][:k]


def residuals(D, values, U, V):
    """Per triplet ||A v - sigma u||_2 + ||A^T u - sigma v||_2."""
    return np.array([np.linalg.norm(D @ V[:, i] - values[i] * U[:, i]) + np.linalg.norm(D.T @ U[:, i] - values[i] * V[:, i])
                     for i in range(len(values))])


def orth_defect(X):
    return float(np.max(np.abs(X.T @ X - np.eye(X.shape[1]))))


def norm1_of(A):
    return float(np.max(np.bincount(A.col, weights=np.abs(A.val), minlength=A.n_cols)))


def hist_scale(hist, norm1):
    """What the history gate is relative to: entry 0, but not less than 64 eps ||A||_1 (with ncv = ns, and at a breakdown,
    entry 0 is 0)."""
    return max(float(hist[0]) if len(hist) else 0.0, 64 * EPS * norm1)
