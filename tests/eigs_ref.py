"""The thick-restart Lanczos eigensolver of include/bis_hip.h (bis_eigs_*) restated in numpy, line by line, with the order
of the sums as an argument, and the inputs the eigensolver tests share.  Not a test file.

The header's "one fma per element and block" lines use lsmr_ref.fma (the product kept exactly); the one-wave lines (the
Jacobi rotations, the estimates, the test) round every operation separately, as the device's lanes do.

INPUTS records, per row of the issue's table, the generator arguments chosen so that the restatement's deciding estimate
sits at most at half its threshold at the last restart and at least at twice the threshold at the restart before it
(tests/test_eigs_ref_cpu.py asserts both): equal restart counts are then a fair demand on the device."""
import numpy as np

from idr_ref import hashed_shadow
from lsmr_ref import dense_of, fma, from_triplets, host_spmv  # noqa: F401  (re-exported for the tests)

EPS = np.finfo(np.float64).eps
EPS23 = EPS ** (2.0 / 3.0)
MAX_SWEEPS = 30
REASONS = {0: "live", 1: "converged", 2: "invariant", 3: "jacobi", 4: "bad_start"}
LIVE, CONVERGED, INVARIANT, JACOBI, BAD_START = range(5)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def sym_banded(n, half, seed):
    """Symmetric CRS: bands d = 0 .. half with uniform(-1, 1) entries from default_rng(seed), the diagonal times 4."""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for d in range(min(half, n - 1) + 1):
        v = rng.uniform(-1.0, 1.0, n - d)
        i = np.arange(n - d, dtype=np.int64)
        if d == 0:
            rows.append(i); cols.append(i); vals.append(4.0 * v)
        else:
            rows += [i, i + d]; cols += [i + d, i]; vals += [v, v]
    return from_triplets(n, n, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


def default_ncv(n, k):
    return min(n, 64, max(2 * k + 1, 20))


def keep_count(k, m):
    return min(k + (m - k) // 2, m - 1)


# name -> (generator, arguments, k, ncv, the `which` values): the issue's table with the seeds, and where no seed would do the
# ncv, chosen for the margins.  Two rows moved off the table's ncv: hpcg 16 -> 17 (at 16 SA's last estimate sits at 0.72 of
# its threshold, and the generator has no seed), band515 3 -> 16 (with ncv = k + 1 a cycle adds one vector to l = m - 1 kept
# ones, the estimates fall by one to five percent per restart and no seed of 39 tried comes near a factor 2 on either side:
# the restatement's last two ratios were 1.00 .. 1.05 and 0.94 .. 0.999).  EXTRA_KP1 is that shape, kept as a test of its own
# that demands no equal restart count.
INPUTS = {
    "anderson5": ("anderson", dict(L=5, seed=33), 3, 12, ("SA", "LA")),
    "anderson8": ("anderson", dict(L=8, seed=2), 4, 24, ("SA", "LA", "LM")),
    "anderson11": ("anderson", dict(L=11, seed=1), 6, 64, ("SA",)),
    "hpcg5x7x37": ("hpcg", dict(nx=5, ny=7, nz=37), 2, 17, ("SA", "LA")),
    "band1301": ("banded", dict(n=1301, half=5, seed=1), 5, 32, ("LM",)),
    "band515": ("banded", dict(n=515, half=2, seed=2), 2, 16, ("LA",)),
    "band7": ("banded", dict(n=7, half=2, seed=1), 2, 7, ("LM",)),
    "band3": ("banded", dict(n=3, half=1, seed=1), 1, 3, ("SA",)),
}
EXTRA_KP1 = dict(n=515, half=2, seed=29, k=2, ncv=3, which="LA")  # the restatement: 327 restarts, ratios 1.03 and 0.956
ROWS = [(name, which) for name, e in INPUTS.items() for which in e[4]]


def make_input(name, gen):
    """The host CRS of a table row; gen: an object with gen_anderson / gen_hpcg returning something with row_ptr, col, val
    (the oracle, or a wrapper that downloads the device's matrix)."""
    kind, args = INPUTS[name][:2]
    if kind == "anderson":
        return gen.gen_anderson(args["L"], seed=args["seed"])
    if kind == "hpcg":
        return gen.gen_hpcg(args["nx"], args["ny"], args["nz"])
    return sym_banded(args["n"], args["half"], args["seed"])


# ---- the sums ----------------------------------------------------------------------------------------------------------
def dots_np(V, w):
    return np.asarray(V @ w, dtype=np.float64)


def dots_long(V, w):
    return np.asarray(V.astype(np.longdouble) @ w.astype(np.longdouble), dtype=np.float64)


def dots_blocks(V, w):
    s = np.zeros(V.shape[0])
    for i in range(0, len(w), 256):
        s = s + V[:, i:i + 256] @ w[i:i + 256]
    return s


DOTS = dict(np=dots_np, long=dots_long, blocks=dots_blocks)


# ---- the restart's dense eigen-solve -------------------------------------------------------------------------------------
def off_norm(T):
    """off(T) from the off-diagonal entries themselves: column sums in row order, added in column order."""
    S = T * T
    np.fill_diagonal(S, 0.0)
    col = np.add.reduce(S, axis=0)
    return np.sqrt(np.add.accumulate(col)[-1])


def fro_norm(T):
    col = np.add.reduce(T * T, axis=0)
    return np.sqrt(np.add.accumulate(col)[-1])


def jacobi(T):
    """Cyclic Jacobi as the header states it: (theta, Y, sweeps, ok) with T = Y diag(theta) Y^T, theta unsorted."""
    T = np.array(T, dtype=np.float64)
    m = T.shape[0]
    Y = np.eye(m)
    fro = fro_norm(T)
    sweeps = 0
    while True:  # (the caller keeps numpy quiet: tau^2 may overflow, t is then 0 as on the device)
        if off_norm(T) <= EPS * fro:
            return np.diag(T).copy(), Y, sweeps, True
        if sweeps == MAX_SWEEPS:
            return np.diag(T).copy(), Y, sweeps, False
        for p in range(m - 1):
            for q in range(p + 1, m):
                apq = T[p, q]
                if apq == 0.0:
                    continue
                app, aqq = T[p, p], T[q, q]
                tau = (aqq - app) / (2.0 * apq)
                root = np.sqrt(1.0 + tau * tau)
                t = 1.0 / (tau + root if tau >= 0.0 else tau - root)
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
                rho = s / (1.0 + c)
                tp, tq = T[p, :].copy(), T[q, :].copy()
                new_p, new_q = tp - s * (tq + rho * tp), tq + s * (tp - rho * tq)
                T[p, :] = new_p; T[:, p] = new_p
                T[q, :] = new_q; T[:, q] = new_q
                T[p, p] = app - t * apq
                T[q, q] = aqq + t * apq
                T[p, q] = T[q, p] = 0.0
                yp, yq = Y[:, p].copy(), Y[:, q].copy()
                Y[:, p] = yp - s * (yq + rho * yp)
                Y[:, q] = yq + s * (yp - rho * yq)
        sweeps += 1


def rank_order(theta, which):
    """The columns in rank order: ascending (stable), then SA as sorted, LA descending, LM descending |theta| (stable)."""
    asc = np.argsort(theta, kind="stable")
    if which == "SA":
        return asc
    key = -theta[asc] if which == "LA" else -np.abs(theta[asc])
    return asc[np.argsort(key, kind="stable")]


def assemble_T(theta, s, alpha, beta, l, m):
    T = np.zeros((m, m))
    for i in range(l):
        T[i, i] = theta[i]
        T[i, l] = T[l, i] = s[i]
    for j in range(l, m):
        T[j, j] = alpha[j]
        if j + 1 < m:
            T[j, j + 1] = T[j + 1, j] = beta[j]
    return T


# ---- the method ----------------------------------------------------------------------------------------------------------
def eigs(matvec, n, k, ncv=None, which="SA", tol=1e-10, v0=None, max_cycles=200, dots=dots_np, passes=2):
    """Thick-restart Lanczos as the header states it.  Returns dict(products, restarts, stopped, converged, reason, nconv,
    values, est, hist, hist_nconv, X (n x k, the first k basis blocks), ratios (per restart max_i est_i / threshold_i),
    sweeps (per restart))."""
    m = default_ncv(n, k) if ncv is None else ncv
    assert 1 <= k < m <= min(n, 64)
    l_keep = keep_count(k, m)
    out = dict(products=0, restarts=0, stopped=False, converged=False, reason=LIVE, nconv=0, values=np.zeros(k), est=np.zeros(k),
               hist=[], hist_nconv=[], ratios=[], sweeps=[], X=None)
    v0 = hashed_shadow(n, 1)[:, 0] if v0 is None else np.asarray(v0, dtype=np.float64)
    with np.errstate(all="ignore"):
        nrm = np.sqrt(dots(v0[None, :], v0)[0])
    if not (nrm > 0.0) or not np.isfinite(nrm):
        out.update(stopped=True, reason=BAD_START, hist=np.zeros(0), hist_nconv=np.zeros(0, dtype=np.int64))
        return out
    V = np.zeros((m + 1, n))
    V[0] = v0 / nrm
    alpha, beta, theta, s = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m)
    l = 0

    def restart(me, broke):
        nonlocal l, theta, s
        th, Y, sweeps, ok = jacobi(assemble_T(theta, s, alpha, beta, l, me))
        order = rank_order(th, which)
        nr = min(k, me)
        beta_last = beta[me - 1]
        vals = th[order[:nr]]
        est = np.abs(beta_last * Y[me - 1, order[:nr]])
        thr = tol * np.maximum(np.abs(vals), EPS23)
        nconv = int(np.sum(est <= thr))
        out["values"][:nr], out["est"][:nr] = vals, est
        out["hist"].append(float(np.max(est)))
        out["hist_nconv"].append(nconv)
        out["ratios"].append(float(np.max(est / thr)))
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
        Yk = Y[:me, order[:l_out]]
        a = np.zeros((l_out, n))
        for b in range(me):  # one fma per block from 0, ascending
            a = fma(Yk[b][:, None], V[b][None, :], a)
        tail = V[me].copy()
        V[:l_out] = a
        if reason != LIVE:
            out.update(stopped=True, reason=reason)
            return
        V[l_out] = tail
        theta[:l_out] = th[order[:l_out]]
        s[:l_out] = beta_last * Y[me - 1, order[:l_out]]
        l = l_out

    cycles = 0
    old_err = np.seterr(all="ignore")
    while not out["stopped"] and cycles < max_cycles:
        for j in range(l, m):
            w = np.asarray(matvec(V[j]), dtype=np.float64).copy()
            size = np.sqrt(dots(w[None, :], w)[0])  # || OP V_j ||, summed with the first group of h
            aj = 0.0
            for _ in range(passes):
                h = dots(V[:j + 1], w)
                for b in range(j + 1):
                    w = fma(-h[b], V[b], w)
                aj = aj + h[j]
            alpha[j] = aj
            beta[j] = np.sqrt(dots(w[None, :], w)[0])
            out["products"] += 1
            if beta[j] <= EPS * size:  # an invariant subspace: beta_j is 0 or the rounding noise that is left of it
                beta[j] = 0.0
                restart(j + 1, True)
                break
            V[j + 1] = w / beta[j]
        else:
            restart(m, False)
        cycles += 1
    np.seterr(**old_err)
    out["hist"] = np.array(out["hist"])
    out["hist_nconv"] = np.array(out["hist_nconv"], dtype=np.int64)
    out["X"] = V[:k].T.copy()
    return out


def eigen_bound(D, values, X):
    """Per returned pair (x normalised): (|theta - nearest lambda|, ||A x - theta x||_2 + 64 eps ||A||_1), and the dense
    spectrum: the theorem for symmetric A says the first is at most the residual norm."""
    lam = np.linalg.eigvalsh(D)
    norm1 = np.max(np.sum(np.abs(D), axis=0))
    dist, bound = [], []
    for i, th in enumerate(values):
        x = X[:, i] / np.linalg.norm(X[:, i])
        dist.append(np.min(np.abs(lam - th)))
        bound.append(np.linalg.norm(D @ x - th * x) + 64 * EPS * norm1)
    return np.array(dist), np.array(bound), lam


def hist_scale(hist, norm1):
    """What the history gate is relative to: entry 0, but not less than 64 eps ||A||_1.  With ncv = n the last beta of the
    only cycle is rounding noise (exactly 0 in exact arithmetic: the basis spans the whole space), so is entry 0, and two
    orders of the sums agree on it to no digit; an estimate below the rounding level of one product carries no information."""
    return max(float(hist[0]), 64 * EPS * norm1)


def norm1_of(A):
    return float(np.max(np.bincount(A.col, weights=np.abs(A.val), minlength=A.n_cols)))


def wanted(lam, k, which):
    """The k wanted eigenvalues of the ascending spectrum in rank order, and the nearest unwanted one(s)."""
    order = rank_order(lam, which)
    return lam[order[:k]], lam[order[k:]]
