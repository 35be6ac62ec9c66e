"""The numpy restatement of right-preconditioned IDR(s) with biorthogonalisation as include/bis_hip.h states it for
bis_idr_*: the hashed shadow space and the method, one function each.  Test infrastructure: it runs on the host only."""
import numpy as np


def hash32(x):
    """The header's hash32 on a uint32 array."""
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def hashed_shadow(n, s):
    """P (n x s): P[i][j] = (h + 0.5) 2^-31 - 1, h = hash32(hash32(i) ^ ((j + 1) 0x9e3779b9 mod 2^32))."""
    hi = hash32(np.arange(n, dtype=np.uint32))
    P = np.empty((n, s))
    for j in range(s):
        salt = np.uint32(((j + 1) * 0x9e3779b9) & 0xffffffff)
        P[:, j] = (hash32(hi ^ salt).astype(np.float64) + 0.5) * 2.0 ** -31 - 1.0
    return P


def idr(matvec, b, x0, s, tol, max_iters, apply=None, P=None, sequential=False, acc=np.float64):
    """IDR(s) on A x = b from x0: `matvec(v)` is A v, `apply(v)` is M^-1 v (None: no preconditioner), P the shadow space
    (None: the hashed one).  One iteration is one position of a cycle of s + 1: one product, one apply, one history entry.
    sequential: the published loop (a dot and an update of G_k, U_k for every i < k in turn) instead of the one multi-dot q
    with the forward substitution for alpha.  acc: the type the dots accumulate in.
    Returns dict(iters, conv, hist, x): hist[0] = ||b - A x0||, the stop test is hist[it] < tol hist[0] (converged) or a
    non-finite hist[it] (not converged)."""
    b = np.asarray(b, dtype=np.float64)
    n = len(b)
    P = hashed_shadow(n, s) if P is None else np.asarray(P, dtype=np.float64)
    Pa = P.astype(acc)
    M_inv = (lambda v: v) if apply is None else apply

    def dots(V, w):  # V^T w, accumulated in `acc`
        return np.asarray(np.dot(V.T.astype(acc), w.astype(acc)), dtype=np.float64)

    def norm(w):
        return float(np.sqrt(dots(w[:, None], w)[0]))

    x = np.array(x0, dtype=np.float64)
    r = b - matvec(x)
    hist = [norm(r)]
    stop = tol * hist[0]
    G, U, M = np.zeros((n, s)), np.zeros((n, s)), np.eye(s)
    omega = 1.0
    f = dots(Pa, r)
    conv = done = False

    def record():
        nonlocal conv, done
        hist.append(norm(r))
        conv = bool(hist[-1] < stop)
        done = conv or not np.isfinite(hist[-1])

    with np.errstate(all="ignore"):
        while not done and len(hist) - 1 < max_iters:
            for k in range(s):
                c = np.zeros(s)
                for i in range(k, s):  # forward substitution M[k.., k..] c = f[k..]
                    c[i] = (f[i] - np.dot(M[i, k:i], c[k:i])) / M[i, i]
                v = r - G[:, k:] @ c[k:]
                vh = M_inv(v)
                U[:, k] = omega * vh + U[:, k:] @ c[k:]
                G[:, k] = matvec(U[:, k])
                if sequential:
                    for i in range(k):
                        alpha = dots(Pa[:, i:i + 1], G[:, k])[0] / M[i, i]
                        G[:, k] -= alpha * G[:, i]
                        U[:, k] -= alpha * U[:, i]
                    M[k:, k] = dots(Pa[:, k:], G[:, k])
                else:
                    q = dots(Pa, G[:, k])
                    alpha = np.zeros(k)
                    for i in range(k):
                        alpha[i] = (q[i] - np.dot(M[i, :i], alpha[:i])) / M[i, i]
                    for i in range(k, s):
                        M[i, k] = q[i] - np.dot(M[i, :k], alpha)
                    G[:, k] -= G[:, :k] @ alpha
                    U[:, k] -= U[:, :k] @ alpha
                beta = f[k] / M[k, k]
                r = r - beta * G[:, k]
                x = x + beta * U[:, k]
                f[k + 1:] -= beta * M[k + 1:, k]
                record()
                if done or len(hist) - 1 >= max_iters:
                    break
            if done or len(hist) - 1 >= max_iters:
                break
            vh = M_inv(r)
            t = matvec(vh)
            tt, tr = dots(t[:, None], t)[0], dots(t[:, None], r)[0]
            omega = tr / tt
            rho = abs(tr) / (np.sqrt(tt) * hist[-1])
            if rho < 0.7:
                omega = omega * 0.7 / rho
            x = x + omega * vh
            r = r - omega * t
            record()
            f = dots(Pa, r)
    return dict(iters=len(hist) - 1, conv=conv, hist=np.array(hist), x=x)
