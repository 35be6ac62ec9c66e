"""The numpy restatement of block Jacobi as include/bis_hip.h defines it (extraction, Gauss-Jordan with partial pivoting,
symmetrisation, the block-diagonal product), and numpy restatements of the iterations the GPU test solves with it.  Every
array operation below rounds each elementwise product, quotient, difference and sum on its own, as the header asks, so the
blocks and the apply are comparable bit for bit.  Blocks of one size are inverted and applied together (one array of shape
(blocks, m, 2 m)): the order of the operations inside a block is the header's."""
import numpy as np


def host_spmv(A, x):
    rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
    return np.bincount(rows, weights=A.val * x[A.col], minlength=A.n_rows)


def block_ptr_of(n, block_size=None, block_ptr=None):
    if block_ptr is not None:
        return np.asarray(block_ptr, dtype=np.int64)
    return np.minimum(np.arange(0, n + block_size, block_size, dtype=np.int64), n)[:(n + block_size - 1) // block_size + 1]


def extract(A, bptr):
    """The dense diagonal blocks: zeros, then every entry of the block's rows whose column lies in the block added in
    storage order (np.add.at adds one entry after the other)."""
    bptr = np.asarray(bptr, dtype=np.int64)
    sizes = np.diff(bptr)
    offs = np.concatenate([[0], np.cumsum(sizes * sizes)])
    flat = np.zeros(offs[-1])
    blk_of_row = np.repeat(np.arange(len(sizes)), sizes)
    rows = np.repeat(np.arange(A.n_rows), np.diff(A.row_ptr))
    b = blk_of_row[rows]
    col = np.asarray(A.col, dtype=np.int64)
    inside = (col >= bptr[b]) & (col < bptr[b + 1])
    r, c, b = rows[inside], col[inside], b[inside]
    np.add.at(flat, offs[b] + (r - bptr[b]) * sizes[b] + (c - bptr[b]), np.asarray(A.val)[inside])
    return [flat[offs[i]:offs[i + 1]].reshape(sizes[i], sizes[i]) for i in range(len(sizes))]


def invert_batch(B):
    """B: (nb, m, m).  Returns (R, singular): the inverses and, per block, whether some pivot was 0 or not finite (the
    block's R is then meaningless)."""
    nb, m, _ = B.shape
    T = np.concatenate([B.astype(np.float64), np.broadcast_to(np.eye(m), (nb, m, m))], axis=2).copy()
    idx = np.arange(nb)
    bad = np.zeros(nb, dtype=bool)
    with np.errstate(all="ignore"):
        for k in range(m):
            mag = np.abs(T[:, k:, k])
            p = np.full(nb, k)
            for i in range(k + 1, m):  # the first row with the largest |a_ik|: only a strictly larger one replaces it
                p = np.where(mag[:, i - k] > np.abs(T[idx, p, k]), i, p)
            rk, rp = T[idx, k].copy(), T[idx, p].copy()
            T[idx, k], T[idx, p] = rp, rk
            piv = T[:, k, k]
            bad |= (piv == 0.0) | ~np.isfinite(piv)
            r = 1.0 / piv
            rowk = T[:, k, :] * r[:, None]
            f = T[:, :, k].copy()
            T = T - f[:, :, None] * rowk[:, None, :]
            T[:, k, :] = rowk
    return T[:, :, m:].copy(), bad


def invert(B):
    """One block: its inverse, or None where a pivot is 0 or not finite."""
    R, bad = invert_batch(np.asarray(B, dtype=np.float64)[None])
    return None if bad[0] else R[0]


def symmetrized(R):
    return (R + np.swapaxes(R, -1, -2)) * 0.5


class BlockJacobi:
    """The restated handle: .blocks (list of inverse blocks, block order), .singular (indices of the blocks with a bad pivot),
    .apply(x) for x of shape (n,) or (n, k)."""

    def __init__(self, A, block_size=None, block_ptr=None, symmetrize=False):
        self.n = A.n_rows
        self.bptr = block_ptr_of(self.n, block_size, block_ptr)
        sizes = np.diff(self.bptr)
        dense = extract(A, self.bptr)
        self.blocks = [None] * len(sizes)
        self.singular = []
        self.groups = []  # (m, block indices, row index array (nb, m), R (nb, m, m))
        for m in np.unique(sizes):
            which = np.nonzero(sizes == m)[0]
            R, bad = invert_batch(np.stack([dense[b] for b in which]))
            if symmetrize:
                R = symmetrized(R)
            self.singular += [int(b) for b in which[bad]]
            for q, b in enumerate(which):
                self.blocks[b] = R[q]
            self.groups.append((int(m), which, self.bptr[which][:, None] + np.arange(m)[None, :], R))
        self.singular.sort()

    def flat(self):
        """(values, offsets) as bis_bj_blocks gives them: block b row-major at offsets[b]."""
        sizes = np.diff(self.bptr)
        offs = np.concatenate([[0], np.cumsum(sizes * sizes)]).astype(np.int64)
        vals = np.concatenate([b.ravel() for b in self.blocks]) if self.blocks else np.zeros(0)
        return vals, offs

    def apply(self, x):
        x = np.asarray(x, dtype=np.float64)
        out = np.empty_like(x)
        for m, _, rows, R in self.groups:
            xb = x[rows]  # (nb, m) or (nb, m, k)
            if x.ndim == 1:
                acc = R[:, :, 0] * xb[:, 0:1]
                for j in range(1, m):
                    acc = acc + R[:, :, j] * xb[:, j:j + 1]
            else:
                acc = R[:, :, 0, None] * xb[:, None, 0, :]
                for j in range(1, m):
                    acc = acc + R[:, :, j, None] * xb[:, None, j, :]
            out[rows] = acc
        return out


# ---- the iterations -------------------------------------------------------------------------------------------------------

def np_pcg(A, apply, b, tol, max_iters, x0=None):
    """bis_cg_* with a general preconditioner: history of ||r||, stop at ||r|| < tol ||r0||."""
    x = np.zeros_like(b) if x0 is None else x0.copy()
    r = b - host_spmv(A, x)
    z = apply(r)
    p = z.copy()
    rz = r @ z
    hist = [np.linalg.norm(r)]
    while len(hist) - 1 < max_iters and not hist[-1] < tol * hist[0]:
        Ap = host_spmv(A, p)
        alpha = rz / (p @ Ap)
        x = x + alpha * p
        r = r - alpha * Ap
        z = apply(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
        hist.append(np.linalg.norm(r))
    return dict(iters=len(hist) - 1, conv=bool(hist[-1] < tol * hist[0]), hist=np.array(hist), x=x)


def np_minres(A, apply, b, tol, max_iters):
    """bis_minres_* line by line (include/bis_hip.h), from x0 = 0; the history is phibar."""
    n = A.n_rows
    f = np.float64
    with np.errstate(all="ignore"):
        x = np.zeros(n)
        r1 = b - host_spmv(A, x)
        y = apply(r1)
        beta1 = np.sqrt(f(r1 @ y))
        r2 = r1.copy()
        w, w2 = np.zeros(n), np.zeros(n)
        oldb, beta, dbar, epsln, phibar, cs, sn = f(0), beta1, f(0), f(0), beta1, f(-1), f(0)
        hist, conv, k = [beta1], False, 0
        while k < max_iters:
            k += 1
            v = y * (1.0 / beta)
            y = host_spmv(A, v)
            if k >= 2:
                y = y - (beta / oldb) * r1
            alpha = f(v @ y)
            y = y - (alpha / beta) * r2
            r1, r2 = r2, y
            y = apply(r2)
            oldb, beta = beta, np.sqrt(f(r2 @ y))
            oldeps, delta, gbar = epsln, cs * dbar + sn * alpha, sn * dbar - cs * alpha
            epsln, dbar = sn * beta, -cs * beta
            gamma = np.sqrt(gbar * gbar + beta * beta)
            cs, sn = gbar / gamma, beta / gamma
            phi, phibar = cs * phibar, sn * phibar
            w1, w2 = w2, w
            w = (v - oldeps * w1 - delta * w2) * (1.0 / gamma)
            x = x + phi * w
            hist.append(phibar)
            if phibar < tol * beta1:
                conv = True
                break
            if not np.isfinite(phibar):
                break
    return dict(iters=k, conv=conv, hist=np.array(hist), x=x)


def np_bicgstab(A, apply, b, x0, tol, max_iters):
    """One column of bis_mbicgstab_*: the left-preconditioned iteration whose shadow residual and p_0 are M^-1 r_0."""
    f = np.float64
    x = x0.copy()
    r = b - host_spmv(A, x)
    hist = [np.linalg.norm(r)]
    stop = tol * hist[0]
    p = apply(r)
    r0 = p.copy()
    rho = f(r @ p)
    conv = False
    with np.errstate(all="ignore"):
        for _ in range(max_iters):
            y = apply(p)
            v = host_spmv(A, y)
            alpha = rho / f(r0 @ v)
            s = r - alpha * v
            st = apply(s)
            z = host_spmv(A, st)
            omega = f(z @ s) / f(z @ z)
            x = (x + alpha * y) + omega * st
            rn = s - omega * z
            rho_new = f(r0 @ rn)
            beta = (rho_new / rho) * (alpha / omega)
            p = rn + beta * (p - omega * v)
            r, rho = rn, rho_new
            norm = np.linalg.norm(r)
            hist.append(norm)
            conv = bool(abs(norm) < stop)
            if conv or not np.isfinite(norm):
                break
    return dict(iters=len(hist) - 1, conv=conv, hist=np.array(hist), x=x)


class Givens:
    """The least-squares problem of one GMRES cycle: stored rotations on the new Hessenberg column, c = a / den, s = b / den,
    den = sqrt(a^2 + b^2); g follows; y by back substitution."""

    def __init__(self, m, beta):
        self.m = m
        self.R = np.zeros((m + 1, m))
        self.cs, self.sn = np.zeros(m), np.zeros(m)
        self.g = np.zeros(m + 1)
        self.g[0] = beta

    def step(self, n, hcol):
        h = np.array(hcol, dtype=np.float64)
        for i in range(n):
            a, b = h[i], h[i + 1]
            h[i] = self.cs[i] * a + self.sn[i] * b
            h[i + 1] = self.cs[i] * b - self.sn[i] * a
        a, b = h[n], h[n + 1]
        den = np.sqrt(a * a + b * b)
        c, s = a / den, b / den
        self.cs[n], self.sn[n] = c, s
        self.R[:n, n] = h[:n]
        self.R[n, n] = c * a + s * b
        self.g[n + 1] = -s * self.g[n]
        self.g[n] = c * self.g[n]
        return abs(self.g[n + 1])

    def y(self, steps):
        y = np.zeros(self.m)
        for r in range(steps - 1, -1, -1):
            y[r] = (self.g[r] - np.dot(self.R[r, r + 1:steps], y[r + 1:steps])) / self.R[r, r]
        return y


def np_gmres(A, apply, b, x0, m, tol, max_iters, right):
    """Restarted GMRES(m).  right = False: one column of bis_mgmres_* (left-preconditioned; entry 0 the unpreconditioned
    ||r0||, the other entries the estimate of ||M^-1 r||, a restart writes beta as one more entry).  right = True:
    bis_fgmres_* (the basis Z_n = M^-1 V_n kept, every entry the true residual norm or its estimate)."""
    n = A.n_rows
    x = x0.copy()

    def start_cycle():
        r = b - host_spmv(A, x)
        unpre = np.linalg.norm(r)
        if not right:
            r = apply(r)
        beta = np.linalg.norm(r)
        return unpre, beta, r * (1.0 / beta)

    with np.errstate(all="ignore"):
        r0, beta, v0 = start_cycle()
        hist = [r0]
        stop = tol * r0
        V, Z = np.zeros((m + 1, n)), np.zeros((m, n))
        V[0] = v0
        G = Givens(m, beta)
        iters, conv, pos = 0, False, 0
        while iters < max_iters:
            if right:
                Z[pos] = apply(V[pos])
                w = host_spmv(A, Z[pos])
            else:
                w = apply(host_spmv(A, V[pos]))
            hcol = []
            for i in range(pos + 1):
                hcol.append(np.float64(w @ V[i]))
                w = w - hcol[-1] * V[i]
            hcol.append(np.linalg.norm(w))
            V[pos + 1] = w * (1.0 / hcol[-1])
            est = G.step(pos, hcol)
            iters += 1
            pos += 1
            hist.append(est)
            conv = bool(est < stop)
            if conv or not np.isfinite(est):
                break
            if pos == m:
                x = x + G.y(pos)[:pos] @ (Z if right else V)[:pos]
                _, beta, v0 = start_cycle()
                hist.append(beta)
                V[0] = v0
                G = Givens(m, beta)
                pos = 0
                conv = bool(beta < stop)
                if conv or not np.isfinite(beta):
                    break
        if pos > 0:
            x = x + G.y(pos)[:pos] @ (Z if right else V)[:pos]
    return dict(iters=iters, conv=conv, hist=np.array(hist), x=x)
