"""CPU: the numpy restatement of the thick-restart Lanczos eigensolver (tests/eigs_ref.py) against numpy.linalg.eigvalsh
on the inputs the GPU test uses, the margins that make "equal restart counts" a fair demand on the device, the licence of
the GPU history gate, and the Jacobi solve alone.  Each test prints what it measured before it asserts.

Measured here (the oracle's generators, which the device's reproduce bit for bit): the history moves by at most 1.7e-14 of
entry 0 between three orders of the sums (the issue's prototype: 4e-15 to 5e-14); 100 times that stays below the gate
HIST_TOL["cg"] = 1e-10.  The Jacobi solve alone: 8 sweeps at m = 64, ||Y^T Y - I||_max = 1.1e-15 (5 eps)."""
import numpy as np
import pytest

import eigs_ref as E
from helpers import HIST_TOL

TOL = 1e-10


class Cache:
    def __init__(self, orc):
        self.orc, self.mats, self.runs = orc, {}, {}

    def matrix(self, name):
        if name not in self.mats:
            A = E.make_input(name, self.orc)
            D = E.dense_of(A)
            self.mats[name] = (A, D, np.linalg.eigvalsh(D))
        return self.mats[name]

    def run(self, name, which, dots="np"):
        key = (name, which, dots)
        if key not in self.runs:
            A = self.matrix(name)[0]
            k, ncv = E.INPUTS[name][2:4]
            self.runs[key] = E.eigs(lambda v: E.host_spmv(A, v), A.n_rows, k, ncv, which, TOL, dots=E.DOTS[dots])
        return self.runs[key]


@pytest.fixture(scope="module")
def cache(oracle):
    return Cache(oracle)


@pytest.mark.parametrize("name", list(E.INPUTS))
def test_wanted_eigenvalues_are_simple(cache, name):
    """Single-vector Lanczos finds one vector per distinct eigenvalue: the inputs must have simple wanted eigenvalues."""
    A, D, lam = cache.matrix(name)
    assert np.array_equal(D, D.T)
    norm = np.max(np.abs(lam))
    k = E.INPUTS[name][2]
    for which in E.INPUTS[name][4]:
        w, rest = E.wanted(lam, k, which)
        chain = np.concatenate([w, rest[:1]])
        gap = min(abs(a - b) for i, a in enumerate(chain) for b in chain[i + 1:])
        print(f"{name} {which}: smallest gap among the wanted and to the next unwanted = {gap / norm:.3e} ||A||")
        assert gap > 1e-3 * norm


@pytest.mark.parametrize("name,which", E.ROWS)
def test_against_eigvalsh(cache, name, which):
    A, D, lam = cache.matrix(name)
    k = E.INPUTS[name][2]
    r = cache.run(name, which)
    dist, bound, _ = E.eigen_bound(D, r["values"], r["X"])
    w, _ = E.wanted(lam, k, which)
    print(f"{name} {which}: products {r['products']} restarts {r['restarts']} reason {E.REASONS[r['reason']]} "
          f"max |theta - lambda| {np.max(dist):.2e} (bound {np.max(bound):.2e}) max |theta - wanted| {np.max(np.abs(r['values'] - w)):.2e}")
    # ncv = n: the basis spans the whole space, the last step of the only cycle meets the invariant subspace
    assert r["converged"] and r["nconv"] == k
    assert r["reason"] == (E.INVARIANT if E.INPUTS[name][3] == A.n_rows else E.CONVERGED)
    assert np.all(dist <= bound)
    # the k wanted ones, none skipped: value i is nearer to wanted eigenvalue i than half the gap to any other eigenvalue
    for th, wi in zip(r["values"], w):
        others = lam[lam != wi]
        assert abs(th - wi) < 0.5 * np.min(np.abs(others - wi))


@pytest.mark.parametrize("name,which", E.ROWS)
def test_threshold_margins(cache, name, which):
    """At the last restart the deciding estimate is at most half its threshold, at the one before at least twice."""
    r = cache.run(name, which)
    ratios = r["ratios"]
    print(f"{name} {which}: est / threshold at the last two restarts: {[f'{x:.3g}' for x in ratios[-2:]]} of {len(ratios)}")
    assert ratios[-1] <= 0.5
    if len(ratios) > 1:
        assert ratios[-2] >= 2.0


def test_gate_licence(cache):
    """The largest move of the history between three orders of the sums, relative to entry 0 (eigs_ref.hist_scale: not
    less than 64 eps ||A||_1, which matters where ncv = n makes entry 0 itself rounding noise)."""
    worst = 0.0
    for name, which in E.ROWS:
        base = cache.run(name, which)
        for dots in ("long", "blocks"):
            r = cache.run(name, which, dots)
            assert r["restarts"] == base["restarts"] and r["products"] == base["products"], (name, which, dots)
            assert np.array_equal(r["hist_nconv"], base["hist_nconv"]), (name, which, dots)
            move = np.max(np.abs(r["hist"] - base["hist"])) / E.hist_scale(base["hist"], E.norm1_of(cache.matrix(name)[0]))
            worst = max(worst, move)
            print(f"{name} {which} {dots}: history moves by {move:.2e} of entry 0")
    print(f"largest move {worst:.2e}; gate {HIST_TOL['cg']:.0e}")
    assert 100 * worst <= HIST_TOL["cg"]


def jacobi_case(name):
    rng = np.random.default_rng(7)
    if name == "random64":
        B = rng.uniform(-1, 1, (64, 64))
        return (B + B.T) / 2
    if name == "arrow":
        l, m = 9, 24
        th, s = np.sort(rng.uniform(-3, 3, l)), 1e-3 * rng.uniform(-1, 1, l)
        return E.assemble_T(th, s, rng.uniform(-3, 3, m), rng.uniform(0.5, 1.5, m), l, m)
    if name == "repeated":
        Q, _ = np.linalg.qr(rng.uniform(-1, 1, (12, 12)))
        T = Q @ np.diag([1.0, 1.0, 1.0, 2.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0]) @ Q.T
        return (T + T.T) / 2
    return np.diag(np.arange(1.0, 6.0))


@pytest.mark.parametrize("name", ["random64", "arrow", "repeated", "diag"])
def test_jacobi_alone(name):
    T = jacobi_case(name)
    with np.errstate(all="ignore"):
        theta, Y, sweeps, ok = E.jacobi(T)
    fro = np.linalg.norm(T)
    res = np.max(np.abs(T @ Y - Y * theta[None, :]))
    orth = np.max(np.abs(Y.T @ Y - np.eye(len(T))))
    print(f"{name}: {sweeps} sweeps, ||T Y - Y theta||_max = {res:.2e} (64 eps ||T||_F = {64 * E.EPS * fro:.2e}), ||Y^T Y - I||_max = {orth:.2e}")
    assert ok
    assert res <= 64 * E.EPS * fro
    assert orth <= 64 * E.EPS
    assert np.allclose(np.sort(theta), np.linalg.eigvalsh(T), rtol=0, atol=64 * E.EPS * fro)
    if name == "diag":
        assert sweeps == 0
