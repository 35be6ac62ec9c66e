"""GPU: the device ILU(0) (bis_ilu0.hip: two row sorts, three eliminations) on adversarial patterns, against the
reference's factor_ILU0_old.

The fixture (tests/golden/golden_ilu_edges.npz, made by the reference: make_golden.py --ilu-edges-only) holds missing,
zero, -0.0 and near-tolerance diagonals, empty rows, entries that cancel to 0, unsorted and unsymmetric rows, rows of
63 to 1025 entries and repeated columns.  Every case runs under the default configuration, under every ILU(0) kernel /
launch / grid setting and with 32- and 64-bit row pointers; the library names the kernel that ran (Mat.ilu0_kernel()),
so that a setting cannot pass by falling back quietly.  A seeded random differential at 20-50 k rows against the oracle
(the reference's arithmetic restated, equal to it bit for bit on the fixture: test_oracle_golden.py) follows."""
import numpy as np
import pytest

from helpers import OptionScope, has_repeated_column, load_ilu_edges, relerr
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

KTOL = 1e-13
KILU_MAX_ROW = 1024  # bis_ilu0.hip kIluMaxRow: longer rows take the lane-per-row kernel

_CASES = load_ilu_edges()

# the settings of test_gpu_option_paths._ILU_CONFIGS
_ILU_CONFIGS = [dict(ilu0_wave=w, ilu0_persistent=p, ilu0_wgs=g) for w in (0, -1) for p in (0, -1) for g in (1, 2, 4)
                if not (p == 0 and g != 4)]  # (ilu0_wgs sizes the persistent grid only: once with the per-level launches)


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    base = c.options()
    yield c
    assert c.options() == base
    c.close()


def _expected_kernel(A, cfg):
    """Repeated columns and rows past kIluMaxRow take the lane-per-row kernel whatever the options say."""
    if has_repeated_column(A) or np.diff(A.row_ptr).max(initial=0) > KILU_MAX_ROW or cfg.get("ilu0_wave", -1) == 0:
        return "ilu0_level_kernel"
    return "ilu0_level_wave_kernel" if cfg.get("ilu0_persistent", -1) == 0 else "ilu0_persistent_kernel"


def _factor(ctx, A, **kw):
    """(Ls, L_D, Us, U_D, kernel, device handles) of ctx.ilu0 on A."""
    dA = ctx.matrix(A)
    dLs, dL_D, dUs, dU_D = ctx.ilu0(dA, **kw)
    dA.free()
    n = A.n_rows
    Ls, Us = CRS(n, *dLs.download()), CRS(n, *dUs.download())
    return Ls, dL_D.to_host(), Us, dU_D.to_host(), dLs.ilu0_kernel(), (dLs, dL_D, dUs, dU_D)


def _free(dev):
    for h in dev:
        h.free()


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def _assert_factors(got, want, exact, tag):
    """Patterns, L_D and U_D exactly; values bit for bit where every operation is exact, else within 1e-13 per factor."""
    (Ls, L_D, Us, U_D), (wLs, wL_D, wUs, wU_D) = got, want
    for k, (a, b) in enumerate(((Ls, wLs), (Us, wUs))):
        assert np.array_equal(a.row_ptr, b.row_ptr) and np.array_equal(a.col, b.col), (tag, "LU"[k], "pattern")
        if exact:
            assert np.array_equal(_bits(a.val), _bits(b.val)), (tag, "LU"[k])
        else:
            assert relerr(a.val, b.val) <= KTOL, (tag, "LU"[k])
    assert np.array_equal(_bits(L_D), _bits(wL_D)), (tag, "L_D")
    assert np.array_equal(_bits(U_D), _bits(wU_D)), (tag, "U_D")


def _check_apply(ctx, oracle, dev, Ls, L_D, Us, U_D, y, want=None, sweep_tol=0.0):
    """The ILU(0) apply on the device's factors against the golden apply (1e-12), and both device sweeps against the
    oracle's on the device's own factors: bit for bit (sweep_tol = 0), or within sweep_tol where the small fixture
    patterns reach a sweep form whose summation order is not the serial one (unsorted_reverse, unsorted_shuffled and
    dup_long_row differ in the last bits: a sweep finding, out of this file's ILU(0) scope)."""
    dLs, dL_D, dUs, dU_D = dev
    n = len(y)
    ones = ctx.upload(np.ones(n))
    inp, out, tmp, work = ctx.upload(y), ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
    if want is not None:
        ctx.apply_preconditioner("ilu0", n, dLs, dUs, ones, ones, dL_D, dU_D, out, inp, tmp, work)
        assert relerr(out.to_host(), want) <= 1e-12
        assert np.array_equal(inp.to_host(), y)
    t, x = ctx.alloc(n), ctx.alloc(n)
    ctx.sptrsv(dLs, t, dL_D, inp)
    ctx.bsptrsv(dUs, x, dU_D, t)
    to = oracle.sptrsv(Ls, L_D, y)
    xo = oracle.sptrsv(Us, U_D, to, backward=True)
    if sweep_tol == 0.0:
        assert np.array_equal(_bits(t.to_host()), _bits(to)), "forward sweep"
        assert np.array_equal(_bits(x.to_host()), _bits(xo)), "backward sweep"
    else:
        assert relerr(t.to_host(), to) <= sweep_tol, "forward sweep"
        assert relerr(x.to_host(), xo) <= sweep_tol, "backward sweep"
    for v in (ones, inp, out, tmp, work, t, x):
        v.free()


@pytest.mark.parametrize("rp64", [-1, 1])
@pytest.mark.parametrize("name", sorted(_CASES))
def test_ilu0_edge_case_vs_reference(ctx, oracle, name, rp64):
    """Each case under the default configuration and every ILU(0) setting: factors equal the reference's, every setting
    gives the same bits, the kernel that ran is the one the input and the setting call for, and the apply and both
    sweeps on the device's factors match."""
    c = _CASES[name]
    A = c["A"]
    want = (c["Ls"], c["L_D"], c["Us"], c["U_D"])
    base = None
    for cfg in [{}] + _ILU_CONFIGS:
        with OptionScope(ctx, force_rp64=rp64, **cfg):
            Ls, L_D, Us, U_D, kernel, dev = _factor(ctx, A)
            try:
                assert kernel == _expected_kernel(A, cfg), (name, cfg, kernel)
                got = (Ls, L_D, Us, U_D)
                _assert_factors(got, want, c["exact"], (name, cfg, kernel))
                if base is None:
                    base = got
                    _check_apply(ctx, oracle, dev, Ls, L_D, Us, U_D, c["y"], c["pc_ilu0"], sweep_tol=KTOL)
                else:
                    _assert_factors(got, base, True, (name, cfg, kernel, "vs default"))
            finally:
                _free(dev)


# pivot arguments the reference cannot take (its tolerance is a compile-time constant): pivot_tol = 0 keeps a zero or
# missing diagonal at 0, pivot_repl = 0 / 1e-20 replaces it by a value below 1e-16 -- either way the |u_kk| < 1e-16 skip
_PIVOT_ARGS = [dict(pivot_tol=0.0), dict(pivot_repl=0.0), dict(pivot_repl=1e-20)]
_PIVOT_CASES = ["no_diag", "zero_diag", "negzero_diag", "tiny_diag", "empty_rows", "rand_unsorted_dups", "rand_unsymmetric",
                "rand_long_rows"]


@pytest.mark.parametrize("args", _PIVOT_ARGS, ids=lambda a: ",".join(f"{k}={v}" for k, v in a.items()))
@pytest.mark.parametrize("name", _PIVOT_CASES)
def test_ilu0_pivot_arguments_vs_oracle(ctx, oracle, name, args):
    """Non-default pivot arguments on every kernel: the same factors as oracle.factor_ilu0 with the same arguments."""
    c = _CASES[name]
    A = c["A"]
    oLs, oL_D, oUs, oU_D = oracle.factor_ilu0(A, **{**dict(pivot_tol=1e-8, pivot_repl=1e-4), **args})
    assert np.any(np.abs(oU_D[oLs.col]) < 1e-16), "some row eliminates against a pivot below 1e-16"
    for cfg in [{}, dict(ilu0_wave=0), dict(ilu0_persistent=0)]:
        with OptionScope(ctx, **cfg):
            Ls, L_D, Us, U_D, kernel, dev = _factor(ctx, A, **args)
            _free(dev)
        assert kernel == _expected_kernel(A, cfg), (name, cfg, kernel)
        _assert_factors((Ls, L_D, Us, U_D), (oLs, oL_D, oUs, oU_D), c["exact"], (name, args, cfg, kernel))


def _random_ilu_matrix(rng, n, seed):
    """Unsymmetric, unsorted: a band plus far entries, some repeated columns (in some seeds), explicit zeros, a few tiny
    or missing diagonals, a few rows longer than 64."""
    band = [8, 40, 300, 3][seed % 4]
    lens = rng.integers(1, [6, 4, 3, 8][seed % 4], n)
    rows = np.repeat(np.arange(n), lens)
    col = np.clip(rows + rng.integers(-band, band + 1, rows.size), 0, n - 1)
    far = rng.random(rows.size) < 0.05
    col[far] = rng.integers(0, n, int(far.sum()))
    # every row gets its diagonal, then a few lose it
    rows = np.concatenate([rows, np.arange(n)])
    col = np.concatenate([col, np.arange(n)])
    long_rows = rng.choice(n, 6, replace=False)
    for r in long_rows:
        extra = rng.choice(n, 70 + int(rng.integers(0, 60)), replace=False)
        rows, col = np.concatenate([rows, np.full(extra.size, r)]), np.concatenate([col, extra])
    val = np.round(rng.uniform(-1, 1, rows.size) * 1024) / 1024
    diag = rows == col
    val[diag] = 8.0 + val[diag]
    tiny = diag & (rng.random(rows.size) < 0.01)
    val[tiny] = rng.choice([0.0, -0.0, 1e-9, -1e-9, 1e-17], int(tiny.sum()))
    val[~diag & (rng.random(rows.size) < 0.03)] = 0.0
    keep = ~(diag & (rng.random(rows.size) < 0.005))
    rows, col, val = rows[keep], col[keep], val[keep]
    if seed % 2 == 0:  # repeated columns: the lane-per-row kernel whatever the options say
        dup = rng.choice(rows.size, n // 200, replace=False)
        rows, col = np.concatenate([rows, rows[dup]]), np.concatenate([col, col[dup]])
        val = np.concatenate([val, np.round(rng.uniform(-1, 1, dup.size) * 1024) / 1024])
    else:  # no repeated column: the wave kernels run
        _, first = np.unique(rows.astype(np.int64) * n + col, return_index=True)
        rows, col, val = rows[first], col[first], val[first]
    order = np.lexsort((rng.random(rows.size), rows))  # grouped by row, shuffled inside each row
    rows, col, val = rows[order], col[order], val[order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return CRS(n, rp, col.astype(np.int32), val)


@pytest.mark.parametrize("seed", range(6))
def test_ilu0_random_patterns_vs_oracle(ctx, oracle, seed):
    """Seeded random patterns of 20-50 k rows against oracle.factor_ilu0 under the default and two other settings: the
    same factor assertions, the path named, and the sweeps on the device's factors bit for bit."""
    rng = np.random.default_rng(7100 + seed)
    n = [20000, 33000, 50000, 27000, 41000, 24000][seed]
    A = _random_ilu_matrix(rng, n, seed)
    assert has_repeated_column(A) == (seed % 2 == 0)
    want = oracle.factor_ilu0(A)
    want = (want[0], want[1], want[2], want[3])
    y = np.round(rng.uniform(-1, 1, n) * 1024) / 1024
    for t, cfg in enumerate([{}, dict(ilu0_wave=0, force_rp64=1), dict(ilu0_persistent=0, ilu0_wgs=2)]):
        with OptionScope(ctx, **cfg):
            Ls, L_D, Us, U_D, kernel, dev = _factor(ctx, A)
            try:
                assert kernel == _expected_kernel(A, cfg), (seed, cfg, kernel)
                _assert_factors((Ls, L_D, Us, U_D), want, False, (seed, cfg, kernel))
                if t == 0:
                    _check_apply(ctx, oracle, dev, Ls, L_D, Us, U_D, y)
            finally:
                _free(dev)
