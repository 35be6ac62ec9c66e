"""GPU: the multi-right-hand-side layer past its grid caps -- the lock-step solvers on a second trip of their 2048
workgroups, the persistent multi-vector sweep at its residency cap, the per-level sweep and the elementwise multi-vector
kernels past theirs.  Sizes and generators: tests/mrhs_cases.py (proved on the CPU by tests/test_mrhs_cases_cpu.py); every
test asserts that its case crosses the cap it is named for on the device it runs on.  References and gates are those of the
small-size tests of the same entry points (test_gpu_mcg.py, test_gpu_mbicgstab.py, test_gpu_mgmres.py, test_gpu_sptrsm.py,
test_gpu_mprecond.py, test_gpu_spmm.py); measured values: docs/EXPERIMENTS.md section 42."""
import numpy as np
import pytest

import mrhs_cases as mc
import test_gpu_mbicgstab as tbi
import test_gpu_mcg as tcg
import test_gpu_mgmres as tgm
from helpers import HIST_TOL, OptionScope, hist_dev
from oracle.pyoracle import Oracle
from test_gpu_sptrsm import expected_name, sweepm

pytestmark = pytest.mark.gpu

TOL = tcg.TOL
ZERO_START = (0, 1, 3, 6)  # the columns that start at x0 = 0 (columns() of test_gpu_mcg.py): r0 = b exactly


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


@pytest.fixture(scope="module")
def n_cus(ctx):
    return ctx.device_info()["n_cus"]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def norm_ld(v):
    v = np.asarray(v, dtype=np.longdouble)
    return float(np.sqrt(np.sum(v * v)))


# ---- a. the lock-step solvers past 2048 workgroups ----

@pytest.fixture(scope="module")
def band(ctx):
    """spd_band(180001, 3, 1) on the device with the operands of Jacobi and the eight columns -- built once, never changed;
    the single-vector and lock-step runs are cached in it by the tests that share them."""
    n = mc.N_LOCKSTEP
    A = mc.spd_band(n, 3, 1)
    diags = mc.spd_band_diagonals(n, 3, 1)
    dA = ctx.matrix(A)
    Ls, Us, D, Dinv = ctx.split_strict(dA)
    B, X0 = mc.rhs_columns(lambda v: mc.band_matvec(n, diags, v, dtype=np.float64), n, 8, seed=108)
    assert not X0[:, ZERO_START].any()
    return dict(n=n, A=A, diags=diags, dA=dA, dD=ctx.mat_diag(dA)[0], Ls=Ls, Us=Us, D=D, Dinv=Dinv, B=B, X0=X0,
                bnorm=[norm_ld(B[:, j]) for j in range(8)], single={}, mbi={}, mgm={}, cache={})


def true_residual(band, b, x):
    """|| b - A x || with longdouble products and sums"""
    return norm_ld(np.asarray(b, dtype=np.longdouble) - mc.band_matvec(band["n"], band["diags"], x))


def check_r0(tag, band, r0, k):
    """the r0 that init returns for the columns that start at 0 against || b || in longdouble, at the project's dot / norm gate
    1e-13: the reduction sums about 5 + act / k + 128 + 16 terms in sequence at most, an error near 3e-14"""
    for j in (j for j in ZERO_START if j < k):
        err = abs(r0[j] - band["bnorm"][j]) / band["bnorm"][j]
        print(f"{tag} j={j}: r0 {r0[j]:.17e}, || b || in longdouble {band['bnorm'][j]:.17e}, relative error {err:.3e}")
        assert err <= 1e-13, (tag, j, err)


def assert_strides(band, k):
    assert mc.lockstep_strides(band["n"], k), f"n k = {band['n'] * k} fits {mc.LOCKSTEP_MAX_BLOCKS} workgroups of {mc.lockstep_act(k)} lanes"


def cg_refs(ctx, band, jacobi):
    key = ("cg", jacobi)
    if key not in band["cache"]:
        dD = band["dD"] if jacobi else None
        band["cache"][key] = [tcg.run_cg(ctx, band["dA"], dD, band["B"][:, j].copy(), band["X0"][:, j].copy()) for j in range(8)]
    return band["cache"][key]


def mcg_run(ctx, band, jacobi, k):
    key = ("mcg", jacobi, k)
    if key not in band["cache"]:
        band["cache"][key] = tcg.run_mcg(ctx, band["dA"], band["dD"] if jacobi else None, band["B"][:, :k].copy(),
                                         band["X0"][:, :k].copy(), extra=50)
    return band["cache"][key]


@pytest.mark.parametrize("k", [3, 7, 8])
@pytest.mark.parametrize("jacobi", [False, True])
def test_mcg_past_the_reduce_cap(ctx, band, jacobi, k):
    """Crosses kMaxReduceBlocks = 2048 (lockstep_grid): n k > 2048 act, act = 255 / 252 / 256 for k = 3 / 7 / 8, so every
    elementwise pass of bis_mcg_* takes a second trip with the stride gridDim.x act and sum_partials folds 2048 partials."""
    assert_strides(band, k)
    tag = f"mcg {'jacobi' if jacobi else 'none'} k={k}"
    cg = cg_refs(ctx, band, jacobi)
    run = mcg_run(ctx, band, jacobi, k)
    counts = [c["iters"] for c in cg[:k]]
    print(f"{tag}: cg iteration counts {counts}, mcg {run['iters']}")
    assert max(counts) <= 100 and len(set(counts)) >= 2, counts  # short runs, and a column freezes while others run
    for j in range(k):
        dev = hist_dev(run["hist"][j], cg[j]["hist"])
        res = true_residual(band, band["B"][:, j], run["X"][:, j])
        print(f"{tag} j={j}: mcg iters {run['iters'][j]} conv {run['conv'][j]}, cg iters {cg[j]['iters']} conv {cg[j]['conv']}, "
              f"hist dev {dev:.3e}, true residual {res:.6e}, last history entry {run['hist'][j][-1]:.6e}, r0 {run['hist'][j][0]:.6e}")
        assert dev <= HIST_TOL["cg"], (tag, j)
        assert abs(run["iters"][j] - cg[j]["iters"]) <= 2 and run["conv"][j] == cg[j]["conv"], (tag, j)
        assert res <= run["hist"][j][-1] + 1e-10 * run["hist"][j][0], (tag, j)
    assert all(run["conv"]) and len(set(run["iters"])) >= 2
    check_r0(tag, band, run["r0"], k)
    # two runs give the same bits; 50 iterations after every column has stopped move nothing
    again = tcg.run_mcg(ctx, band["dA"], band["dD"] if jacobi else None, band["B"][:, :k].copy(), band["X0"][:, :k].copy())
    assert again["iters"] == run["iters"] and same_bits(again["X"], run["X"]) and same_bits(again["r0"], run["r0"])
    after = run["after"]
    assert after["iters"] == run["iters"] and after["conv"] == run["conv"] and same_bits(after["X"], run["X"])
    for j in range(k):
        assert same_bits(again["hist"][j], run["hist"][j]) and same_bits(after["hist"][j], run["hist"][j]), (tag, j)


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("jacobi", [False, True])
def test_mcg_columns_never_mix_past_the_reduce_cap(ctx, band, jacobi, k):
    """Crosses kMaxReduceBlocks = 2048 with act = 255 (k = 3) and 252 (k = 7), not multiples of 256: a stride that is not a
    multiple of k would hand a lane another column on its second trip.  One column of B changed: no other column moves a bit."""
    assert_strides(band, k)
    assert mc.lockstep_act(k) % k == 0 and mc.lockstep_act(k) != 256
    base = mcg_run(ctx, band, jacobi, k)
    B = band["B"][:, :k].copy()
    B[:, 1] = np.random.default_rng(9).uniform(-3, 3, band["n"])
    run = tcg.run_mcg(ctx, band["dA"], band["dD"] if jacobi else None, B, band["X0"][:, :k].copy())
    assert not same_bits(run["hist"][1][:2], base["hist"][1][:2])
    for j in (j for j in range(k) if j != 1):
        assert run["iters"][j] == base["iters"][j] and run["conv"][j] == base["conv"][j], j
        assert same_bits(run["hist"][j], base["hist"][j]) and same_bits(run["X"][:, j], base["X"][:, j]), j


def single_bi(ctx, band, pc):
    if pc not in band["single"]:
        band["single"][pc] = [tbi.run_single(ctx, band, pc, 0, band["B"][:, j].copy(), band["X0"][:, j].copy()) for j in range(8)]
    return band["single"][pc]


@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("pc", ["none", "j"])
def test_mbicgstab_past_the_reduce_cap(ctx, band, pc, k):
    """Crosses kMaxReduceBlocks = 2048 (lockstep_grid) in the mbi_* passes of bis_mbicgstab_*: act = 255 (k = 3), 256 (k = 8).
    Reference and gates of test_gpu_mbicgstab.py."""
    assert_strides(band, k)
    tag = f"mbicgstab {pc} k={k}"
    ref = single_bi(ctx, band, pc)
    B, X0 = band["B"][:, :k].copy(), band["X0"][:, :k].copy()
    done, after = tbi.run_mbi(ctx, band, pc, 0, B, X0, steps=(tbi.ITERS, 50))
    print(f"{tag}: single iteration counts {[c['iters'] for c in ref[:k]]}, mbicgstab {done['iters']}")
    for j in range(k):
        tbi.check_column(f"{tag} j={j}", band["A"], B[:, j], done["iters"][j], done["conv"][j], done["hist"][j], done["X"][:, j], ref[j])
    assert all(done["conv"])
    check_r0(tag, band, done["r0"], k)
    again = tbi.run_mbi(ctx, band, pc, 0, B, X0)[0]
    assert again["iters"] == done["iters"] and same_bits(again["X"], done["X"])
    assert after["iters"] == done["iters"] and after["conv"] == done["conv"] and same_bits(after["X"], done["X"])
    for j in range(k):
        assert same_bits(again["hist"][j], done["hist"][j]) and same_bits(after["hist"][j], done["hist"][j]), (tag, j)
    if k == 3:  # act = 255: one column of B changed, no other column moves a bit
        B2 = B.copy()
        B2[:, 1] = np.random.default_rng(9).uniform(-3, 3, band["n"])
        run = tbi.run_mbi(ctx, band, pc, 0, B2, X0)[0]
        assert not same_bits(run["hist"][1][:2], done["hist"][1][:2])
        for j in (0, 2):
            assert run["iters"][j] == done["iters"][j] and same_bits(run["hist"][j], done["hist"][j]), (tag, j)
            assert same_bits(run["X"][:, j], done["X"][:, j]), (tag, j)


def single_gm(ctx, band, pc):
    key = ("gm", pc)
    if key not in band["single"]:
        band["single"][key] = [tgm.run_single(ctx, band, pc, 0, band["B"][:, j].copy(), band["X0"][:, j].copy(), tgm.M) for j in range(8)]
    return band["single"][key]


@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("pc", ["none", "j"])
def test_mgmres_past_the_reduce_cap(ctx, band, pc, k):
    """Crosses kMaxReduceBlocks = 2048 (lockstep_grid) in the mgm_* passes of bis_mgmres_*, restart 10 (a basis of 11 n k
    doubles: 127 MB at k = 8): act = 255 (k = 3), 256 (k = 8).  Reference and gates of test_gpu_mgmres.py."""
    assert_strides(band, k)
    assert tgm.M == 10
    tag = f"mgmres {pc} k={k}"
    ref = single_gm(ctx, band, pc)
    B, X0 = band["B"][:, :k].copy(), band["X0"][:, :k].copy()
    done, after = tgm.run_mgm(ctx, band, pc, 0, B, X0, steps=(tgm.ITERS, 50))
    print(f"{tag}: single iteration counts {[c['iters'] for c in ref[:k]]}, mgmres {done['iters']}")
    for j in range(k):
        tgm.check_column(ctx, f"{tag} j={j}", band, pc, 0, j, done["iters"][j], done["conv"][j], done["hist"][j], done["X"][:, j], ref[j])
    assert all(done["conv"])
    check_r0(tag, band, done["r0"], k)
    again = tgm.run_mgm(ctx, band, pc, 0, B, X0)[0]
    assert again["iters"] == done["iters"] and same_bits(again["X"], done["X"])
    assert after["iters"] == done["iters"] and after["conv"] == done["conv"] and same_bits(after["X"], done["X"])
    for j in range(k):
        assert same_bits(again["hist"][j], done["hist"][j]) and same_bits(after["hist"][j], done["hist"][j]), (tag, j)
    if k == 3:  # act = 255: one column of B changed, no other column moves a bit
        B2 = B.copy()
        B2[:, 1] = np.random.default_rng(9).uniform(-3, 3, band["n"])
        run = tgm.run_mgm(ctx, band, pc, 0, B2, X0)[0]
        assert not same_bits(run["hist"][1][:2], done["hist"][1][:2])
        for j in (0, 2):
            assert run["iters"][j] == done["iters"][j] and same_bits(run["hist"][j], done["hist"][j]), (tag, j)
            assert same_bits(run["X"][:, j], done["X"][:, j]), (tag, j)


# ---- b. the persistent multi-vector sweep at its residency cap ----

def rhs_block(n, k, seed):
    """n x k: column 0 ones, column 1 uniform, the rest uniform at the scales 1e-6, 1, 1e6 (rhs_block of test_gpu_sptrsm.py)"""
    rng = np.random.default_rng(seed)
    B = rng.uniform(-1, 1, (n, k))
    B[:, 0] = 1.0
    for j in range(2, k):
        B[:, j] *= (1e-6, 1.0, 1e6)[(j - 2) % 3]
    return B


def triangle_case(ctx, orc, widths, fan, seed, rp64=True):
    """A layered triangle and its mirror on the device in both row-pointer widths, eight right-hand sides and the oracle's
    serial sweep on each, forward and backward -- the reference every k shares."""
    L, D = mc.layered_lower(widths, fan, seed)
    U = mc.mirror(L)
    n = L.n_rows
    dev = {32: (ctx.matrix(L), ctx.matrix(U))}
    if rp64:
        with OptionScope(ctx, force_rp64=1):
            dev[64] = (ctx.matrix(L), ctx.matrix(U))
    for rp, (dL, dU) in dev.items():
        assert dL.rp_width == rp // 8 and dU.rp_width == rp // 8
    B = rhs_block(n, 8, seed=seed + 1)
    ref = {bw: [orc.sptrsv(T, D, B[:, j].copy(), backward=bw) for j in range(8)] for bw, T in ((False, L), (True, U))}
    for bw in ref:
        assert all(np.all(np.isfinite(x)) for x in ref[bw])
    return dict(L=L, U=U, D=D, n=n, widths=list(widths), dev=dev, dD=ctx.upload(D), B=B, ref=ref)


@pytest.fixture(scope="module")
def wave_cases(ctx, orc):
    return dict(large=triangle_case(ctx, orc, mc.WAVE_WIDTHS, 4, seed=31), small=triangle_case(ctx, orc, mc.WAVE_WIDTHS_SMALL, 4, seed=41))


def check_sweeps(ctx, e, ks, levels, nan_fill=False, widths=(32, 64)):
    for rp in widths:
        for backward in (False, True):
            dT = e["dev"][rp][1 if backward else 0]
            for k in ks:
                B = np.ascontiguousarray(e["B"][:, :k])
                tag = (rp, "backward" if backward else "forward", k)
                if nan_fill:
                    dB, dX = ctx.upload(B.ravel()), ctx.upload(np.full(e["n"] * k, np.nan))
                    (ctx.bsptrsm if backward else ctx.sptrsm)(dT, dX, e["dD"], dB, k)
                    ctx.sync()
                    X = dX.to_host().reshape(e["n"], k)
                    dB.free(); dX.free()
                else:
                    X = sweepm(ctx, dT, e["dD"], B, backward)
                kernel = dT.sweepm_kernel(backward)
                Xa = sweepm(ctx, dT, e["dD"], B, backward, alias=True)
                for j in range(k):
                    assert same_bits(X[:, j], e["ref"][backward][j]), tag + (j, kernel, int(np.sum(X[:, j] != e["ref"][backward][j])))
                assert same_bits(Xa, X), tag + ("X aliasing B",)
                assert kernel == expected_name(-1, levels, k, backward, rp=rp), tag + (kernel,)


def test_wave_sweep_at_the_residency_cap(ctx, n_cus, wave_cases):
    """Crosses launch_wave's cap n_cus wave_resident / device_share (bis_sptrsm.hip): 70 levels of 1100 rows, widest level + 1 =
    1101 > 4 n_cus and n = 77,000 > 16 n_cus, so the persistent grid is the cap itself and every wave deals itself a second
    and later position (pos += n_waves) across level boundaries."""
    e = wave_cases["large"]
    grid, cap = mc.wave_grid(e["n"], max(e["widths"]), n_cus)
    print(f"n_cus {n_cus}: persistent grid {grid} workgroups = the cap {cap}, {-(-e['n'] // (4 * grid))} positions per wave")
    assert max(e["widths"]) + 1 > cap and e["n"] > 4 * cap and grid == cap
    assert len(e["widths"]) > mc.FEW_LEVELS
    check_sweeps(ctx, e, (2, 3, 5, 8), len(e["widths"]))


@pytest.mark.parametrize("name", ["small", "large"])
def test_wave_sweep_on_an_eighth_of_the_device(ctx, n_cus, wave_cases, name):
    """Crosses launch_wave's cap under device_share = 8: n_cus 4 / 8 workgroups (128 on 256 CUs) for levels of 300 and 1100
    rows -- a wave walks about 40 (small) and 150 (large) positions, a level spans several rounds of the grid."""
    e = wave_cases[name]
    grid, cap = mc.wave_grid(e["n"], max(e["widths"]), n_cus, share=mc.WAVE_SHARE)
    positions = -(-e["n"] // (4 * grid))
    print(f"n_cus {n_cus}, device_share {mc.WAVE_SHARE}: persistent grid {grid} = the cap {cap}, {positions} positions per wave")
    assert grid == cap and max(e["widths"]) + 1 > cap and positions >= 20
    with OptionScope(ctx, device_share=mc.WAVE_SHARE):
        check_sweeps(ctx, e, (2, 3, 5, 8), len(e["widths"]))


# ---- c. the per-level multi-vector sweep past its grid cap ----

def test_level_sweep_past_its_grid_cap(ctx, orc, n_cus):
    """Crosses launch_level's cap n_cus 32 workgroups (bis_sptrsm.hip): level 0 holds n_cus 32 256 / 8 + 5,000 rows, so at
    k = 8 its (row, column) pairs exceed the capped grid's lanes and trsm_level_kernel strides; at k = 3 it does not.  The
    2,000 rows of level 1 read rows of the strided part; X is NaN before the call."""
    w0 = mc.level_w0(n_cus)
    one_trip = n_cus * mc.LEVEL_BLOCKS_PER_CU * 256 // 8
    e = triangle_case(ctx, orc, [w0, 2000], 3, seed=51, rp64=False)
    grid8, cap = mc.level_grid(w0, 8, n_cus)
    grid3, _ = mc.level_grid(w0, 3, n_cus)
    print(f"n_cus {n_cus}: level 0 of {w0} rows, grid {grid8} = the cap {cap} at k = 8 ({w0 * 8} pairs on {cap * 256} lanes), grid {grid3} at k = 3")
    assert grid8 == cap and w0 * 8 > cap * 256 and grid3 < cap
    assert mc.level_widths(e["L"]) == [w0, 2000]
    assert int(e["L"].col.max()) >= one_trip, "no row of level 1 reads the strided part of level 0"
    # (the mirror's level 0 is its rows 2000 .. n - 1, in that order in the level-sorted plan)
    assert int(e["U"].col.max()) >= 2000 + one_trip, "no row of the mirror's level 1 reads the strided part of its level 0"
    check_sweeps(ctx, e, (8, 3), 2, nan_fill=True, widths=(32,))
    for dT in e["dev"][32]:
        dT.free()
    e["dD"].free()


# ---- d. the elementwise multi-vector kernels past their caps ----

@pytest.mark.parametrize("k", [8, 3])
def test_diag_kernels_past_their_grid_cap(ctx, k):
    """Crosses kMpMaxBlocks = 16,384 workgroups (mvec_diag_kernel, bis_mprecond.hip): n = 524,301, k = 8 is more than 16,384 x 256
    elements, so the kernel strides and d[e / k] is read on the second trip; k = 3 for the e / k map with k no power of two."""
    n = mc.N_DIAG
    assert (n * k > mc.MVEC_DIAG_MAX_BLOCKS * 256) == (k == 8)
    rng = np.random.default_rng(k)
    V = rng.uniform(-1, 1, (n, k)) * 10.0 ** rng.integers(-6, 7, (1, k))
    D = rng.uniform(1, 2, n) * 10.0 ** rng.integers(-3, 4, n)
    dD, A, R = ctx.upload(D), ctx.upload(V.ravel()), ctx.upload(np.full(n * k, np.nan))
    ctx.mvec_div_diag(R, A, dD, n, k)
    assert same_bits(R.to_host().reshape(n, k), V / (1.0 * D[:, None]))
    ctx.mvec_mul_diag(R, A, dD, n, k)
    assert same_bits(R.to_host().reshape(n, k), V * 1.0 * D[:, None])
    assert same_bits(A.to_host().reshape(n, k), V)
    ctx.mvec_mul_diag(A, A, dD, n, k)  # in place
    assert same_bits(A.to_host().reshape(n, k), V * 1.0 * D[:, None])
    A.set(V.ravel())
    ctx.mvec_div_diag(A, A, dD, n, k)
    assert same_bits(A.to_host().reshape(n, k), V / (1.0 * D[:, None]))
    for v in (dD, A, R):
        v.free()


def test_column_copies_past_their_grid_cap(ctx):
    """Crosses copy_grid's 8,192 workgroups (mvec_set_col_kernel / mvec_get_col_kernel, bis_spmm.hip): n = 2^21 + 5 > 8,192 x 256
    rows, k = 3.  The round trip of test_mvec_columns_round_trip: every other column's bits untouched."""
    n, k = mc.N_COPY, 3
    assert n > mc.MVEC_COPY_MAX_BLOCKS * 256
    rng = np.random.default_rng(n + k)
    base = rng.uniform(-1, 1, (n, k))
    dX = ctx.upload(base.ravel())
    dv, dw = ctx.alloc(n), ctx.upload(np.full(n, np.nan))
    want = base.copy()
    for j in range(k):
        v = rng.uniform(-1, 1, n)
        v[0] = -0.0
        v[-1] = -0.0
        dv.set(v)
        ctx.mvec_set_col(dX, n, k, j, dv)
        want[:, j] = v
        assert same_bits(dX.to_host().reshape(n, k), want), j
        ctx.mvec_get_col(dw, dX, n, k, j)
        assert same_bits(dw.to_host(), v), j
    dX.free(); dv.free(); dw.free()


def test_mitrsv_past_the_diag_cap(ctx):
    """Crosses kMpMaxBlocks = 16,384 in the MP_MUL start and the MP_ITRSV epilogue of bis_mitrsv (n = 524,301, k = 8), with
    bis_spmm on 2,560+ row blocks between them: against bis_itrsv per column and against the recurrence x_0 = b D_inv,
    x_{s+1} = (b - T x_s) D_inv built on spmm_band_ref, each operation rounded -- both bit for bit."""
    n, k = mc.N_DIAG, 8
    assert n * k > mc.MVEC_DIAG_MAX_BLOCKS * 256
    diags, T, D_inv = mc.band_lower_full(n, 4, seed=6)
    dT, dDinv = ctx.matrix(T), ctx.upload(D_inv)
    rng = np.random.default_rng(7)
    V = rng.uniform(-1, 1, (n, k))
    for j in range(1, k):
        V[:, j] *= (1.0, 1e-6, 1e6)[j % 3]
    B, X, W = ctx.upload(V.ravel()), ctx.alloc(n * k), ctx.alloc(n * k)
    b, x, w = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
    for sweeps in (0, 3):
        ctx.init_vector(X, np.nan)
        ctx.mitrsv(dT, dDinv, B, X, W, sweeps, k)
        got = X.to_host().reshape(n, k)
        want = mc.mitrsv_ref(diags, D_inv, V, sweeps)
        assert same_bits(got, want), (sweeps, dT.spmm_kernel(), int(np.sum(got != want)))
        for j in range(k):
            b.set(V[:, j].copy())
            ctx.itrsv(dT, dDinv, b, x, w, sweeps)
            assert same_bits(got[:, j], x.to_host()), (sweeps, j, dT.spmm_kernel(), dT.itrsv_kernel())
    assert same_bits(B.to_host().reshape(n, k), V)
    for v in (B, X, W, b, x, w, dDinv):
        v.free()
    dT.free()
