"""GPU: the kernel paths that only the tuning options reach (bis_set_option / BIS_* variables), each against a reference
and against the default configuration, and each with the kernel that ran named by the library (spmv_kernel(),
sweep_kernel(), spmv_stream_info()) -- so that no test passes because the library fell back quietly.

Options are set through helpers.OptionScope (reset to -1 afterwards, ctx.options() back at its baseline).  Options that
pick workgroups per CU are only ever set BELOW their defaults: the persistent grids must be resident as a whole."""
import re

import numpy as np
import pytest

from helpers import (GOLDEN_MATS, OptionScope, SPMV_CATALOGUE, check_history, check_rows, crs_of, load_golden,
                     load_histories, load_histories_mid, parse_hist_key, permute_crs, relerr, spmv_catalogue_case,
                     spmv_catalogue_x, window_fits)

pytestmark = pytest.mark.gpu

KTOL = 1e-13


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    base = c.options()
    yield c
    assert c.options() == base
    c.close()


# ---- A. row-block SpMV ------------------------------------------------------------------------------------------------

# A covering design: every spmv_variant, spmv_packed 0/1/2, spmv_packed32, every spmv_xcd_remap form (0 blockIdx order,
# 1 XCD slabs, G = 2, 3, 16 groups), every spmv_chunk, spmv_lds_pad and spmv_window appear on every catalogue matrix.
# Variant 20 is the default variant of the packed stream, under which the dictionary / window + sliced-ELL forms take
# precedence: its configuration switches those off so that the row-block kernel itself runs.
SPMV_CONFIGS = [
    dict(spmv_variant=10, spmv_packed=0, spmv_xcd_remap=0, spmv_chunk=256),
    dict(spmv_variant=11, spmv_packed=1, spmv_xcd_remap=1, spmv_chunk=300),
    dict(spmv_variant=12, spmv_packed=2, spmv_xcd_remap=2, spmv_chunk=1024),
    dict(spmv_variant=20, spmv_packed=0, spmv_xcd_remap=3, spmv_chunk=4096, spmv_valdict=0, spmv_win8=0),
    dict(spmv_variant=21, spmv_packed=1, spmv_xcd_remap=16, spmv_chunk=256, spmv_packed32=1),
    dict(spmv_variant=22, spmv_packed=2, spmv_xcd_remap=0, spmv_chunk=300, spmv_lds_pad=16384),
    dict(spmv_variant=40, spmv_packed=1, spmv_xcd_remap=2, spmv_chunk=1024, spmv_packed32=1),
    dict(spmv_variant=41, spmv_packed=0, spmv_xcd_remap=3, spmv_chunk=4096),
    dict(spmv_variant=41, spmv_packed=2, spmv_xcd_remap=16, spmv_chunk=1024, spmv_lds_pad=16384, spmv_packed32=1),
    dict(spmv_window=1, spmv_chunk=1024, spmv_xcd_remap=1),
    dict(spmv_window=1, spmv_chunk=256, spmv_xcd_remap=0, spmv_variant=10),
    dict(spmv_window=1, spmv_chunk=4096, spmv_xcd_remap=3),
]
_NAME = re.compile(r"spmv_rowblock_kernel U=(\d) PK=(\d)( WIDE)? BR=(\d)$")


def _check_kernel(name, A, cfg, info):
    """The kernel the configuration targets ran -- or the library refused it for a reason the test can state."""
    lens = np.diff(A.row_ptr)
    chunk = max(256, cfg.get("spmv_chunk", 256))
    if int(lens.max(initial=0)) + chunk + 8 > 8192:  # a row past the LDS budget: the wave-per-row kernel for every form
        assert name == "spmv_wave_per_row_kernel", (name, cfg)
        return
    if cfg.get("spmv_window") == 1 and window_fits(A, chunk):
        assert name == "spmv_window_kernel", (name, cfg)
        return
    # (spmv_window = 1 on a matrix whose blocks touch more than 128 tiles, or past the LDS budget: the structure is
    # dropped and the row-block kernel runs)
    m = _NAME.match(name)
    assert m, (name, cfg)
    U, PK, BR = int(m.group(1)), int(m.group(2)), int(m.group(4))
    col_bytes = info[0]
    assert (PK != 0) == (col_bytes == 2), (name, info)
    packed = cfg.get("spmv_packed", 1)
    if packed == 0:
        assert PK == 0, name
    elif PK:
        assert PK == (3 if PK == 3 else packed), (name, cfg)
        assert PK != 3 or cfg.get("spmv_packed32") == 1, (name, cfg)
    v = cfg.get("spmv_variant", 20 if PK else 41)
    if PK >= 2 and v % 10 != 0:  # the lane-permute / 32-window decodes need the whole wave: the branch-free form only
        assert (U, BR) == (2, 0), (name, cfg)
    else:
        assert (U, BR) == (v // 10, v % 10), (name, cfg)


@pytest.mark.parametrize("name", SPMV_CATALOGUE + ["scatter32"])
def test_spmv_option_paths_bit_identical(ctx, oracle, name):
    """Every row-block configuration of SPMV_CONFIGS on a catalogue matrix (tests/helpers.py): y bit-identical to the
    default configuration's y -- phase 2 is one lane per row summing the parked products left to right in CRS order
    (bis_spmv_rowblock.hip "phase 2"), so staging, chunking, remapping and packing cannot change a bit -- and every row within its
    own bound of the exact sum (helpers.check_rows).  y is poisoned with NaN before every call; x holds Inf / NaN at
    columns no row references.  Each configuration runs on a freshly created matrix and on a matrix created under the
    default options and rebuilt with retune(): the same bits.  spmv_kernel() must name the instance targeted."""
    if name == "scatter32":
        # 12 column windows 16384 apart per row block: more than the 8 windows of 8192 the default packed form has,
        # within the 32 windows of 2048 of the opt-in 32-window form (PK 3)
        from oracle.pyoracle import CRS
        n, n_cols = 6000, 200000
        rows = [sorted({(r // 4) % 1500 + k * 16384 for k in range(12)}) for r in range(n)]
        rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])])
        A = CRS(n, rp, np.array([c for cs in rows for c in cs], dtype=np.int32),
                np.random.default_rng(7).uniform(-1, 1, int(rp[-1])), n_cols=n_cols)
        rp64 = 0
    else:
        A, rp64 = spmv_catalogue_case(name, oracle)
    x = spmv_catalogue_x(A, seed=3, scale=0.5 if name == "extreme_values" else 1.0)
    dx, dy = ctx.upload(x), ctx.alloc(A.n_rows)

    def run(dA):
        ctx.init_vector(dy, np.nan)
        ctx.spmv(dA, dx, dy)
        return dy.to_host()

    with OptionScope(ctx, force_rp64=rp64):
        dA0 = ctx.matrix(A)
        assert dA0.spmv_kernel() == ""
        y0 = run(dA0)
        default_kernel = dA0.spmv_kernel()
        assert default_kernel
        check_rows(y0, A, x, f"{name} default ({default_kernel})")
        dR = ctx.matrix(A)  # created under the default options, retuned under each configuration
        run(dR)
        pk3 = False
        for cfg in SPMV_CONFIGS:
            with OptionScope(ctx, **cfg):
                dA = ctx.matrix(A)
                assert dA.rp_width == (8 if rp64 else 4)
                y = run(dA)
                k = dA.spmv_kernel()
                assert np.array_equal(y, y0, equal_nan=True), (name, cfg, k, default_kernel)
                _check_kernel(k, A, cfg, dA.spmv_stream_info())
                pk3 |= "PK=3" in k
                dR.retune()
                yr = run(dR)
                assert np.array_equal(yr, y0, equal_nan=True), (name, cfg, "retune", dR.spmv_kernel())
                assert dR.spmv_kernel() == k, (name, cfg)
                dA.free()
        if name == "scatter32":
            assert pk3, "the 32-window packed form never ran"
        dR.retune()  # back under the default options: the default kernel again
        assert np.array_equal(run(dR), y0, equal_nan=True) and dR.spmv_kernel() == default_kernel
        dA0.free(); dR.free()
    dx.free(); dy.free()


# ---- B. fused CG --------------------------------------------------------------------------------------------------------

_H = load_histories()
_CG_KEYS = sorted(k for k in _H if k.split("|")[1] == "cg" and k.split("|")[2] in ("none", "j") and "num_scale" not in k)
_HM = load_histories_mid()
_MID_KEY = "hpcg48|cg|none|"


def _cg_run(ctx, key, opts):
    """(hist, iters, converged, x, fused kernel name) of the fused CG on a golden / mid-size key under the options."""
    with OptionScope(ctx, **opts):
        if key == _MID_KEY:
            dA, D = ctx.gen_hpcg(48), None
            n = dA.n_rows
        else:
            name, _, pc, _ = parse_hist_key(key)
            g = load_golden(name)
            dA = ctx.matrix(crs_of(g, "A"))
            n = dA.n_rows
            D = ctx.upload(g["A_D"]) if pc == "j" else None
        b, x = ctx.upload(np.full(n, 1.0)), ctx.upload(np.full(n, 0.1))
        cg = ctx.cg(dA, b, x, D)
        cg.init(1e-14)
        cg.iterate(1000)
        iters, conv, hist = cg.status()
        kernel = dA.spmv_kernel(fused=True)
        out = (np.asarray(hist), iters, conv, x.to_host(), kernel)
        cg.free(); dA.free(); b.free(); x.free()
        if D is not None:
            D.free()
    return out


_CG_CHUNK_CONFIGS = [dict(spmv_chunk_fused=c, spmv_variant=v) for c in (256, 777, 4096) for v in (10, 21, 40)] + \
                    [dict(spmv_window=1, spmv_chunk=1024)]


@pytest.mark.parametrize("key", _CG_KEYS + [_MID_KEY])
def test_fused_cg_chunk_and_variant_options(ctx, key):
    """spmv_chunk_fused in {256, 777, 4096} x spmv_variant in {10, 21, 40}, and spmv_window = 1, in the fused CG: histories
    held to check_history; the same chunk under another variant gives bit-identical histories and x (the per-wave dot
    partials depend on the block table only); spmv_kernel(fused=True) names the targeted kernel."""
    e = (_HM if key == _MID_KEY else _H)[key]
    runs = {}
    for cfg in _CG_CHUNK_CONFIGS:
        hist, iters, conv, x, kernel = _cg_run(ctx, key, cfg)
        check_history(dict(hist=hist, iters=iters, converged=conv), e, "cg", long_history=key == _MID_KEY)
        if cfg.get("spmv_window"):
            assert kernel == "spmv_window_kernel", kernel
        else:
            m = _NAME.match(kernel)
            assert m, kernel
            v = cfg["spmv_variant"]
            PK = int(m.group(2))
            assert (int(m.group(1)), int(m.group(4))) == ((2, 0) if PK >= 2 and v % 10 else (v // 10, v % 10)), (kernel, cfg)
            runs.setdefault(cfg["spmv_chunk_fused"], []).append((hist, x, cfg))
    for chunk, rs in runs.items():
        for hist, x, cfg in rs[1:]:
            assert np.array_equal(hist, rs[0][0]) and np.array_equal(x, rs[0][1]), (key, chunk, cfg)


@pytest.mark.parametrize("key", _CG_KEYS[:3] + [_MID_KEY])
def test_fused_cg_cache_hints_are_bit_identical(ctx, key):
    """cg_nt_x in {0, 2, 3} (x through the caches / the non-temporal p-update forms) and spmv_sellwin_nt = 0 (the sliced-ELL
    code stream through the caches) are cache hints only: histories and x bit-identical to the default configuration."""
    h0, it0, c0, x0, k0 = _cg_run(ctx, key, {})
    assert k0
    for cfg in (dict(cg_nt_x=0), dict(cg_nt_x=2), dict(cg_nt_x=3), dict(spmv_sellwin_nt=0)):
        h, it, c, x, k = _cg_run(ctx, key, cfg)
        assert k == k0, (cfg, k, k0)
        assert it == it0 and c == c0 and np.array_equal(h, h0) and np.array_equal(x, x0), (key, cfg)


# ---- C. level-scheduled and sync-free sweeps ------------------------------------------------------------------------------

_SWEEP_CONFIGS = [  # on top of trsv_tiled = 0, trsv_chain = 0; (options, kernel targeted)
    (dict(trsv_host_analysis=1), None),
    (dict(trsv_wave=0, trsv_batch=4), "sptrsv_syncfree_kernel"),
    (dict(trsv_wave=0, trsv_batch=8, trsv_by_pos=0), "sptrsv_syncfree_kernel"),
    (dict(trsv_wave=0, trsv_batch=16, trsv_one_xcd=1), "sptrsv_syncfree_kernel"),
    (dict(trsv_wave=0, trsv_batch=32, trsv_one_xcd=2), "sptrsv_syncfree_kernel"),
    (dict(trsv_wave=1, trsv_wave_wgs=1), "sptrsv_wave_kernel"),
    (dict(trsv_wave=1, trsv_wave_wgs=2, trsv_by_pos=0), "sptrsv_wave_kernel"),
    (dict(trsv_wave=1, trsv_wave_wgs=4, trsv_host_analysis=1), "sptrsv_wave_kernel"),
    (dict(trsv_wave=1, trsv_one_xcd=1), "sptrsv_syncfree_kernel"),  # (one_xcd: the lane-per-row grid on one XCD)
]
_LEVEL_NAMES = ("spmv_rowblock_kernel (triangular epilogue", "trsv_level_kernel")


def _sweep_inputs(ctx, oracle, kind):
    if kind in ("hpcg", "anderson"):
        A = oracle.gen_hpcg(20) if kind == "hpcg" else oracle.gen_anderson(20, shift=9.0)
        return A, ctx.matrix(A)
    A = oracle.gen_unstr(12, 12, 13)
    dA = ctx.gen_unstr(12, 12, 13)
    if kind == "unstr_rcm":
        perm = ctx.bfs_order(dA, rcm=True)
        dB = ctx.permute(dA, perm)
        dA.free()
        return permute_crs(A, perm), dB
    if kind == "unstr_colour":
        dB, perm, _ = ctx.multicolour(dA)
        dA.free()
        return permute_crs(A, perm), dB
    return A, dA


@pytest.mark.parametrize("kind", ["unstr", "unstr_rcm", "unstr_colour", "hpcg", "anderson"])
def test_level_and_syncfree_sweep_options(ctx, oracle, kind):
    """The level paths (trsv_tiled = 0, trsv_chain = 0) under trsv_host_analysis, trsv_batch 4..32, trsv_by_pos = 0,
    trsv_one_xcd 1, 2, trsv_wave 0 / 1 and trsv_wave_wgs 1, 2, 4: forward and backward bit-identical to the same sweep
    under the default level options (except the per-level launches under trsv_host_analysis, see below), and against the oracle as the existing sweep tests hold them -- bit-exact for the
    sync-free / wave-per-row kernels (the reference's fma chain), the kernel tolerance for the per-level launches of
    few-level / multi-colour triangles (products, then sums).  sweep_kernel() names the kernel targeted."""
    A, dA = _sweep_inputs(ctx, oracle, kind)
    n = A.n_rows
    L, Ls, U, Us = oracle.split_LU(A)
    D, _, _ = oracle.peel_diag(L)
    b = np.random.default_rng(5).uniform(-1, 1, n)
    fw, bw = oracle.sptrsv(Ls, D, b), oracle.sptrsv(Us, D, b, backward=True)
    db, x = ctx.upload(b), ctx.alloc(n)

    def sweeps(opts):
        with OptionScope(ctx, trsv_tiled=0, trsv_chain=0, **opts):
            dLs, dUs, dD, dDinv = ctx.split_strict(dA)
            ctx.init_vector(x, np.nan)
            ctx.sptrsv(dLs, x, dD, db)
            f = x.to_host()
            ctx.init_vector(x, np.nan)
            ctx.bsptrsv(dUs, x, dD, db)
            out = (f, x.to_host(), dLs.sweep_kernel(False), dUs.sweep_kernel(True))
            dLs.free(); dUs.free(); dD.free(); dDinv.free()
        return out

    f0, b0, kf0, kb0 = sweeps({})
    for got, want, k in ((f0, fw, kf0), (b0, bw, kb0)):
        if k.startswith(_LEVEL_NAMES):
            assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (kind, k)
        else:
            assert np.array_equal(got, want), (kind, k)
    for opts, want_kernel in _SWEEP_CONFIGS:
        f, bk, kf, kb = sweeps(opts)
        for got, base, want, k, k0 in ((f, f0, fw, kf, kf0), (bk, b0, bw, kb, kb0)):
            if k0.startswith(_LEVEL_NAMES) and "trsv_host_analysis" in opts:
                # (the host analysis has no block search: the backward levels of the multi-colour input are not ascending
                # row ranges there, and the sweep takes the launch-per-level kernel instead of the row-block views --
                # other arithmetic, held to the oracle at the kernel tolerance)
                assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (kind, opts, k)
            else:
                assert np.array_equal(got, base), (kind, opts, k, k0)
        for k, k0 in ((kf, kf0), (kb, kb0)):
            if k0.startswith(_LEVEL_NAMES) and "trsv_host_analysis" in opts:
                assert k.startswith(_LEVEL_NAMES), (kind, opts, k)
            elif k0.startswith(_LEVEL_NAMES) or want_kernel is None:
                assert k == k0, (kind, opts, k, k0)  # (the per-level launches do not read the sync-free options)
            else:
                assert k == want_kernel, (kind, opts, k)
    dA.free(); db.free(); x.free()


# ---- D. chained and tiled sweeps ----------------------------------------------------------------------------------------

_CHAIN_OPTS = [dict(trsv_chain_prefix=1), dict(trsv_chain_idle=0, trsv_chain_pause=0), dict(trsv_chain_idle=4, trsv_chain_pause=1),
               dict(trsv_chain_prefix=1, trsv_chain_idle=4, trsv_chain_pause=0)]


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_chained_sweep_polling_options_bit_exact(ctx, oracle, seed):
    """The inputs of test_chained_sweep_randomised_bit_exact under trsv_chain_prefix = 1 (the feeder sums part of a row's
    fma chain itself), trsv_chain_idle 0 / 4 and trsv_chain_pause 0 / 1: forward and backward bit-exact against the fma
    oracle, and the sweep that ran is the chained one."""
    from oracle.pyoracle import CRS
    from test_gpu_unstr import _random_chain_triangle
    rng = np.random.default_rng(100 + seed)
    n = 12000 + 777 * seed
    rp, col = _random_chain_triangle(rng, n, band=[50, 3000, 400, n][seed % 4], p_link=[0.95, 0.8, 0.99, 0.6][seed % 4],
                                     max_extra=[3, 40, 12, 6][seed % 4], sort_cols=seed % 3 != 1, long_rows=seed % 2 == 0)
    val = rng.uniform(-1, 1, rp[-1]) / 8.0
    D = rng.uniform(1.0, 2.0, n)
    b = rng.uniform(-1, 1, n)
    L = CRS(n, rp, col, val)
    lens = np.diff(rp)[::-1]
    rpu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in range(n - 1, -1, -1)]) if rp[-1] else np.zeros(0, np.int64)
    U = CRS(n, rpu, (n - 1 - col[idx]).astype(np.int32), val[idx])
    fw = oracle.sptrsv(L, D, b)
    bw = oracle.sptrsv(U, D[::-1].copy(), b, backward=True)
    dD, dDr, db, x = ctx.upload(D), ctx.upload(D[::-1].copy()), ctx.upload(b), ctx.alloc(n)
    for opts in _CHAIN_OPTS:
        with OptionScope(ctx, trsv_chain=1, force_rp64=1 if seed % 4 == 3 else -1, **opts):
            dL, dU = ctx.matrix(L), ctx.matrix(U)
            ctx.init_vector(x, np.nan)
            ctx.sptrsv(dL, x, dD, db)
            assert np.array_equal(x.to_host(), fw), (seed, opts)
            ctx.init_vector(x, np.nan)
            ctx.bsptrsv(dU, x, dDr, db)
            assert np.array_equal(x.to_host(), bw), (seed, opts)
            assert dL.sweep_kernel(False) == "trsv_chain_kernel" and dU.sweep_kernel(True) == "trsv_chain_kernel", opts
            dL.free(); dU.free()
    for v in (dD, dDr, db, x):
        v.free()


_TILE_OPTS = [dict(trsv_tile_wgs=1), dict(trsv_tile_wgs=2, trsv_tile_backoff=0), dict(trsv_tile_backoff=64),
              dict(trsv_tile_wgs=1, trsv_tile_backoff=64)]


@pytest.mark.parametrize("shape,dof", [((13, 11, 9), 1), ((9, 8, 7), 3), ((20, 20, 20), 1)])
def test_tiled_sweep_grid_and_backoff_options_bit_exact(ctx, oracle, shape, dof):
    """The tiled sweep (grid-hinted stencils of test_tiled_sweep_random_stencils' kind: every lower neighbour within
    distance 1) under trsv_tile_wgs 1 / 2 and trsv_tile_backoff 0 / 64: forward and backward bit-exact against the fma
    oracle, and the sweep that ran is the tiled one."""
    from oracle.pyoracle import CRS
    rng = np.random.default_rng(sum(shape) + dof)
    nx, ny, nz = shape
    cand = [(ddx, ddy, ddz, dd) for ddz in (-1, 0, 1) for ddy in (-1, 0, 1) for ddx in (-1, 0, 1) for dd in range(-(dof - 1), dof)
            if (ddz, ddy, ddx, dd) < (0, 0, 0, 0)]
    n = nx * ny * nz * dof
    rows = [[] for _ in range(n)]
    for z in range(nz):
        for y in range(ny):
            for xx in range(nx):
                for d in range(dof):
                    r = ((z * ny + y) * nx + xx) * dof + d
                    for ddx, ddy, ddz, dd in cand:
                        X, Y, Z, Dd = xx + ddx, y + ddy, z + ddz, d + dd
                        if 0 <= X < nx and 0 <= Y < ny and 0 <= Z < nz and 0 <= Dd < dof:
                            rows[r].append(((Z * ny + Y) * nx + X) * dof + Dd)
    for r in range(n):
        rows[r].sort()
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])])
    col = np.array([c for cs in rows for c in cs], dtype=np.int32)
    L = CRS(n, rp, col, rng.uniform(-0.3, 0.3, len(col)))
    Ut = L.to_scipy().T.tocsr()
    Ut.sort_indices()
    U = CRS(n, Ut.indptr, Ut.indices.astype(np.int32), Ut.data)
    D, b = rng.uniform(1, 2, n), rng.uniform(-1, 1, n)
    fw, bw = oracle.sptrsv(L, D, b), oracle.sptrsv(U, D, b, backward=True)
    dD, db, x = ctx.upload(D), ctx.upload(b), ctx.alloc(n)
    for opts in _TILE_OPTS:
        with OptionScope(ctx, trsv_tiled=1, trsv_chain=0, **opts):
            dL, dU = ctx.matrix(L), ctx.matrix(U)
            dL.set_grid_hint(nx, ny, nz, dof); dU.set_grid_hint(nx, ny, nz, dof)
            ctx.init_vector(x, np.nan)
            ctx.sptrsv(dL, x, dD, db)
            assert np.array_equal(x.to_host(), fw), (shape, dof, opts)
            ctx.init_vector(x, np.nan)
            ctx.bsptrsv(dU, x, dD, db)
            assert np.array_equal(x.to_host(), bw), (shape, dof, opts)
            assert dL.sweep_kernel(False) == "trsv_tiled_kernel" and dU.sweep_kernel(True) == "trsv_tiled_kernel", opts
            dL.free(); dU.free()
    dD.free(); db.free(); x.free()


# ---- E. ILU(0) ----------------------------------------------------------------------------------------------------------

_ILU_CONFIGS = [dict(ilu0_wave=w, ilu0_persistent=p, ilu0_wgs=g) for w in (0, -1) for p in (0, -1) for g in (1, 2, 4)
                if not (p == 0 and g != 4)]  # (ilu0_wgs sizes the persistent grid only: once with the per-level launches)


def _ilu(ctx, dA):
    dLs, L_D, dUs, U_D = ctx.ilu0(dA)
    out = dLs.download() + dUs.download() + (L_D.to_host(), U_D.to_host())
    dLs.free(); dUs.free(); L_D.free(); U_D.free()
    return out


def _assert_factors_identical(got, base, cfg):
    for a, b in zip(got, base):
        assert np.array_equal(a, b), cfg


@pytest.mark.parametrize("name", GOLDEN_MATS + ["unstr_mid"])
def test_ilu0_option_paths(ctx, oracle, name):
    """ILU(0) under ilu0_wave 0 / -1 (lane per row / wave per row), ilu0_persistent 0 / -1 (a launch per level / one
    persistent launch) and ilu0_wgs 1, 2, 4: the patterns match the reference's factors (golden) or oracle.factor_ilu0
    (mid-size unstructured input) exactly, the values within the kernel tolerance; and all settings give bit-identical
    factors -- every form eliminates a row with the same operation sequence (the row's entries in CRS order, one update per
    earlier pivot row, bis_ilu0.hip), only the scheduling of rows differs, so the values are compared bit for bit."""
    if name == "unstr_mid":
        A = oracle.gen_unstr(10, 10, 11)
        Ls, L_D, Us, U_D = oracle.factor_ilu0(A)
        want = (Ls.row_ptr, Ls.col, Ls.val, Us.row_ptr, Us.col, Us.val, L_D, U_D)
        make = lambda: ctx.gen_unstr(10, 10, 11)  # noqa: E731
    else:
        g = load_golden(name)
        want = (g["iluLs_rp"], g["iluLs_col"], g["iluLs_val"], g["iluUs_rp"], g["iluUs_col"], g["iluUs_val"], g["iluLD"], g["iluUD"])
        make = lambda: ctx.matrix(crs_of(g, "A"))  # noqa: E731
    base = None
    for cfg in [{}] + _ILU_CONFIGS:
        with OptionScope(ctx, **cfg):
            dA = make()
            got = _ilu(ctx, dA)
            dA.free()
        for k in (0, 1, 3, 4):
            assert np.array_equal(got[k], want[k]), (name, cfg, k)
        for k in (2, 5, 7):
            assert relerr(got[k], want[k]) <= KTOL, (name, cfg, k)
        if name != "unstr_mid":
            assert np.array_equal(got[6], want[6])
        if base is None:
            base = got
        else:
            _assert_factors_identical(got, base, (name, cfg))
