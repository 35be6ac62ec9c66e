"""GPU: the SpMV form a matrix gets is one decision -- what bis_mat_spmv_stream_info reports is what bis_spmv launches
(bis_mat_spmv_kernel), before and after the first launch, and the report builds nothing the launch does not use.  On every
catalogue matrix (tests/helpers.py) under the default options, under every configuration of test_gpu_option_paths.py's
SPMV_CONFIGS (which include spmv_window = 1) and with the dictionary / win8 forms switched off one by one; the catalogue's
very_long_row has a row past the LDS budget.  The fused SpMV runs through a CG of a few iterations; the second test runs
it in a context of its own per form, so that the partials buffer is sized by that call alone (bis_spmv_partials_bound)."""
import numpy as np
import pytest

from helpers import OptionScope, SPMV_CATALOGUE, spmv_catalogue_case, spmv_catalogue_x
from test_gpu_option_paths import SPMV_CONFIGS

pytestmark = pytest.mark.gpu

# public form numbers (include/bis_hip.h) by the prefix of the kernel name; everything else is form 0
FORM_OF_PREFIX = [("sellwin", (4, 5)), ("spmv_rowmajor_vd_kernel", (2, 3)), ("spmv_rowblock_vd_kernel", (1,)), ("win8", (6,)),
                  ("colslab", (7,))]
CONFIGS = [dict()] + SPMV_CONFIGS + [dict(spmv_sellwin=0), dict(spmv_valdict=1), dict(spmv_valdict=0),
                                     dict(spmv_valdict=0, spmv_win8=0), dict(spmv_valdict=0, spmv_win8=0, spmv_colslab=0)]
NO_WIN8 = (0, 0, 0, 0, False)


def forms_of(kernel):
    assert kernel
    for prefix, forms in FORM_OF_PREFIX:
        if kernel.startswith(prefix):
            return forms
    return (0,)


def fused_cg(ctx, dA, iters=3):
    """a few iterations of the fused CG (tolerance 0: all of them execute); the fused SpMV's kernel name"""
    n = dA.n_rows
    b, x = ctx.upload(np.full(n, 1.0)), ctx.upload(np.full(n, 0.1))
    cg = ctx.cg(dA, b, x)
    try:
        cg.init(0.0)
        cg.iterate(iters)
        cg.status()
    finally:
        cg.free(); b.free(); x.free()
    return dA.spmv_kernel(fused=True)


@pytest.mark.parametrize("name", SPMV_CATALOGUE)
def test_report_names_the_form_that_runs(oracle, name):
    from basic_iterative_solvers_amd import BisError, Context
    A, rp64 = spmv_catalogue_case(name, oracle)
    x = spmv_catalogue_x(A, seed=5, scale=0.5 if name == "extreme_values" else 1.0)
    long_rows = int(np.diff(A.row_ptr).max(initial=0)) + 256 + 8 > 8192  # past the LDS budget of every chunk
    ctx = Context()
    try:
        for cfg in CONFIGS:
            with OptionScope(ctx, force_rp64=rp64, **cfg):
                dA = ctx.matrix(A)
                dx, dy = ctx.upload(x), ctx.alloc(A.n_rows)
                before = dA.spmv_stream_info()
                assert dA.spmv_kernel() == "", (name, cfg)  # (the report launches nothing)
                ctx.spmv(dA, dx, dy)
                k = dA.spmv_kernel()
                info = dA.spmv_stream_info()
                print(name, cfg, k, info, dA.spmv_streamed_bytes())
                assert info == before, (name, cfg, k, before, info)
                assert info[3] in forms_of(k), (name, cfg, k, info)
                if long_rows:
                    assert k == "spmv_wave_per_row_kernel" and info == (4, 8, 0, 0), (name, cfg, k, info)
                if not k.startswith("win8"):
                    assert dA.win8_layout() == NO_WIN8, (name, cfg, k, dA.win8_layout())
                if A.n_rows == A.n_cols:
                    if long_rows:
                        with pytest.raises(BisError, match="fused dot unsupported"):
                            fused_cg(ctx, dA)
                    else:
                        kf = fused_cg(ctx, dA)  # (must not raise "partials buffer too small")
                        ff = forms_of(kf)
                        # the two block tables pack their columns independently: a row-block kernel (forms 0, 1) may pair
                        # with the other row-block kernel; every other form is the matrix', whatever the table
                        assert info[3] in ff or (set(ff) | {info[3]}) <= {0, 1}, (name, cfg, k, kf, info)
                        if not (k.startswith("win8") or kf.startswith("win8")):
                            assert dA.win8_layout() == NO_WIN8, (name, cfg, k, kf)
                        assert dA.spmv_stream_info() == before, (name, cfg, k, kf)
                dA.free(); dx.free(); dy.free()
    finally:
        ctx.close()


@pytest.mark.parametrize("cfg,prefix", [(dict(), "sellwin"), (dict(spmv_sellwin=0), "spmv_rowmajor_vd_kernel"),
                                        (dict(spmv_valdict=1), "spmv_rowblock"), (dict(spmv_valdict=0), "win8"),
                                        (dict(spmv_valdict=0, spmv_win8=0), "spmv_rowblock_kernel"),
                                        (dict(spmv_window=1), "spmv_")])
def test_fused_cg_partials_bound(cfg, prefix):
    """HPCG 128^3 (2.1 M rows: the forms on 64-row slices and 256-row blocks write 32768 partials, twice what a fresh context
    holds) in a context of its own per form: the buffer bis_cg_iterate sizes before any form exists holds what the fused SpMV
    then writes.  The report before the first launch names the form that runs."""
    from basic_iterative_solvers_amd import Context
    ctx = Context()
    try:
        with OptionScope(ctx, **cfg):
            dA = ctx.gen_hpcg(128)
            before = dA.spmv_stream_info()
            kf = fused_cg(ctx, dA)
            print(cfg, kf, before)
            assert kf.startswith(prefix), (cfg, kf)
            if "spmv_window" not in cfg:
                assert before[3] in forms_of(kf), (cfg, kf, before)
            assert dA.spmv_stream_info() == before
            dA.free()
    finally:
        ctx.close()
