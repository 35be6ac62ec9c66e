"""GPU: the lifecycle of the SpMV forms that own their state (bis_spmv_forms.hpp: packed columns, value dictionary and its
lane-per-row blocks, x window; sellwin, win8, column slabs) -- build at the first SpMV, drop and rebuild at bis_mat_retune,
drop of everything derived from the values at bis_mat_scale_sym, free.

Matrices: the 7-point Laplacian on 9 x 9 x 9 (729 rows, three 256-row blocks, a plain dictionary of two values) and an
Anderson matrix with L = 12 (1728 rows; random diagonal, so the dictionary keeps the diagonal's values per row).  For
each option set: SpMV; retune and SpMV again -- same reported form, same kernel, same bits --; scale_sym, after which the
values are new and the form is resolved anew: y bit-identical to the same product of the same scaled matrix with every
compressed form off; retune again; free.

Row views (bis_mat_row_view) are made by the row-partitioned layer only: rank 1 of 2, cut so that its interior rows start at
local row 81 (Laplacian) / 144 (Anderson), not a multiple of 256; the view has a view_row0 and a dictionary of its own.  The
public interface has no retune or scale_sym on those views, so there the test runs the SpMV twice -- same report, same bits
-- compares with the run that has every compressed form off, and destroys the handle."""
import functools

import numpy as np
import pytest

import dist_loopback as L
from helpers import OptionScope
from oracle.pyoracle import CRS

pytestmark = pytest.mark.gpu

OPTION_SETS = [dict(), dict(spmv_sellwin=0), dict(spmv_valdict=1), dict(spmv_valdict=0), dict(spmv_window=1), dict(spmv_packed=0)]
PLAIN = dict(spmv_valdict=0, spmv_win8=0, spmv_packed=0, spmv_colslab=0)  # every compressed form off
CUT = {"laplace9": 81, "anderson12": 144}  # first row of rank 1: one grid plane


def laplace9():
    n1 = 9
    idx = np.arange(n1 ** 3).reshape(n1, n1, n1)  # [z, y, x]
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(n1 ** 3, 6.0)]
    for axis in range(3):
        for lo, hi in ((slice(None, -1), slice(1, None)), (slice(1, None), slice(None, -1))):
            a, b = [slice(None)] * 3, [slice(None)] * 3
            a[axis], b[axis] = lo, hi
            rows.append(idx[tuple(a)].ravel()); cols.append(idx[tuple(b)].ravel()); vals.append(np.full(rows[-1].size, -1.0))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n1 ** 3))]).astype(np.int64)
    return CRS(n1 ** 3, rp, cols[order].astype(np.int32), vals[order], n_cols=n1 ** 3)


@functools.lru_cache(maxsize=None)
def case(name):
    """(A, x, y of the scaled matrix with every compressed form off) -- computed once per matrix, shared, never written"""
    from basic_iterative_solvers_amd import Context
    ctx = Context()
    try:
        if name == "laplace9":
            A = laplace9()
        else:
            g = ctx.gen_anderson(12)
            rp, col, val = g.download()
            g.free()
            A = CRS(len(rp) - 1, rp, col, val, n_cols=len(rp) - 1)
        x = np.random.default_rng(7).uniform(-1.0, 1.0, A.n_rows)
        with OptionScope(ctx, **PLAIN):
            dA, dx, dy = ctx.matrix(A), ctx.upload(x), ctx.alloc(A.n_rows)
            ctx.scale_sym(dA).free()
            ctx.spmv(dA, dx, dy)
            assert dA.spmv_kernel().startswith("spmv_rowblock_kernel") and dA.spmv_stream_info() == (4, 8, 0, 0)
            y_scaled = dy.to_host()
            dA.free(); dx.free(); dy.free()
    finally:
        ctx.close()
    for v in (x, y_scaled):
        v.setflags(write=False)
    return A, x, y_scaled


@pytest.mark.parametrize("cfg", OPTION_SETS, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()) or "default")
@pytest.mark.parametrize("name", ["laplace9", "anderson12"])
def test_build_retune_scale_free(name, cfg):
    from basic_iterative_solvers_amd import Context
    A, x, y_scaled = case(name)
    ctx = Context()
    try:
        with OptionScope(ctx, **cfg):
            dA, dx, dy = ctx.matrix(A), ctx.upload(x), ctx.alloc(A.n_rows)
            ctx.spmv(dA, dx, dy)
            first = (dA.spmv_stream_info(), dA.spmv_kernel(), dy.to_host())
            print(name, cfg, first[0], first[1])
            dA.retune()
            dy2 = ctx.upload(np.full(A.n_rows, np.nan))
            ctx.spmv(dA, dx, dy2)
            assert (dA.spmv_stream_info(), dA.spmv_kernel()) == first[:2], (name, cfg, first[:2])
            assert L.same_bits(dy2.to_host(), first[2]), (name, cfg, first[1])
            ctx.scale_sym(dA).free()  # the values leave the dictionary: the form is resolved anew
            ctx.spmv(dA, dx, dy)
            print(name, cfg, "scaled:", dA.spmv_stream_info(), dA.spmv_kernel())
            assert L.same_bits(dy.to_host(), y_scaled), (name, cfg, dA.spmv_kernel())
            dA.retune()
            dA.free(); dx.free(); dy.free(); dy2.free()
    finally:
        ctx.close()


def view_spmv(ctx, name, cfg):
    """rank 1 of 2 (rows from CUT[name] on): the distributed SpMV twice; (report, y)"""
    from basic_iterative_solvers_amd import Dist
    A, x, _ = case(name)
    rs = np.array([0, CUT[name], A.n_rows], dtype=np.int64)
    plans = L.case_plans(A, rs)
    halo, recv, (a, b) = plans[1]
    assert a % 256 != 0 and b - a > 512, (a, b)  # the interior rows' view: cut off a block boundary, three blocks or more
    sc, scols = L.send_lists([(h, r) for h, r, _ in plans], 1)
    with OptionScope(ctx, **cfg):
        d = Dist(ctx, ctx.matrix(L.local_rows(A, int(rs[1]), int(rs[2]))), 1, 2, rs)
        d.set_send_lists(sc, scols)
        tr = L.KnownVectorTransport(x, sc, scols, halo, recv)
        d.set_comm(tr.ops)
        xe = np.concatenate([x[rs[1]:], np.full(len(halo), np.nan)])
        out = []
        for _ in range(2):
            x_ext, y = ctx.upload(xe), ctx.upload(np.full(d.n_local, np.nan))
            with tr.checked():
                d.spmv(x_ext, y)
            out.append((d.spmv_stream_info(), y.to_host()))
            x_ext.free(); y.free()
        assert all(tr.sendbuf_exact)
        assert out[0][0] == out[1][0] and L.same_bits(out[0][1], out[1][1]), (name, cfg, out[0][0], out[1][0])
        d.free()
    return out[0]


@pytest.mark.parametrize("name", ["laplace9", "anderson12"])
def test_row_view(name):
    from basic_iterative_solvers_amd import Context
    ctx = Context()
    try:
        info_plain, y_plain = view_spmv(ctx, name, PLAIN)
        assert info_plain == (4, 8, 0, 0), info_plain
        assert not np.isnan(y_plain).any()
        for cfg in OPTION_SETS:
            info, y = view_spmv(ctx, name, cfg)
            print(name, cfg, info)
            assert L.same_bits(y, y_plain), (name, cfg, info)
    finally:
        ctx.close()
