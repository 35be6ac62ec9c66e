"""GPU: bis_mapply_preconditioner (the preconditioner apply on n x k interleaved blocks) column by column against
bis_apply_preconditioner, bit for bit, and against the oracle at the kernel gate; bis_mitrsv against bis_itrsv; the types
that have no multi-vector form."""
import numpy as np
import pytest

from helpers import crs_of, load_golden, relerr
from oracle.pyoracle import CRS, Oracle

pytestmark = pytest.mark.gpu

KTOL = 1e-13  # kernel-level relative tolerance (tests/test_gpu_kernels.py)
MATS = ["hpcg_4x6x5", "FDM-2d-16", "fem444"]
KS = (2, 5, 8)
# (type, inner): the types the dispatcher serves; for "bj" the second entry is the block size (5: no power of two)
TYPES = [("none", 0), ("j", 0), ("gs", 0), ("bgs", 0), ("sgs", 0), ("ilu0", 0), ("ilu0it", 0), ("ilu0it", 1), ("ilu0it", 3),
         ("fsai", 0), ("bj", 4), ("bj", 5)]
NO_ORACLE = ("ilu0it", "fsai", "bj")  # the types the oracle does not have


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def host(dM):
    return CRS(dM.n_rows, *dM.download())


@pytest.fixture(scope="module")
def setups(ctx):
    """Per matrix: the strict triangles and diagonal of A, the device ILU(0) factors, 1 / U_D, device and host copies."""
    out = {}
    for name in MATS:
        dA = ctx.gen_fem(4, 4, 4) if name == "fem444" else ctx.matrix(crs_of(load_golden(name), "A"))
        n = dA.n_rows
        Ls, Us, D, Dinv = ctx.split_strict(dA)
        iLs, iLD, iUs, iUD = ctx.ilu0(dA)
        iUinv = ctx.alloc(n)
        ctx.elemwise_div_vectors(iUinv, iLD, iUD)
        ones = ctx.upload(np.ones(n))
        G, Gt, _ = ctx.fsai(dA)
        bj = {bs: ctx.bjacobi(dA, block_size=bs) for bs in (4, 5)}
        out[name] = dict(n=n, dA=dA, Ls=Ls, Us=Us, D=D, Dinv=Dinv, iLs=iLs, iLD=iLD, iUs=iUs, iUD=iUD, iUinv=iUinv, ones=ones,
                         G=G, Gt=Gt, bj=bj,
                         h=dict(Ls=host(Ls), Us=host(Us), D=D.to_host(), Dinv=Dinv.to_host(), iLs=host(iLs), iUs=host(iUs),
                                iLD=iLD.to_host(), iUD=iUD.to_host()))
    return out


def operands(s, pc, block_size=0):
    """(Ls, Us, A_D, A_D_inv, L_D, U_D) as bis_apply_preconditioner takes them for this type"""
    if pc == "fsai":  # G and Gt; the diagonal arguments are not read
        return s["G"], s["Gt"], None, None, None, None
    if pc == "bj":  # the handle's operand; nothing else is read
        return s["bj"][block_size].operand, None, None, None, None, None
    if pc == "ilu0":
        return s["iLs"], s["iUs"], s["D"], s["Dinv"], s["iLD"], s["iUD"]
    if pc == "ilu0it":
        return s["iLs"], s["iUs"], s["D"], s["iUinv"], s["iLD"], s["iUD"]
    return s["Ls"], s["Us"], s["D"], s["Dinv"], s["ones"], s["ones"]


def block(n, k, seed):
    rng = np.random.default_rng(seed)
    V = rng.uniform(-1, 1, (n, k))
    for j in range(1, k):
        V[:, j] *= (1.0, 1e-6, 1e6)[j % 3]
    return V


@pytest.mark.parametrize("pc,inner", TYPES)
@pytest.mark.parametrize("name", MATS)
def test_columns_equal_the_single_vector_apply(ctx, setups, name, pc, inner):
    s = setups[name]
    n = s["n"]
    ops = operands(s, pc, inner)
    if pc == "bj":
        assert s["bj"][inner].max_block == inner
        inner = 0
    orc = Oracle()
    h = s["h"]
    for k in KS:
        V = block(n, k, seed=k)
        # the single-vector dispatcher on every column
        ref = np.empty((n, k))
        inp, out, tmp, work = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
        for j in range(k):
            inp.set(V[:, j].copy())
            ctx.apply_preconditioner(pc, n, *ops, out, inp, tmp, work, inner=inner)
            ref[:, j] = out.to_host()
        for v in (inp, out, tmp, work):
            v.free()
        IN, OUT, TMP, WORK = ctx.upload(V.ravel()), ctx.alloc(n * k), ctx.alloc(n * k), ctx.alloc(n * k)
        ctx.mapply_preconditioner(pc, n, k, *ops, OUT, IN, TMP, WORK, inner=inner)
        got = OUT.to_host().reshape(n, k)
        assert same_bits(IN.to_host().reshape(n, k), V), "IN was written"
        ctx.mapply_preconditioner(pc, n, k, *ops, IN, IN, TMP, WORK, inner=inner)  # OUT aliasing IN
        got_alias = IN.to_host().reshape(n, k)
        if pc == "fsai":  # TMP holds G IN between the two bis_spmm: it must be distinct from OUT and from IN
            from basic_iterative_solvers_amd import BisError
            for out_, in_, tmp_ in ((OUT, IN, OUT), (OUT, IN, IN), (IN, IN, IN)):
                with pytest.raises(BisError, match="status 2"):
                    ctx.mapply_preconditioner(pc, n, k, *ops, out_, in_, tmp_, WORK, inner=inner)
            assert same_bits(IN.to_host().reshape(n, k), got_alias), "a refused call wrote"
        for v in (IN, OUT, TMP, WORK):
            v.free()
        for j in range(k):
            assert same_bits(got[:, j], ref[:, j]), (name, pc, inner, k, j, int(np.sum(got[:, j] != ref[:, j])))
            assert same_bits(got_alias[:, j], ref[:, j]), (name, pc, inner, k, j, "in place")
        if pc not in NO_ORACLE:  # the oracle has every other type
            hops = ((h["iLs"], h["iUs"], h["D"], h["Dinv"], h["iLD"], h["iUD"]) if pc == "ilu0" else
                    (h["Ls"], h["Us"], h["D"], h["Dinv"], None, None))
            for j in range(k):
                want = orc.apply_preconditioner(pc, *hops, V[:, j].copy())
                err = relerr(got[:, j], want)
                print(f"{name} {pc} k={k} j={j}: relerr against the oracle {err:.3e}")
                assert err <= KTOL, (name, pc, k, j, err)


@pytest.mark.parametrize("name", MATS)
def test_mitrsv_columns_equal_itrsv(ctx, setups, name):
    s = setups[name]
    n = s["n"]
    for T, Dinv in ((s["Ls"], s["Dinv"]), (s["Us"], s["Dinv"]), (s["iLs"], s["iLD"]), (s["iUs"], s["iUinv"])):
        for k in KS:
            V = block(n, k, seed=20 + k)
            B, X, W = ctx.upload(V.ravel()), ctx.alloc(n * k), ctx.alloc(n * k)
            b, x, w = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
            for sweeps in (0, 1, 2, 3):
                ctx.mitrsv(T, Dinv, B, X, W, sweeps, k)
                got = X.to_host().reshape(n, k)
                for j in range(k):
                    b.set(V[:, j].copy())
                    ctx.itrsv(T, Dinv, b, x, w, sweeps)
                    assert same_bits(got[:, j], x.to_host()), (name, k, sweeps, j, T.spmm_kernel(), T.itrsv_kernel())
            for v in (B, X, W, b, x, w):
                v.free()


def test_diag_kernels(ctx, setups):
    s = setups["fem444"]
    n, k = s["n"], 5
    V = block(n, k, seed=3)
    D = s["h"]["D"]
    A, R = ctx.upload(V.ravel()), ctx.alloc(n * k)
    ctx.mvec_div_diag(R, A, s["D"], n, k)
    assert same_bits(R.to_host().reshape(n, k), V / (1.0 * D[:, None]))
    ctx.mvec_mul_diag(R, A, s["D"], n, k)
    assert same_bits(R.to_host().reshape(n, k), V * 1.0 * D[:, None])
    ctx.mvec_mul_diag(A, A, s["D"], n, k)  # in place
    assert same_bits(A.to_host().reshape(n, k), V * 1.0 * D[:, None])
    A.free(); R.free()


def test_types_without_a_multi_vector_form(ctx, setups):
    from basic_iterative_solvers_amd import BisError
    s = setups["hpcg_4x6x5"]
    n, k = s["n"], 4
    IN, OUT, TMP, WORK = ctx.upload(block(n, k, 1).ravel()), ctx.alloc(n * k), ctx.alloc(n * k), ctx.alloc(n * k)
    ops = operands(s, "gs")
    for pc in ("2st", "s2st"):
        with pytest.raises(BisError, match="status 6"):  # BIS_ERR_UNSUPPORTED
            ctx.mapply_preconditioner(pc, n, k, *ops, OUT, IN, TMP, WORK, inner=2)
    with pytest.raises(BisError, match="status 6"):
        ctx.mapply_preconditioner("gs", n, k, *ops, OUT, IN, TMP, WORK, outer=2)
    for bad_k in (0, 9):
        with pytest.raises(BisError, match="status 2"):
            ctx.mapply_preconditioner("gs", n, bad_k, *ops, OUT, IN, TMP, WORK)
    for v in (IN, OUT, TMP, WORK):
        v.free()
