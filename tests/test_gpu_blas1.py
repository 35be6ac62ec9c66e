"""The BLAS-1 and device-scalar layer (csrc/bis_blas1.hip) at alignment, tail and grid-cap edges.

Every elementwise kernel and every reduction has a 16-byte (double2) form -- all pointers 16-byte aligned and n >= 2,
the odd element patched by block 0, thread 0 -- and a scalar form, each with a grid cap (16384 workgroups elementwise,
8192 for the reductions) past which the grid-stride loop takes another trip.  The tests here

  * restate the reduction order in numpy (restated_sum: a pure function, tested on the CPU) and hold bis_dot,
    bis_dot_dev, bis_sumsq_dev, bis_euclidean_vec_norm and bis_axpy_dot_dev to it bit for bit on dyadic inputs whose
    products are exact (there fma(a, b, acc) == acc + a*b, so numpy needs no fma), and on a probe of half ulps in
    lane 0 that makes the order inside one lane show in the final bits;
  * hold the same reductions on general inputs (magnitudes over six decades, mixed signs, one cancellation case) to
    k 2^-53 sum|a_i b_i| of the np.longdouble sum, k the depth of the summation tree derived from n;
  * hold the elementwise kernels to IEEE numpy (mult, div, scale, copy, init: every bit) or to a correctly rounded fma
    (sub, sum, normalize_x: a sample of the edges, the trip boundaries and 20 000 random indices; the rest within one
    ulp of plain numpy), at both alignments of every pointer, aliased, inside guard bands nothing may write to;
  * bis_multi_axpy, the one-thread scalar kernels, the argument checks;
  * the Jacobi device schedule against the kernel-by-kernel schedule past the reduction's grid cap.

Worst observed error / bound of the general-input reductions on an MI355X (observations, not gates):
dot 0.0266, dot with cancellation 0.0406, sum of squares 0.0474, fused axpy + dot 0.0324.
"""
import ctypes as C
import math

import numpy as np
import pytest

T = 256            # threads of a workgroup (kEwThreads)
DOT_CAP = 8192     # kMaxDotBlocks
EW_CAP = 16384     # kMaxEwBlocks
GUARD = 64
SENT = -1.2345678e77  # guard-band sentinel: no kernel here produces it
U = 2.0 ** -53
BIS_OK, BIS_ERR_INVALID = 0, 2

SMALL = [0, 1, 2, 3, 255, 256, 257, 511, 512, 513]
C1, C2 = T * DOT_CAP, 2 * T * DOT_CAP
RED_VEC_SIZES = SMALL + [C2 - 1, C2, C2 + 2, C2 + 3, 3 * T * DOT_CAP + 1]
RED_SCALAR_SIZES = SMALL + [C1 - 1, C1, C1 + 2, C1 + 3, 3 * T * DOT_CAP + 1]
RED_NMAX = 3 * T * DOT_CAP + 1
E1, E2 = T * EW_CAP, 2 * T * EW_CAP
EW_VEC_BIG = [E2 - 1, E2, E2 + 2, E2 + 3]
EW_SCALAR_BIG = [E1, E1 + 1]
EW_NMAX = E2 + 3
SCALES = [1.0, -1.25, 0.0, 2.0 ** -1070]


# ---- the reduction order, restated ---------------------------------------------------------------------------------

def red_grid(n, vec, cap=DOT_CAP):
    """Workgroups of a reduction (ew_grid) over n elements: one lane per element, or per pair in the double2 form."""
    items = (n >> 1) if vec else n
    return min(max(-(-items // T), 1), cap)


def schedule(n, vec, grid):
    """The index map as a list of steps (accumulator, first lane, slice of elements) in the order a lane performs them:
    the elements of a step go to consecutive lanes from `first lane`, one each.  Scalar form: element i to lane
    i mod (grid T), trip after trip.  double2 form: pair i to that lane, its two elements to acc0 and acc1; the odd
    element to acc0 of lane 0 of block 0 after that lane's loop."""
    L = grid * T
    steps = []
    if vec:
        n2 = n >> 1
        for t in range(-(-n2 // L)):
            lo, hi = t * L, min((t + 1) * L, n2)
            steps.append((0, 0, slice(2 * lo, 2 * hi, 2)))
            steps.append((1, 0, slice(2 * lo + 1, 2 * hi, 2)))
        if n & 1:
            steps.append((0, 0, slice(n - 1, n)))
    else:
        for t in range(-(-n // L)):
            steps.append((0, 0, slice(t * L, min((t + 1) * L, n))))
    return steps


def wave_sum(v):
    """wave_sum over the last axis (64 lanes): v[:32] + v[32:], then halves again down to 1 (lane 0 of the shuffles)."""
    w = 32
    while w >= 1:
        v = v[..., :w] + v[..., w:2 * w]
        w >>= 1
    return v[..., 0]


def block_sum(v):
    """block_sum<256> over the last axis: 0.0 + w0 + w1 + w2 + w3 of the four wave sums."""
    w = wave_sum(v.reshape(v.shape[:-1] + (4, 64)))
    r = np.zeros(w.shape[:-1])
    for i in range(4):
        r = r + w[..., i]
    return r


def finish_sum(partials):
    """reduce_finish_kernel: thread t adds p[t], p[t + 256], ... serially from 0.0, then a block_sum<256>."""
    acc = np.zeros(T)
    for k in range(0, len(partials), T):
        seg = partials[k:k + T]
        acc[:len(seg)] += seg
    return float(block_sum(acc))


def restated_sum(p, vec):
    """Sum of the (exact) products p in the order dot_partial_kernel / axpy_dot_kernel + reduce_finish_kernel form it:
    `vec` says whether the double2 form runs (all operands 16-byte aligned and len(p) >= 2)."""
    p = np.asarray(p, dtype=np.float64)
    n = len(p)
    assert not vec or n >= 2
    grid = red_grid(n, vec)
    acc = np.zeros((2, grid * T))
    for a, lane0, sl in schedule(n, vec, grid):
        seg = p[sl]
        acc[a, lane0:lane0 + len(seg)] += seg  # products in trip order, one accumulator per lane
    return finish_sum(block_sum((acc[0] + acc[1]).reshape(grid, T)))


def lane0_probe(n, vec):
    """Products that make the order INSIDE a lane show in the final bits: 1.0 at the first element of lane 0 of block 0,
    half an ulp of it (2^-53) at every other element that lane gets (second trips, the second accumulator, the odd
    tail), zero elsewhere.  A half ulp added to 1.0 is lost (ties to even), two of them added to each other first are
    not: moving one element from acc0 to acc1 changes the sum.  (On random data a last-bit change of one lane's sum all but
    never survives the sum over the other 255 lanes of the block.)"""
    a = np.zeros(n)
    first = True
    for _, lane0, sl in schedule(n, vec, red_grid(n, vec)):
        if lane0 == 0:
            a[sl.start] = 1.0 if first else 2.0 ** -53
            first = False
    return a


def tree_depth(n, vec):
    """Depth k of the summation tree for the bound k 2^-53 sum|a_i b_i|: the lane's trip count plus 1 (the two
    accumulators / the odd element), 6 levels of wave_sum, 4 additions of block_sum, the finish lane's count, and
    the finish kernel's 6 + 4."""
    grid = red_grid(n, vec)
    items = (n >> 1) if vec else n
    return -(-items // (grid * T)) + 1 + 6 + 4 + -(-grid // T) + 6 + 4


def exact_products(a, b):
    """a * b, asserted exact (the double product equals the 64-bit-mantissa product)."""
    assert np.finfo(np.longdouble).nmant >= 63
    p = a * b
    assert np.array_equal(p.astype(np.longdouble), a.astype(np.longdouble) * b.astype(np.longdouble))
    return p


def test_restatement_index_map_and_exact_sums():
    """The restatement on the CPU: at every size and form the GPU tests use the index map touches each element exactly
    once, on lanes that exist, and on small integers (every partial sum exact) the restated sum is the exact sum."""
    ints = np.random.default_rng(7).integers(-8, 9, RED_NMAX).astype(np.float64)
    for vec, sizes in ((True, RED_VEC_SIZES + GEN_VEC_SIZES), (False, RED_SCALAR_SIZES + GEN_SCALAR_SIZES)):
        for n in sorted(set(sizes)):
            v = vec and n >= 2
            grid = red_grid(n, v)
            assert 1 <= grid <= DOT_CAP
            hits = np.zeros(n, dtype=np.int64)
            for a, lane0, sl in schedule(n, v, grid):
                hits[sl] += 1
                m = len(range(*sl.indices(n)))
                assert a in (0, 1) and 0 <= lane0 and lane0 + m <= grid * T
            assert np.all(hits == 1), (n, v)
            assert restated_sum(ints[:n], v) == float(int(ints[:n].sum())), (n, v)
            assert tree_depth(n, v) >= 22
    # the cap is reached and passed: a second (and third) trip, more than one partial per lane of the finish kernel
    assert red_grid(C2, True) == DOT_CAP == red_grid(C1, False) and len(schedule(C2 + 2, True, DOT_CAP)) == 4
    assert len(schedule(C1 + 2, False, DOT_CAP)) == 2 and len(schedule(RED_NMAX, False, DOT_CAP)) == 4
    # and the pieces: wave_sum / block_sum / finish_sum pair what the kernels pair
    w = np.zeros(64); w[[3, 35]] = [1.0, 2.0 ** -53]
    assert wave_sum(w) == 1.0 and wave_sum(np.arange(64.0)) == 2016.0
    # the lane-0 probe: half ulps that are lost one by one in acc0 but not when two of them meet in acc1 first
    assert restated_sum(lane0_probe(3, True), True) == 1.0 and restated_sum(lane0_probe(C2 + 3, True), True) == 1.0 + 2.0 ** -52
    assert np.count_nonzero(lane0_probe(C2 + 3, True)) == 5 and np.count_nonzero(lane0_probe(RED_NMAX, False)) == 4
    assert block_sum(np.arange(256.0)) == 32640.0 and finish_sum(np.arange(1000.0)) == 499500.0


def fma_exact(x, y, z):
    """Correctly rounded x*y + z for finite doubles: math.fma where the interpreter has it, otherwise exact integer
    arithmetic on the significands and one correctly rounded int / int division."""
    if hasattr(math, "fma"):
        return math.fma(x, y, z)
    (mx, ex), (my, ey), (mz, ez) = math.frexp(x), math.frexp(y), math.frexp(z)
    X, Y, Z = int(mx * 2.0 ** 53), int(my * 2.0 ** 53), int(mz * 2.0 ** 53)
    e1, e2 = ex + ey - 106, ez - 53
    e = min(e1, e2)
    N = ((X * Y) << (e1 - e)) + (Z << (e2 - e))
    if N == 0:  # an exact zero: +0 unless the (zero) product and z are both -0
        return (x * y) + z if z == 0.0 else 0.0
    return float(N << e) if e >= 0 else N / (1 << -e)


def test_fma_exact_is_correctly_rounded():
    assert fma_exact(1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52, -1.0) == -2.0 ** -104
    assert fma_exact(3.0, 2.0 ** -1074, 2.0 ** -1074) == 4 * 2.0 ** -1074 and fma_exact(0.1, 10.0, -1.0) == 2.0 ** -54
    assert math.copysign(1.0, fma_exact(-0.0, 2.0, -0.0)) == -1.0 and math.copysign(1.0, fma_exact(1.5, 2.0, -3.0)) == 1.0
    assert fma_exact(2.0 ** 600, 2.0 ** 400, 1.0) == 2.0 ** 1000
    from fractions import Fraction
    rng = np.random.default_rng(11)
    for x, y, z in (rng.choice([-1.0, 1.0], (300, 3)) * 10.0 ** rng.uniform(-3, 3, (300, 3))).tolist():
        z = -x * y * (1 + z * 1e-19) if abs(z) < 1.0 else z  # (half of them cancel almost completely)
        exact = Fraction(x) * Fraction(y) + Fraction(z)
        assert fma_exact(x, y, z) == float(exact), (x, y, z)  # (Fraction -> float is one correctly rounded division)


# ---- device plumbing -------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


def P(ptr):
    return C.c_void_p(ptr if ptr else None)


def I64(n):
    return C.c_int64(int(n))


def same_bits(x, y):
    """Bit for bit, nan position by position (the payload of a generated nan is the platform's)."""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    nx, ny = np.isnan(x), np.isnan(y)
    return x.shape == y.shape and np.array_equal(nx, ny) and np.array_equal(x.view(np.uint64)[~nx], y.view(np.uint64)[~ny])


class Guarded:
    """n doubles on the device with at least GUARD sentinel doubles on each side, starting at a 16-byte aligned address
    (off8 = 0) or 8 bytes past one (off8 = 1); read() returns them after checking that the guard bands are untouched."""

    def __init__(self, ctx, n, off8, fill=None):
        self.n, self.lead = n, GUARD + (1 if off8 else 0)
        self.host = np.full(GUARD + 1 + n + GUARD, SENT)
        if fill is not None:
            self.host[self.lead:self.lead + n] = fill
        self.vec = ctx.upload(self.host)
        self.ptr = self.vec.ptr + 8 * self.lead
        assert self.ptr % 16 == (8 if off8 else 0)

    def read(self):
        got = self.vec.to_host()
        lo, hi = self.lead, self.lead + self.n
        assert same_bits(got[:lo], self.host[:lo]) and same_bits(got[hi:], self.host[hi:]), "a write outside [0, n)"
        return got[lo:hi]

    def free(self):
        self.vec.free()


class Master:
    """A host array with one device copy; view(off8, n) is (device pointer, host operand) of n elements at a 16-byte
    aligned address (off8 = 0) or 8 bytes past it (off8 = 1) -- inside the allocation either way."""

    def __init__(self, ctx, host):
        self.host, self.vec = host, ctx.upload(host)
        assert self.vec.ptr % 16 == 0

    def view(self, off8, n):
        assert off8 + n <= len(self.host)
        return self.vec.ptr + 8 * off8, self.host[off8:off8 + n]


class Scalars:
    """A few doubles on the device for the scalar arguments and results of the _dev entry points."""

    def __init__(self, ctx, k=16):
        self.ctx, self.k, self.vec = ctx, k, ctx.upload(np.full(k, SENT))

    def at(self, i):
        return self.vec.ptr + 8 * i

    def put(self, i, v):
        self.ctx.check(self.ctx.lib.bis_vec_upload(self.ctx.h, P(self.at(i)), np.array([v], dtype=np.float64).ctypes, I64(1)))

    def get(self, i):
        return float(self.vec.to_host()[i])


def sample_indices(n, L, seed=0):
    """The first and last 600 indices, 300 on each side of every multiple of L (the trip boundaries of a grid-stride loop
    of L lanes; 2 L elements in the double2 form -- both are taken), and 20 000 random ones."""
    if n <= 25000:
        return np.arange(n)
    parts = [np.arange(600), np.arange(n - 600, n), np.random.default_rng(seed).integers(0, n, 20000)]
    for step in (L, 2 * L):
        for m in range(step, n + 300, step):
            parts.append(np.arange(max(m - 300, 0), min(m + 300, n)))
    return np.unique(np.concatenate(parts))


# ---- 2. reductions, bit for bit ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dyadic(ctx):
    """Integers below 2^26 (a) and 2^27 (b), scaled to below 1 and by a power of two of the element's own between 2^-12
    and 2^12: every product a_i b_j and a_i a_j is exact in 53 bits, and with exponents that differ from element to
    element the sums round from the first addition on.  For the fused axpy, integers below 2^22 with one power of two
    per index for both w and u: w + 1.25 u is exact in 26 bits, its products with itself and with b in 53."""
    rng = np.random.default_rng(20260101)
    N = RED_NMAX + 2
    pw = lambda: 2.0 ** rng.integers(-12, 13, N).astype(np.float64)
    wu = pw()
    d = dict(a=rng.integers(-2 ** 26 + 1, 2 ** 26, N).astype(np.float64) * 2.0 ** -26 * pw(),
             b=rng.integers(-2 ** 27 + 1, 2 ** 27, N).astype(np.float64) * 2.0 ** -27 * pw(),
             w=rng.integers(-2 ** 22 + 1, 2 ** 22, N).astype(np.float64) * wu,
             u=rng.integers(-2 ** 22 + 1, 2 ** 22, N).astype(np.float64) * wu)
    d["zeros"], d["ones"] = np.zeros(N), np.ones(N)
    m = {k: Master(ctx, v) for k, v in d.items()}
    m["a_copy"] = Master(ctx, d["a"])
    m["sc"] = Scalars(ctx)
    yield m
    for v in m.values():
        v.vec.free()


def check_lane_order(ctx, m, n, off8):
    """The lane-0 probe through bis_dot_dev and through the fused kernel (w = probe, u = 0, v = 1)."""
    sc = m["sc"]
    vec = n >= 2 and not off8
    a = lane0_probe(n, vec)
    want = restated_sum(a, vec)
    (p1, _), (p0, _) = m["ones"].view(off8, n), m["zeros"].view(off8, n)
    gw = Guarded(ctx, n, off8, fill=a)
    assert dev_dot(ctx, sc, gw.ptr, p1, n) == want, (n, off8)
    assert dev_dot(ctx, sc, p1, gw.ptr, n) == want, (n, off8)
    sc.put(0, AXPY_S)
    sc.put(2, SENT)
    assert ctx.lib.bis_axpy_dot_dev(ctx.h, P(gw.ptr), P(p0), P(sc.at(0)), P(p1), I64(n), P(sc.at(2))) == BIS_OK
    ctx.sync()
    got_w, got = gw.read(), sc.get(2)
    gw.free()
    assert same_bits(got_w, a) and got == want, (n, off8, got, want)


def dev_dot(ctx, sc, pa, pb, n, entry="bis_dot_dev"):
    sc.put(1, SENT)
    if entry == "bis_dot":
        out = C.c_double(SENT)
        assert ctx.lib.bis_dot(ctx.h, P(pa), P(pb), I64(n), C.byref(out)) == BIS_OK
        return out.value
    if entry == "bis_sumsq_dev":
        assert ctx.lib.bis_sumsq_dev(ctx.h, P(pa), I64(n), P(sc.at(1))) == BIS_OK
    else:
        assert ctx.lib.bis_dot_dev(ctx.h, P(pa), P(pb), I64(n), P(sc.at(1))) == BIS_OK
    ctx.sync()
    return sc.get(1)


def dev_norm(ctx, pa, n):
    out = C.c_double(SENT)
    assert ctx.lib.bis_euclidean_vec_norm(ctx.h, P(pa), I64(n), C.byref(out)) == BIS_OK
    return out.value


AXPY_S = -1.25


def check_axpy_dot(ctx, m, n, ow, ou, ov, with_v):
    """bis_axpy_dot_dev on dyadic operands at the given 8-byte offsets: w and the value against the restatement.  The
    fused kernel runs when the axpy and the dot would take the same form; otherwise the library runs them separately
    (axpy in one form, dot in the other) -- the dot's form decides the order of the sum either way."""
    sc = m["sc"]
    pu, u = m["u"].view(ou, n)
    pv, v = m["b"].view(ov, n)
    w0 = m["w"].host[ou:ou + n]  # (the elements that share u's powers of two, wherever w is put)
    gw = Guarded(ctx, n, ow, fill=w0)
    sc.put(0, AXPY_S)
    sc.put(2, SENT)
    st = ctx.lib.bis_axpy_dot_dev(ctx.h, P(gw.ptr), P(pu), P(sc.at(0)), P(pv) if with_v else None, I64(n), P(sc.at(2)))
    assert st == BIS_OK
    ctx.sync()
    w_new = w0 - AXPY_S * u
    assert np.array_equal(w_new.astype(np.longdouble), w0.astype(np.longdouble) - np.longdouble(AXPY_S) * u.astype(np.longdouble))
    vec_dot = n >= 2 and not ow and (not with_v or not ov)
    want = restated_sum(exact_products(w_new, v if with_v else w_new), vec_dot)
    got_w, got = gw.read(), sc.get(2)
    gw.free()
    assert same_bits(got_w, w_new), (n, ow, ou, ov, with_v)
    assert got == want, (n, ow, ou, ov, with_v, got, want)
    if n == 0:
        assert got == 0.0 and math.copysign(1.0, got) == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("n", RED_VEC_SIZES)
def test_reductions_double2_form_bit_exact(ctx, dyadic, n):
    """Aligned operands (the double2 form from n = 2 on, second and third trips past 2 * 256 * 8192 elements, 8192
    partials = 32 per lane of the finish kernel): every reduction entry point equals the restatement bit for bit."""
    m, sc = dyadic, dyadic["sc"]
    (pa, a), (pb, b), (pc, _) = m["a"].view(0, n), m["b"].view(0, n), m["a_copy"].view(0, n)
    vec = n >= 2
    want = restated_sum(exact_products(a, b), vec)
    want_sq = restated_sum(exact_products(a, a), vec)
    assert dev_dot(ctx, sc, pa, pb, n) == want
    assert dev_dot(ctx, sc, pa, pb, n, "bis_dot") == want
    assert dev_dot(ctx, sc, pa, None, n, "bis_sumsq_dev") == want_sq
    assert dev_dot(ctx, sc, pa, pa, n) == want_sq              # the SAME path ...
    assert dev_dot(ctx, sc, pa, pc, n) == want_sq              # ... against the two-operand dot of a copy
    assert dev_norm(ctx, pa, n) == math.sqrt(want_sq)
    if n == 0:
        assert want == 0.0 and want_sq == 0.0
    check_axpy_dot(ctx, m, n, 0, 0, 0, True)
    check_axpy_dot(ctx, m, n, 0, 0, 0, False)
    check_lane_order(ctx, m, n, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", RED_SCALAR_SIZES)
def test_reductions_scalar_form_bit_exact(ctx, dyadic, n):
    """Operands 8 bytes into their allocations (the scalar form; trips past 256 * 8192 elements), and mixed alignment --
    one operand aligned, one not -- which must take the scalar form too."""
    m, sc = dyadic, dyadic["sc"]
    (pa, a), (pb, b), (pc, _) = m["a"].view(1, n), m["b"].view(1, n), m["a_copy"].view(1, n)
    want = restated_sum(exact_products(a, b), False)
    want_sq = restated_sum(exact_products(a, a), False)
    assert dev_dot(ctx, sc, pa, pb, n) == want
    assert dev_dot(ctx, sc, pa, pb, n, "bis_dot") == want
    assert dev_dot(ctx, sc, pa, None, n, "bis_sumsq_dev") == want_sq
    assert dev_dot(ctx, sc, pa, pa, n) == want_sq
    assert dev_dot(ctx, sc, pa, pc, n) == want_sq
    assert dev_norm(ctx, pa, n) == math.sqrt(want_sq)
    # mixed alignment: (aligned, offset) and (offset, aligned)
    (pa0, a0), (pb0, b0) = m["a"].view(0, n), m["b"].view(0, n)
    assert dev_dot(ctx, sc, pa0, pb, n) == restated_sum(exact_products(a0, b), False)
    assert dev_dot(ctx, sc, pa, pb0, n) == restated_sum(exact_products(a, b0), False)
    assert dev_dot(ctx, sc, pa0, pc, n) == restated_sum(exact_products(a0, a), False)
    check_axpy_dot(ctx, m, n, 1, 1, 1, True)
    check_axpy_dot(ctx, m, n, 1, 1, 1, False)
    check_axpy_dot(ctx, m, n, 1, 0, 0, True)    # w offset: both steps scalar
    check_axpy_dot(ctx, m, n, 0, 0, 1, True)    # v offset only: the axpy may be double2, the dot is scalar
    check_axpy_dot(ctx, m, n, 0, 1, 0, True)    # u offset only: the axpy is scalar, the dot double2
    check_axpy_dot(ctx, m, n, 0, 1, 0, False)
    check_lane_order(ctx, m, n, 1)


# ---- 3. reductions on general inputs -------------------------------------------------------------------------------

GEN_VEC_SIZES = [3, 257, 513, C2 + 3, 3 * T * DOT_CAP + 1]
GEN_SCALAR_SIZES = [1, 257, C1 + 3, 3 * T * DOT_CAP + 1]
WORST = {}


def ld_dot(a, b):
    """(sum a_i b_i, sum |a_i b_i|) in np.longdouble."""
    p = a.astype(np.longdouble) * b.astype(np.longdouble)
    return p.sum(), np.abs(p).sum()


def record(kind, n, vec, got, refmag):
    ref, mag = refmag
    bound = tree_depth(n, vec) * np.longdouble(U) * mag
    err = abs(np.longdouble(got) - ref)
    ratio = float(err / bound) if bound > 0 else 0.0
    WORST[kind] = max(WORST.get(kind, 0.0), ratio)
    print(f"blas1 general inputs: {kind:>12} n={n:<8} form={'double2' if vec else 'scalar '} k={tree_depth(n, vec)} "
          f"err/bound={ratio:.4f} (worst so far {WORST[kind]:.4f})")
    assert err <= bound, (kind, n, vec, got, float(ref), float(bound))


def general(rng, n):
    """Doubles of mixed sign with magnitudes over six decades."""
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 3, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n,off8", [(n, 0) for n in GEN_VEC_SIZES] + [(n, 1) for n in GEN_SCALAR_SIZES])
def test_reductions_general_inputs_against_longdouble(ctx, n, off8):
    """Random doubles over six decades with mixed signs, and one cancellation case (sum|a_i b_i| >= 1e8 |sum a_i b_i|):
    within k 2^-53 sum|a_i b_i| of the np.longdouble sum, k the depth of the summation tree for this n and form."""
    rng = np.random.default_rng(1000 + 2 * n + off8)
    vec = n >= 2 and not off8
    sc = Scalars(ctx)
    a, b = general(rng, n), general(rng, n)
    # the cancellation case: move one entry of b so that the sum all but vanishes
    bc = b.copy()
    if n >= 2:
        j = int(np.argmax(np.abs(a)))
        bc[j] = 0.0
        rest, rest_mag = ld_dot(a, bc)  # (all entries but j)
        bc[j] = float((np.longdouble(1e-10) * rest_mag - rest) / np.longdouble(a[j]))
        s, mag = ld_dot(a, bc)
        assert mag >= 1e8 * abs(s)
    pad = lambda v: np.concatenate([np.zeros(off8), v])
    da, db, dbc = ctx.upload(pad(a)), ctx.upload(pad(b)), ctx.upload(pad(bc))
    pa, pb, pbc = da.ptr + 8 * off8, db.ptr + 8 * off8, dbc.ptr + 8 * off8
    assert pa % 16 == 8 * off8
    ab = ld_dot(a, b)
    record("dot", n, vec, dev_dot(ctx, sc, pa, pb, n), ab)
    record("dot", n, vec, dev_dot(ctx, sc, pa, pb, n, "bis_dot"), ab)
    ss = dev_dot(ctx, sc, pa, None, n, "bis_sumsq_dev")
    record("sumsq", n, vec, ss, ld_dot(a, a))
    assert dev_norm(ctx, pa, n) == math.sqrt(ss)
    if n >= 2:
        record("dot_cancel", n, vec, dev_dot(ctx, sc, pa, pbc, n), (s, mag))
    # the fused kernel: w -= s u on a copy of a, then (w, b) and (w, w) of the w it left
    for with_v in (True, False):
        gw = Guarded(ctx, n, off8, fill=a)
        sc.put(0, 0.37)
        assert ctx.lib.bis_axpy_dot_dev(ctx.h, P(gw.ptr), P(pbc), P(sc.at(0)), P(pb) if with_v else None, I64(n), P(sc.at(2))) == BIS_OK
        ctx.sync()
        w = gw.read()
        gw.free()
        assert np.all(np.abs(w - (a - 0.37 * bc)) <= np.spacing(np.abs(a) + np.abs(0.37 * bc)))
        for i in sample_indices(n, red_grid(n, vec) * T)[:3000].tolist():
            assert w[i] == fma_exact(-0.37, float(bc[i]), float(a[i]))
        record("axpy_dot", n, vec, sc.get(2), ld_dot(w, b if with_v else w))
    for v in (da, db, dbc, sc.vec):
        v.free()


# ---- 4. elementwise kernels ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ewdata(ctx):
    rng = np.random.default_rng(20260202)
    N = EW_NMAX + 2
    d = dict(a=general(rng, N), b=general(rng, N),
             d=rng.choice([-1.0, 1.0], N) * rng.uniform(0.5, 2.0, N), x=rng.uniform(-1, 1, N))
    m = {k: Master(ctx, v) for k, v in d.items()}
    m["sc"] = Scalars(ctx)
    yield m
    for v in m.values():
        v.vec.free()


def check_fma_result(got, a, b, s, L, tag):
    """got against fma(s, b, a): correctly rounded on the sample, within one ulp (of the operands' magnitude: the
    rounding of s*b that plain numpy adds is at most half an ulp of |s b|, and rounding is monotone) elsewhere."""
    with np.errstate(under="ignore"):
        sb = s * b
        plain = a + sb
    assert np.all(np.abs(got - plain) <= np.spacing(np.abs(a) + np.abs(sb))), tag
    idx = sample_indices(len(a), L)
    g, al, bl = got[idx].tolist(), a[idx].tolist(), b[idx].tolist()
    for k in range(len(idx)):
        e = fma_exact(s, bl[k], al[k])
        assert g[k] == e and math.copysign(1.0, g[k]) == math.copysign(1.0, e), (tag, int(idx[k]), g[k], e)


EW3 = {"sub": "bis_subtract_vectors", "sum": "bis_sum_vectors", "mult": "bis_elemwise_mult_vectors",
       "div": "bis_elemwise_div_vectors", "sub_dev": "bis_subtract_vectors_dev", "sum_dev": "bis_sum_vectors_dev"}


def run_ew3(ctx, m, op, n, ar, aa, ab, s, alias=""):
    """One three-operand launch: r, a, b at 8-byte offsets ar, aa, ab; alias names the inputs that ARE r ("a", "b", "ab")."""
    pa, a = m["a"].view(aa, n)
    pb, b = m["b"].view(ab, n)
    if alias == "ab":
        b = a
    fill = a if "a" in alias else (b if "b" in alias else None)
    gr = Guarded(ctx, n, ar, fill=fill)
    if "a" in alias:
        pa = gr.ptr
    if "b" in alias:
        pb = gr.ptr
    fn = getattr(ctx.lib, EW3[op])
    if op.endswith("_dev"):
        m["sc"].put(0, s)
        st = fn(ctx.h, P(gr.ptr), P(pa), P(pb), I64(n), P(m["sc"].at(0)))
    else:
        st = fn(ctx.h, P(gr.ptr), P(pa), P(pb), I64(n), C.c_double(s))
    assert st == BIS_OK
    ctx.sync()
    got = gr.read()
    gr.free()
    tag = (op, n, ar, aa, ab, s, alias)
    vec = n >= 2 and not (ar or ("a" not in alias and aa) or ("b" not in alias and ab))
    L = red_grid(n, vec, EW_CAP) * T
    with np.errstate(all="ignore"):
        if op == "mult":
            assert same_bits(got, (a * s) * b), tag
        elif op == "div":
            assert same_bits(got, a / (s * b)), tag
        else:
            check_fma_result(got, a, b, -s if op.startswith("sub") else s, L, tag)


def ew3_cases(n):
    """(ar, aa, ab, scales, alias): every alignment of r, a and b and every aliasing at the small sizes; at the cap sizes
    the alignments that take the form the size is about (double2: all aligned; scalar: all three pointers off, and each
    in turn), one scale -- and every scale and the aliasing at the last size of each form (a vector of 8.4 M doubles
    costs a tenth of a second to send, fetch and compare: the cases at the caps are kept to those that differ)."""
    if n <= 1024:
        for ar in (0, 1):
            for aa in (0, 1):
                for ab in (0, 1):
                    yield ar, aa, ab, SCALES, ""
            for alias in ("a", "b", "ab"):
                yield ar, ar, ar, SCALES, alias
    elif n in EW_VEC_BIG:
        yield 0, 0, 0, (SCALES if n == EW_VEC_BIG[-1] else [-1.25]), ""
        if n == EW_VEC_BIG[-1]:
            for alias in ("a", "b", "ab"):
                yield 0, 0, 0, [-1.25], alias
    elif n == EW_SCALAR_BIG[0]:
        for ar, aa, ab in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            yield ar, aa, ab, [-1.25], ""
    else:
        yield 1, 1, 1, SCALES, ""
        yield 1, 1, 1, [-1.25], "ab"


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL + EW_VEC_BIG + EW_SCALAR_BIG)
@pytest.mark.parametrize("op", list(EW3))
def test_elementwise_three_operand(ctx, ewdata, op, n):
    """subtract / sum / mult / div (and the device-scalar forms of the first two): values, aliasing and guard bands."""
    for ar, aa, ab, scales, alias in ew3_cases(n):
        for s in scales:
            run_ew3(ctx, ewdata, op, n, ar, aa, ab, s, alias)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL + EW_VEC_BIG + EW_SCALAR_BIG)
@pytest.mark.parametrize("op", ["scale", "scale_dev", "copy", "init"])
def test_elementwise_two_operand(ctx, ewdata, op, n):
    """scale, scale_dev, copy_vector and init_vector: plain IEEE, every bit, at both alignments of r and a; in-place
    scale; copy_vector(out, out)."""
    m, lib = ewdata, ctx.lib
    big = n > 1024
    if not big:
        combos = [(ar, aa, False) for ar in (0, 1) for aa in (0, 1)] + [(0, 0, True), (1, 1, True)]
    elif n in EW_VEC_BIG:
        combos = [(0, 0, False), (0, 0, True)]
    else:
        combos = [(1, 1, False), (1, 0, False), (0, 1, False), (1, 1, True)]
    for k, (ar, aa, inplace) in enumerate(combos):
        if op == "init" and (aa or inplace):
            continue
        for s in (SCALES if not big or (k == 0 and n in (EW_VEC_BIG[-1], EW_SCALAR_BIG[-1])) else [-1.25]):
            pa, a = m["a"].view(aa, n)
            gr = Guarded(ctx, n, ar, fill=a if inplace else None)
            if inplace:
                pa = gr.ptr
            if op == "scale":
                st = lib.bis_scale(ctx.h, P(gr.ptr), P(pa), C.c_double(s), I64(n))
            elif op == "scale_dev":
                m["sc"].put(0, s)
                st = lib.bis_scale_dev(ctx.h, P(gr.ptr), P(pa), P(m["sc"].at(0)), I64(n))
            elif op == "copy":
                st = lib.bis_copy_vector(ctx.h, P(gr.ptr), P(pa), I64(n))
            else:
                st = lib.bis_init_vector(ctx.h, P(gr.ptr), C.c_double(s), I64(n))
            assert st == BIS_OK
            ctx.sync()
            got = gr.read()
            gr.free()
            with np.errstate(under="ignore"):
                want = a * s if op.startswith("scale") else (a if op == "copy" else np.full(n, s))
            assert same_bits(got, want), (op, n, ar, aa, inplace, s)
            if op == "copy":
                break  # (no scale)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL + EW_SCALAR_BIG)
def test_normalize_x(ctx, ewdata, n):
    """x_new <- (b - fma(-D, x_old, x_new)) / D (methods/jacobi.hpp:27-40) at every alignment of its four pointers: the
    fma correctly rounded on the sample, the whole vector within the one ulp of the fma carried through the subtraction
    and the division; nothing outside [0, n) written."""
    m = ewdata
    if n <= 1024:
        combos = [(k >> 3 & 1, k >> 2 & 1, k >> 1 & 1, k & 1) for k in range(16)]
    else:
        combos = [(0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 1, 0)]
    L = red_grid(n, False, EW_CAP) * T
    for an, ao, ad, ab in combos:
        _, xn = m["a"].view(an, n)
        po, xo = m["x"].view(ao, n)
        pd, d = m["d"].view(ad, n)
        pb, b = m["b"].view(ab, n)
        gx = Guarded(ctx, n, an, fill=xn)
        assert ctx.lib.bis_normalize_x(ctx.h, P(gx.ptr), P(po), P(pd), P(pb), I64(n)) == BIS_OK
        ctx.sync()
        got = gx.read()
        gx.free()
        dx = d * xo
        adj = xn - dx
        plain = (b - adj) / d
        u1 = np.spacing(np.abs(xn) + np.abs(dx))
        u2 = np.spacing(np.abs(b) + np.abs(adj))
        assert np.all(np.abs(got - plain) <= (u1 + u2) / np.abs(d) * (1 + 2.0 ** -50) + np.spacing(np.abs(plain))), (n, an, ao, ad, ab)
        idx = sample_indices(n, L)
        g, xl, ol, dl, bl = (v[idx].tolist() for v in (got, xn, xo, d, b))
        for k in range(len(idx)):
            assert g[k] == (bl[k] - fma_exact(-dl[k], ol[k], xl[k])) / dl[k], (n, an, ao, ad, ab, int(idx[k]))


# ---- 5. bis_multi_axpy -----------------------------------------------------------------------------------------------

MA_BIG = E1 + 1


@pytest.fixture(scope="module")
def madata(ctx):
    """One master vector per kind of input; column k of V is its slice [37 k, 37 k + n): 64 distinct columns without
    64 n doubles of host data.  Dyadic: integers below 2^12 and coefficients in eighths below 2^6, so that every product
    and every partial sum over 64 columns is exact."""
    rng = np.random.default_rng(20260303)
    N = MA_BIG + 37 * 64
    d = dict(dy=rng.integers(-2 ** 12 + 1, 2 ** 12, N).astype(np.float64), ge=general(rng, N))
    y = dict(dy=rng.integers(-2 ** 9 + 1, 2 ** 9, 65).astype(np.float64) / 8.0, ge=general(rng, 65))
    m = {k: Master(ctx, v) for k, v in d.items()}
    m["V"] = ctx.alloc(64 * (MA_BIG + 7) + 2)
    m["y"] = y
    yield m
    for k in ("dy", "ge"):
        m[k].vec.free()
    m["V"].free()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 257, MA_BIG])
@pytest.mark.parametrize("n_vec", [0, 1, 5, 64])
def test_multi_axpy(ctx, madata, n_vec, n):
    """out[i] = sum_k V[k ldv + i] y[k] in k order from 0.0, V 8 bytes off a 16-byte boundary, ldv = n, n + 1, n + 7:
    bit-exact on dyadic inputs (all products and sums exact, so the fma chain is the plain chain), within
    n_vec 2^-53 sum_k |V_k y_k| of the longdouble value on general inputs (on the sample of indices at the large n);
    n_vec = 0 writes zeros; out keeps its guard bands."""
    m, lib = madata, ctx.lib
    pV = m["V"].ptr + 8
    for kind in ("dy", "ge"):
        y = m["y"][kind][:n_vec]
        cols = [m[kind].view(0, 37 * k + n)[1][37 * k:] for k in range(n_vec)]
        if kind == "dy":
            # integers below 2^12 times eighths below 2^6: every product is an eighth below 2^18 and every partial sum
            # of 64 of them is exact, so fma(V_k, y_k, acc) == acc + V_k y_k all the way
            assert np.all(np.abs(m["dy"].host) < 2 ** 12) and np.all(m["dy"].host == np.rint(m["dy"].host))
            assert np.all(np.abs(8 * y) < 2 ** 9) and np.all(8 * y == np.rint(8 * y))
            want = np.zeros(n)
            for k in range(n_vec):
                want = want + (exact_products(cols[k], np.full(n, y[k])) if n <= 1024 else cols[k] * y[k])
        else:
            idx = sample_indices(n, red_grid(n, False, EW_CAP) * T)
            ref, mag = np.zeros(len(idx), dtype=np.longdouble), np.zeros(len(idx), dtype=np.longdouble)
            for k in range(n_vec):
                p = cols[k][idx].astype(np.longdouble) * np.longdouble(y[k])
                ref, mag = ref + p, mag + np.abs(p)
        for ldv in (n, n + 1, n + 7):
            for k in range(n_vec):  # column k of V <- the master's slice, device to device
                src = m[kind].vec.ptr + 8 * 37 * k
                assert lib.bis_copy_vector(ctx.h, P(pV + 8 * k * ldv), P(src), I64(n)) == BIS_OK
            go = Guarded(ctx, n, 0)
            ybuf = np.ascontiguousarray(y) if n_vec else None
            st = lib.bis_multi_axpy(ctx.h, P(pV), I64(ldv), ybuf.ctypes if n_vec else None, C.c_int(n_vec), P(go.ptr), I64(n))
            assert st == BIS_OK
            ctx.sync()
            got = go.read()
            go.free()
            if n_vec == 0:
                assert same_bits(got, np.zeros(n))
            elif kind == "dy":
                assert same_bits(got, want), (n, n_vec, ldv)
            else:
                assert np.all(np.abs(got[idx].astype(np.longdouble) - ref) <= n_vec * np.longdouble(U) * mag), (n, n_vec, ldv)


@pytest.mark.gpu
def test_multi_axpy_refuses_65_vectors(ctx, madata):
    n = 257
    go = Guarded(ctx, n, 0)
    y = np.ones(65)
    st = ctx.lib.bis_multi_axpy(ctx.h, P(madata["dy"].vec.ptr), I64(n), y.ctypes, C.c_int(65), P(go.ptr), I64(n))
    assert st == BIS_ERR_INVALID
    ctx.sync()
    assert same_bits(go.read(), np.full(n, SENT))
    go.free()


# ---- 6. scalar kernels -----------------------------------------------------------------------------------------------

SCALAR_TABLE = [3.0, -7.5, 0.1, 1e-3, 2.5e10, 1.0 / 3.0, 0.0, -0.0, math.inf, -math.inf, 5e-324, 2.0 ** -1040, -4.0, 1e308]


@pytest.mark.gpu
def test_scalar_kernels(ctx):
    """bis_scalar_div, bis_scalar_ratio_product, bis_scalar_sqrt_inv: the same IEEE operations as the host's doubles
    (0/x, x/0, 0/0, a negative sum of squares, inf, subnormals among them), nan position by position; out may alias an
    input."""
    lib, sc = ctx.lib, Scalars(ctx)
    f = np.float64
    vals = SCALAR_TABLE
    rng = np.random.default_rng(5)
    with np.errstate(all="ignore"):
        for a in vals:
            for b in vals:
                for alias in (None, 0, 1):
                    sc.put(0, a); sc.put(1, b); sc.put(2, SENT)
                    o = 2 if alias is None else alias
                    assert lib.bis_scalar_div(ctx.h, P(sc.at(o)), P(sc.at(0)), P(sc.at(1))) == BIS_OK
                    ctx.sync()
                    assert same_bits([sc.get(o)], [f(a) / f(b)]), ("div", a, b, alias)
        quads = [tuple(rng.choice(vals, 4)) for _ in range(120)] + [(3.0, 7.0, -2.0, 0.3), (0.0, 0.0, 1.0, 1.0), (1.0, 0.0, 0.0, 1.0)]
        for q, (a, b, c, d) in enumerate(quads):
            o = 4 if q % 5 else q // 5 % 4  # out aliases each input in turn
            for i, v in enumerate((a, b, c, d)):
                sc.put(i, v)
            sc.put(4, SENT)
            assert lib.bis_scalar_ratio_product(ctx.h, P(sc.at(o)), P(sc.at(0)), P(sc.at(1)), P(sc.at(2)), P(sc.at(3))) == BIS_OK
            ctx.sync()
            assert same_bits([sc.get(o)], [(f(a) / f(b)) * (f(c) / f(d))]), ("ratio_product", a, b, c, d, o)
        for a in vals + [2.0, 1e-300, 123456.789]:
            for alias in (False, True):
                sc.put(0, a); sc.put(1, SENT); sc.put(2, SENT)
                assert lib.bis_scalar_sqrt_inv(ctx.h, P(sc.at(0 if alias else 1)), P(sc.at(2)), P(sc.at(0))) == BIS_OK
                ctx.sync()
                nrm = np.sqrt(f(a))
                assert same_bits([sc.get(0 if alias else 1), sc.get(2)], [nrm, f(1.0) / nrm]), ("sqrt_inv", a, alias)
    sc.vec.free()


# ---- 7. argument checks ----------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_argument_checks(ctx):
    """Negative n and null operands with n > 0: BIS_ERR_INVALID; null operands with n == 0: BIS_OK (and a reduction's
    result exactly 0.0); a null scalar pointer of a _dev form, and w == u or w == v in bis_axpy_dot_dev: refused.
    Nothing refused touches its output."""
    lib, h = ctx.lib, ctx.h
    n = 300
    v = ctx.upload(np.arange(3.0 * n))
    p0, p1, p2 = v.ptr, v.ptr + 8 * n, v.ptr + 16 * n
    sc = Scalars(ctx)
    s0, res = sc.at(0), sc.at(1)
    sc.put(0, 0.5)
    one, hostres = C.c_double(1.0), C.c_double(SENT)
    ycoef = np.ones(4)
    calls = {  # name -> call(r, a, b, n)
        "sub": lambda r, a, b, k: lib.bis_subtract_vectors(h, P(r), P(a), P(b), I64(k), one),
        "sum": lambda r, a, b, k: lib.bis_sum_vectors(h, P(r), P(a), P(b), I64(k), one),
        "mult": lambda r, a, b, k: lib.bis_elemwise_mult_vectors(h, P(r), P(a), P(b), I64(k), one),
        "div": lambda r, a, b, k: lib.bis_elemwise_div_vectors(h, P(r), P(a), P(b), I64(k), one),
        "sub_dev": lambda r, a, b, k: lib.bis_subtract_vectors_dev(h, P(r), P(a), P(b), I64(k), P(s0)),
        "sum_dev": lambda r, a, b, k: lib.bis_sum_vectors_dev(h, P(r), P(a), P(b), I64(k), P(s0)),
        "normalize_x": lambda r, a, b, k: lib.bis_normalize_x(h, P(r), P(a), P(b), P(b), I64(k)),
        "dot_dev": lambda r, a, b, k: lib.bis_dot_dev(h, P(a), P(b), I64(k), P(res)),
        "dot": lambda r, a, b, k: lib.bis_dot(h, P(a), P(b), I64(k), C.byref(hostres)),
        "axpy_dot": lambda r, a, b, k: lib.bis_axpy_dot_dev(h, P(r), P(a), P(s0), P(b), I64(k), P(res)),
        "multi_axpy": lambda r, a, b, k: lib.bis_multi_axpy(h, P(a), I64(max(k, 0)), ycoef.ctypes, C.c_int(2 if b else 1), P(r), I64(k)),
    }
    calls2 = {  # name -> call(r, a, n)
        "scale": lambda r, a, k: lib.bis_scale(h, P(r), P(a), one, I64(k)),
        "scale_dev": lambda r, a, k: lib.bis_scale_dev(h, P(r), P(a), P(s0), I64(k)),
        "copy": lambda r, a, k: lib.bis_copy_vector(h, P(r), P(a), I64(k)),
        "sumsq_dev": lambda r, a, k: lib.bis_sumsq_dev(h, P(a), I64(k), P(res)),
        "norm": lambda r, a, k: lib.bis_euclidean_vec_norm(h, P(a), I64(k), C.byref(hostres)),
    }
    for name, f in calls.items():
        assert f(p0, p1, p2, -1) == BIS_ERR_INVALID, name
        for nulls in ((0, p1, p2), (p0, 0, p2), (p0, p1, 0)):
            if name == "axpy_dot" and nulls[2] == 0:
                continue  # v = NULL means (w, w)
            if name in ("dot_dev", "dot") and nulls[0] == 0:
                continue  # (no r)
            if name == "multi_axpy" and nulls[2] == 0:
                continue  # (no b)
            assert f(*nulls, n) == BIS_ERR_INVALID, (name, nulls)
        sc.put(1, SENT)
        assert f(0, 0, 0, 0) == BIS_OK, name
    for name, f in calls2.items():
        assert f(p0, p1, -1) == BIS_ERR_INVALID, name
        assert f(p0, 0, n) == BIS_ERR_INVALID, name
        if name in ("scale", "scale_dev"):
            assert f(0, p1, n) == BIS_ERR_INVALID, name
        assert f(0, 0, 0) == BIS_OK, name
    assert lib.bis_copy_vector(h, None, P(p1), I64(n)) == BIS_ERR_INVALID
    assert lib.bis_init_vector(h, None, one, I64(n)) == BIS_ERR_INVALID and lib.bis_init_vector(h, P(p0), one, I64(-1)) == BIS_ERR_INVALID
    assert lib.bis_init_vector(h, None, one, I64(0)) == BIS_OK
    # n == 0 with null operands: the reductions give exactly +0.0
    for f in (lambda: lib.bis_dot_dev(h, None, None, I64(0), P(res)), lambda: lib.bis_sumsq_dev(h, None, I64(0), P(res)),
              lambda: lib.bis_axpy_dot_dev(h, None, None, P(s0), None, I64(0), P(res))):
        sc.put(1, SENT)
        assert f() == BIS_OK
        ctx.sync()
        assert sc.get(1) == 0.0 and math.copysign(1.0, sc.get(1)) == 1.0
    hostres.value = SENT
    assert lib.bis_dot(h, None, None, I64(0), C.byref(hostres)) == BIS_OK and hostres.value == 0.0
    hostres.value = SENT
    assert lib.bis_euclidean_vec_norm(h, None, I64(0), C.byref(hostres)) == BIS_OK and hostres.value == 0.0
    # null scalars / results
    assert lib.bis_subtract_vectors_dev(h, P(p0), P(p1), P(p2), I64(n), None) == BIS_ERR_INVALID
    assert lib.bis_sum_vectors_dev(h, P(p0), P(p1), P(p2), I64(n), None) == BIS_ERR_INVALID
    assert lib.bis_scale_dev(h, P(p0), P(p1), None, I64(n)) == BIS_ERR_INVALID
    assert lib.bis_axpy_dot_dev(h, P(p0), P(p1), None, P(p2), I64(n), P(res)) == BIS_ERR_INVALID
    assert lib.bis_axpy_dot_dev(h, P(p0), P(p1), P(s0), P(p2), I64(n), None) == BIS_ERR_INVALID
    assert lib.bis_dot_dev(h, P(p0), P(p1), I64(n), None) == BIS_ERR_INVALID
    assert lib.bis_sumsq_dev(h, P(p0), I64(n), None) == BIS_ERR_INVALID
    assert lib.bis_dot(h, P(p0), P(p1), I64(n), None) == BIS_ERR_INVALID
    for args in ((None, P(s0), P(s0)), (P(res), None, P(s0)), (P(res), P(s0), None)):
        assert lib.bis_scalar_div(h, *args) == BIS_ERR_INVALID
    for k in range(5):
        args = [P(res), P(s0), P(s0), P(s0), P(s0)]
        args[k] = None
        assert lib.bis_scalar_ratio_product(h, *args) == BIS_ERR_INVALID
    for k in range(3):
        args = [P(res), P(sc.at(2)), P(s0)]
        args[k] = None
        assert lib.bis_scalar_sqrt_inv(h, *args) == BIS_ERR_INVALID
    # aliasing the fused kernel cannot honour
    assert lib.bis_axpy_dot_dev(h, P(p0), P(p0), P(s0), P(p2), I64(n), P(res)) == BIS_ERR_INVALID
    assert lib.bis_axpy_dot_dev(h, P(p0), P(p1), P(s0), P(p0), I64(n), P(res)) == BIS_ERR_INVALID
    ctx.sync()
    assert np.array_equal(v.to_host(), np.arange(3.0 * n))  # no refused call wrote anything
    v.free(); sc.vec.free()


# ---- 8. the shared-dot promise past the cap ------------------------------------------------------------------------

JACOBI_N = C2 + 3
JACOBI_ITERS = 24


@pytest.fixture(scope="module")
def tridiag(ctx):
    """A diagonally dominant tridiagonal matrix of JACOBI_N rows (odd, second trip of the double2 reduction), from CRS."""
    from oracle.pyoracle import CRS
    n = JACOBI_N
    rng = np.random.default_rng(20260404)
    diag, lo, up = rng.uniform(4.0, 5.0, n), -rng.uniform(0.5, 1.0, n), -rng.uniform(0.5, 1.0, n)
    cols = np.arange(n)[:, None] + np.array([-1, 0, 1])[None, :]
    vals = np.stack([lo, diag, up], axis=1)
    keep = (cols >= 0) & (cols < n)
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    A = CRS(n, rp, cols[keep].astype(np.int32), vals[keep])
    dA = ctx.matrix(A)
    yield dict(dA=dA, D=diag, b=rng.uniform(-1, 1, n), x0=0.1 * rng.uniform(-1, 1, n))
    dA.free()


@pytest.mark.gpu
@pytest.mark.parametrize("off8", [0, 1])
def test_jacobi_schedule_shares_the_dot_past_the_cap(ctx, tridiag, off8):
    """Jacobi iterations at n = 2 * 256 * 8192 + 3: the bis_stat_* history and iterate are bit-identical to the
    kernel-by-kernel schedule (spmv, normalize_x, compute_residual, euclidean_vec_norm) -- jacobi_step_kernel forms the
    residual norm with dot_partial_kernel's index map and grid.  off8: b, x and D 8 bytes off a 16-byte boundary; the
    schedule's residual vector stays the aligned allocation it is, so its norm is the double2 form's still (a step
    kernel that let the alignment of b, D or x choose the index map of that norm is what this case caught).
    JACOBI_ITERS iterations, not the three that would do in principle: two orders of one sum of 4 M squares agree in
    most of their bits, and the square root hides half of the last-bit differences that are left, so three norms
    coincide by chance too often for the test to bite."""
    n, dA = JACOBI_N, tridiag["dA"]
    pad = lambda v: np.concatenate([np.zeros(off8), v])
    bufs = [ctx.upload(pad(tridiag[k])) for k in ("b", "D", "x0", "x0")]
    b, D, x, y = (v.offset(off8, n) for v in bufs)
    assert b.ptr % 16 == 8 * off8
    xn, t, r = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
    ctx.compute_residual(dA, x, b, r, t)
    hist = [ctx.euclidean_vec_norm(r)]
    for _ in range(JACOBI_ITERS):
        ctx.spmv(dA, x, xn)
        ctx.normalize_x(xn, x, D, b)
        x, xn = xn, x
        ctx.compute_residual(dA, x, b, r, t)
        hist.append(ctx.euclidean_vec_norm(r))
    x_sep = x.to_host()
    st = ctx.stat("j", dA, D, b, y)
    r0 = st.init(1e-300)
    st.iterate(JACOBI_ITERS)
    iters, conv, h2 = st.status(hist_cap=64)
    out = ctx.alloc(n)
    st.solution(out)
    got = out.to_host()
    st.free()
    for v in bufs + [xn if xn.owner else x, t, r, out]:
        v.free()
    assert iters == JACOBI_ITERS and not conv and r0 == hist[0]
    assert np.all(np.diff(hist) < 0) and np.isfinite(hist[0]) and hist[-1] > 0
    assert np.array_equal(h2, np.array(hist)), (list(h2), hist)
    assert np.array_equal(got, x_sep)
