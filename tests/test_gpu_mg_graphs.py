"""GPU: the multigrid setup and cycle on the adversarial inputs of tests/mg_graphs.py: 8 MIS levels, a row of 1200
neighbours beside rows of three, aggregates of hundreds of members, a dense coarse row that sends the Galerkin product of
smoothed aggregation to spgemm_sort_fallback, components, rows with shuffled columns, stored zeros off the diagonal, MIS
over about 118 workgroups, both sides of the 0.8 drop rule, and hierarchies of exactly 16 levels.  test_mg_graphs_cpu.py
shows without a device that the inputs are that.

Reference: the numpy restatements of test_gpu_mg.py (hierarchy_reference, cycle_reference), spgemm_ref.py (hierarchy,
cycle) and test_gpu_mg_cycle.py (W and K transitions), computed once per input (mg_graphs.reference) and shared.
Setup is held to "the same bits".  The cycle is held to 1e-13 |ref|_inf, the project's kernel gate (CYCLE_GATES).

Out of scope: the grid-stride wrap past 16384 workgroups (mg_grid) needs more than 4 M rows, where the Python MIS
restatement is too slow."""
import ctypes as C

import numpy as np
import pytest

import mg_graphs as g
import spgemm_ref as ref
import test_gpu_mg as base
import test_gpu_mg_cycle as cyc
import test_gpu_mg_smoothed as sm
from helpers import OptionScope

pytestmark = pytest.mark.gpu
GATE = base.GATE
UNSUPPORTED = 6
SORT, BOTH = "spgemm_sort_fallback", "spgemm_row_kernel + spgemm_sort_fallback"
same_bits, apply_host = base.same_bits, base.apply_host

# The cycle gate per (case, smoothed).  The rule: the host-only gap between the restated cycle with longdouble row sums
# (the reference here) and the same cycle with fp64 row sums in CRS order, as test_mg_graphs_cpu.py measures and prints it;
# a case whose gap is at most GATE / 4 = 2.5e-14 uses GATE, any other 4 x its gap.  Measured (fractions of |ref|_inf):
# hub 1.2e-16 plain and 6.9e-17 smoothed (rows of 1203 and 732 entries), hub5000 4.9e-17 (3002 entries), clique300 1.4e-16
# and 1.5e-16, path5000 1.0e-16 and 1.6e-16, chain16 5.1e-17, chain16_exact 3.8e-17, components 7.6e-18 and 3.3e-17, every
# other case below 1e-17 (shuffled and shuffled_ties 5.6e-20 and 2.8e-20: their |ref|_inf is that of the rows that hold only
# the diagonal 1e-3).  The largest is 1.6e-16: no case needs a gate of its own, and the CPU test fails if one ever does.
CYCLE_GATES = {(name, smoothed): GATE for name in g.CASES for smoothed in ((False, True) if g.CASES[name].smoothed else (False,))}
PLAIN = list(g.CASES)
BOTH_KINDS = sorted(CYCLE_GATES, key=lambda k: (k[1], PLAIN.index(k[0])))
IDS = [f"{name}-{'smoothed' if s else 'plain'}" for name, s in BOTH_KINDS]


@pytest.fixture(scope="module")
def ctx():
    from basic_iterative_solvers_amd import Context
    c = Context()
    assert c.device_info()["arch"].startswith("gfx950")
    yield c
    c.close()


def upload(ctx, name):
    c = g.CASES[name]
    dA = ctx.matrix(c.A)
    if c.grid is not None:
        dA.set_grid_hint(*c.grid)
    return dA


@pytest.fixture(scope="module")
def built(ctx):
    """One setup per (case, smoothed), left alone: the device matrix (one per case), the hierarchy and its download."""
    mats, cache = {}, {}

    def get(name, smoothed=False):
        if (name, smoothed) not in cache:
            if name not in mats:
                mats[name] = upload(ctx, name)
            mg = ctx.mg(mats[name], smooth=smoothed, **g.CASES[name].params)
            cache[(name, smoothed)] = dict(dA=mats[name], mg=mg, dev=sm.downloaded(mg) if smoothed else base.downloaded(mg))
        return cache[(name, smoothed)]
    return get


def rhs(n):
    return np.random.default_rng(11).uniform(-1, 1, n)


def check_invariants_on_every_mis_level(dev, want, tag):
    checked = 0
    for l, (d, r) in enumerate(zip(dev[:-1], want[:-1])):
        if d["kind"] == 2:
            # (the level matrix is the restatement's bit for bit: compare_hierarchies has run; so are the restatement's roots)
            base.check_mis_invariants(d["A"], d["agg"], r["root"])
            checked += 1
    return checked


# ---- setup -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PLAIN)
def test_unsmoothed_hierarchy_has_the_restatements_bits(built, name):
    e = built(name)
    dev, want = e["dev"], g.reference(name)
    print(f"{name}: rows {[L['A'].n_rows for L in dev]}, kinds {[L['kind'] for L in dev]}, nnz {[L['A'].nnz for L in dev]}")
    base.compare_hierarchies(dev, want, name)
    mis = g.CASES[name].grid is None
    assert [L["kind"] for L in dev] == [2 if mis else 1] * (len(dev) - 1) + [0]
    assert check_invariants_on_every_mis_level(dev, want, name) == (len(dev) - 1 if mis else 0)
    assert e["mg"].rows == [L["A"].n_rows for L in want] and not e["mg"].smoothed


@pytest.mark.parametrize("name", g.SMOOTHED)
def test_smoothed_hierarchy_has_the_restatements_bits(built, name):
    """omega_l, P, R and the level operators.  On the hub the product R (A P) of level 1 has a row of 773678 products (the CPU
    test shows it past row_cap_max = 4096): the level matrix reports a fallback path through Mat.spgemm_kernel()."""
    e = built(name, True)
    dev, want = e["dev"], g.reference(name, True)
    print(f"{name}: rows {[L['A'].n_rows for L in dev]}, nnz {[L['A'].nnz for L in dev]}, omega_l {[L['omega_l'] for L in dev[:-1]]}, "
          f"nnz(P) {[L['P'].nnz for L in dev[:-1]]}, paths {[e['mg'].level_matrix(l).spgemm_kernel() for l in range(1, len(dev))]}")
    sm.compare_smoothed(dev, want, name)
    assert [L["kind"] for L in dev] == [2] * (len(dev) - 1) + [0] and e["mg"].smoothed
    assert check_invariants_on_every_mis_level(dev, want, name) == len(dev) - 1
    if name == "hub":
        assert len(dev) >= 2 and e["mg"].level_matrix(1).spgemm_kernel() in (SORT, BOTH)
        assert int(np.diff(dev[1]["A"].row_ptr).max()) == dev[1]["A"].n_rows  # the dense coarse row


def test_both_sides_of_the_drop_rule(built):
    for smoothed in (False, True):
        keep, drop = built("boundary_keep", smoothed)["mg"], built("boundary_drop", smoothed)["mg"]
        assert keep.rows == [500, 400] and keep.kinds == [2, 0], (smoothed, keep.rows, keep.kinds)  # 5 * 400 == 4 * 500: kept
        assert drop.levels == 1 and drop.rows == [501] and drop.kinds == [0], (smoothed, drop.rows)  # 5 * 401 > 4 * 501


def test_sixteen_levels(built):
    e = built("chain16")
    mg, want = e["mg"], g.reference("chain16")
    assert mg.levels == 16 and mg.rows == [L["A"].n_rows for L in want] == [1 << k for k in range(16, 0, -1)]
    assert mg.kinds == [1] * 15 + [0]
    assert [L["grid"] for L in e["dev"]] == [(n, 1, 1, 1) for n in mg.rows]
    exact = built("chain16_exact")["mg"]
    assert exact.levels == 16 and exact.rows[-1] == 1 and exact.rows == [1 << k for k in range(15, -1, -1)]


@pytest.mark.parametrize("name,smoothed", [("hub", False), ("hub", True), ("wide30000", False)], ids=["hub", "hub-smoothed", "wide30000"])
def test_two_setups_give_the_same_bits(ctx, built, name, smoothed):
    e = built(name, smoothed)
    mg2 = ctx.mg(e["dA"], smooth=smoothed, **g.CASES[name].params)
    if smoothed:
        sm.compare_smoothed(sm.downloaded(mg2), e["dev"], name + " again")
    else:
        base.compare_hierarchies(base.downloaded(mg2), e["dev"], name + " again")
    mg2.free()


@pytest.mark.parametrize("smoothed", [False, True], ids=["plain", "smoothed"])
def test_hub_with_64_bit_row_pointers(ctx, built, smoothed):
    e = built("hub", smoothed)
    with OptionScope(ctx, force_rp64=1):
        dA = upload(ctx, "hub")
        assert dA.rp_width == 8
        mg = ctx.mg(dA, smooth=smoothed, **g.CASES["hub"].params)
        wide = sm.downloaded(mg) if smoothed else base.downloaded(mg)
    assert all(L["rp_width"] == 8 for L in wide) and all(L["rp_width"] == 4 for L in e["dev"])
    if smoothed:  # (the row-pointer width changes nothing else)
        assert all(L["transfer_rp_width"] == (8, 8) for L in wide[:-1])
        sm.compare_smoothed(wide, e["dev"], "hub rp64")
    else:
        base.compare_hierarchies(wide, e["dev"], "hub rp64")
    mg.free()
    dA.free()


def test_a_repeated_entry_is_refused(ctx):
    D, _ = g.shuffled_with_duplicate()
    dD = ctx.matrix(D)
    st, out = base.raw_create(ctx, dD.h, coarse_limit=30)
    assert st == UNSUPPORTED and not out
    dD.free()


# ---- the cycle -----------------------------------------------------------------------------------------------------------

def restated(levels, v, smoothed, **cfg):
    return ref.cycle(levels, v, ref.config(**cfg)) if smoothed else cyc.cycle_reference(levels, v, cyc.config(**cfg))


def deviation(out, want):
    assert np.all(np.isfinite(want))
    return np.max(np.abs(out - want)) / np.max(np.abs(want))


@pytest.mark.parametrize("name,smoothed", BOTH_KINDS, ids=IDS)
def test_v_cycle_against_the_restatement(ctx, built, name, smoothed):
    e = built(name, smoothed)
    levels = e["dev"]
    v = rhs(levels[0]["A"].n_rows)
    want = restated(levels, v, smoothed)
    if not smoothed:
        assert same_bits(want, base.cycle_reference(levels, v))
    out = apply_host(ctx, e["mg"], v)
    dev = deviation(out, want)
    print(f"{name} {'smoothed' if smoothed else 'plain'}: {len(levels)} levels, |dev - ref|_inf / |ref|_inf = {dev:.3e}")
    assert dev <= CYCLE_GATES[(name, smoothed)]
    assert same_bits(apply_host(ctx, e["mg"], v), out), "two applies differ"
    assert same_bits(apply_host(ctx, e["mg"], v, alias=True), out), "out aliasing in differs"
    assert same_bits(apply_host(ctx, e["mg"], v, through_dispatcher=True), out), "type 10 differs from bis_mg_apply"
    assert same_bits(apply_host(ctx, e["mg"], v, alias=True, through_dispatcher=True), out)


@pytest.mark.parametrize("name,smoothed", [("hub", False), ("hub", True), ("clique300", False), ("clique300", True)],
                         ids=["hub-plain", "hub-smoothed", "clique300-plain", "clique300-smoothed"])
def test_k_cycle_against_the_restatement(ctx, built, name, smoothed):
    e = built(name, smoothed)
    levels = e["dev"]
    assert len(levels) >= 3  # (a K transition needs a level below its coarse level)
    v = rhs(levels[0]["A"].n_rows)
    mg = ctx.mg(e["dA"], smooth=smoothed, cycle=cyc.K, **g.CASES[name].params)
    want = restated(levels, v, smoothed, cycle=cyc.K)
    out = apply_host(ctx, mg, v)
    dev = deviation(out, want)
    print(f"{name} {'smoothed' if smoothed else 'plain'} K: |dev - ref|_inf / |ref|_inf = {dev:.3e}")
    assert dev <= CYCLE_GATES[(name, smoothed)]
    assert not same_bits(want, restated(levels, v, smoothed)), "the cycle is V's"
    mg.free()


@pytest.mark.parametrize("smoothed", [False, True], ids=["plain", "smoothed"])
def test_two_sweeps_on_shuffled_rows(ctx, built, smoothed):
    e = built("shuffled", smoothed)
    levels = e["dev"]
    v = rhs(levels[0]["A"].n_rows)
    mg = ctx.mg(e["dA"], smooth=smoothed, nu=2, coarse_scale=1.5, **g.CASES["shuffled"].params)
    want = restated(levels, v, smoothed, nu=2, coarse_scale=1.5)
    dev = deviation(apply_host(ctx, mg, v), want)
    print(f"shuffled {'smoothed' if smoothed else 'plain'} nu 2 scale 1.5: |dev - ref|_inf / |ref|_inf = {dev:.3e}")
    assert dev <= CYCLE_GATES[("shuffled", smoothed)]
    mg.free()


def test_w_on_the_first_three_transitions_of_sixteen_levels(ctx, built):
    """Three W transitions: 8 visits of level 3 and of everything below it (a W-cycle on all 16 levels would visit the
    coarsest 2^15 times)."""
    e = built("chain16")
    levels = e["dev"]
    v = rhs(levels[0]["A"].n_rows)
    mg = ctx.mg(e["dA"], cycle=cyc.W, cycle_levels=3, **g.CASES["chain16"].params)
    assert mg.cycle == (cyc.W, 3) and mg.levels == 16
    want = restated(levels, v, False, cycle=cyc.W, cycle_levels=3)
    out = apply_host(ctx, mg, v)
    dev = deviation(out, want)
    print(f"chain16 W on 3 transitions: |dev - ref|_inf / |ref|_inf = {dev:.3e}")
    assert dev <= CYCLE_GATES[("chain16", False)]
    assert not same_bits(want, restated(levels, v, False))
    assert same_bits(apply_host(ctx, mg, v), out)
    mg.free()
