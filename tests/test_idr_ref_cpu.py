"""CPU: the numpy restatement of IDR(s) that the device schedule bis_idr_* is tested against (tests/idr_ref.py) solves the
GPU tests' inputs, its two forms of the biorthogonalisation agree, it moves by rounding-level amounts only when its dots
are rounded differently, and the hashed shadow space is the header's formula."""
import numpy as np
import pytest

from idr_ref import hashed_shadow, idr
from test_gpu_idr import SS, TOL, host_matrix, host_spmv, right_hand_side

ITERS = 2000
INPUTS = ["band37", "band600", "cd10", "band40k", "unstr8", "one"]


@pytest.fixture(scope="module")
def systems(oracle):
    out = {}
    for name in INPUTS:
        A = oracle.gen_unstr(8, 8, 8) if name == "unstr8" else host_matrix(name)
        b, x0 = right_hand_side(A.n_rows)
        out[name] = dict(A=A, b=b, x0=x0, mul=lambda v, A=A: host_spmv(A, v), runs={})
    return out


def run(e, s, **kw):
    key = (s, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in e["runs"]:
        e["runs"][key] = idr(e["mul"], e["b"], e["x0"], s, TOL, ITERS, **kw)
    return e["runs"][key]


@pytest.mark.parametrize("s", SS)
@pytest.mark.parametrize("name", INPUTS)
def test_the_restatement_solves_the_inputs(systems, name, s):
    e = systems[name]
    g = run(e, s)
    res = float(np.linalg.norm(e["b"] - e["mul"](g["x"])))
    print(f"{name} s={s}: {g['iters']} iterations, true residual {res / g['hist'][0]:.3e} r0, last entry {g['hist'][-1] / g['hist'][0]:.3e} r0")
    assert g["conv"] and res < 10.0 * TOL * g["hist"][0]


@pytest.mark.parametrize("s", SS)
@pytest.mark.parametrize("name", INPUTS)
def test_one_multi_dot_and_the_published_loop_agree(systems, name, s):
    e = systems[name]
    a, b = run(e, s), run(e, s, sequential=True)
    print(f"{name} s={s}: one multi-dot {a['iters']} iterations, published loop {b['iters']}")
    assert a["conv"] and b["conv"] and abs(a["iters"] - b["iters"]) <= 3


@pytest.mark.parametrize("s", SS)
@pytest.mark.parametrize("name", INPUTS)
def test_differently_rounded_dots_move_the_history_by_rounding_only(systems, name, s):
    """What the GPU tests' gate rests on: fp64 against longdouble accumulation of every dot."""
    e = systems[name]
    a, b = run(e, s), run(e, s, acc=np.longdouble)
    n = min(len(a["hist"]), len(b["hist"]))
    whole = float(np.max(np.abs(a["hist"][:n] - b["hist"][:n])) / a["hist"][0])
    first = float(np.max(np.abs(a["hist"][:3] - b["hist"][:3])) / a["hist"][0])
    print(f"{name} s={s}: {a['iters']} / {b['iters']} iterations, whole history apart {whole:.3e} r0, first three entries {first:.3e} r0")
    assert whole <= 1e-4 and first <= 1e-10 and abs(a["iters"] - b["iters"]) <= 3


def test_hashed_shadow_is_the_formula():
    def hash32(x):
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xffffffff
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xffffffff
        x ^= x >> 16
        return x

    n, s = 300, 8
    P = hashed_shadow(n, s)
    for i in list(range(20)) + [n - 1]:
        for j in range(s):
            h = hash32(hash32(i) ^ (((j + 1) * 0x9e3779b9) % 2 ** 32))
            assert P[i, j] == (h + 0.5) * 2.0 ** -31 - 1.0
    assert np.all(np.abs(P) < 1.0) and abs(P.mean()) < 0.05
    assert np.linalg.matrix_rank(P) == s
