"""tspgemm.epilogue_ref, the numpy statement of the fused epilogue's contract
(include/ternary_spgemm.h tcsc_hip_gemm_dev_ex), against an independent
evaluation -- a per-element Python loop on np.float32 scalars -- and on the
special values; then the case builder of test_gpu_epilogue.py without a GPU:
every case that file runs builds, which asserts its input conditions (the
expectation told apart from a fused multiply-add, from the add before the
multiply and from a 16-bit a; RELU and RELU2 told apart from NONE; everything
finite, also in the Y type)."""
import numpy as np
import pytest

import test_gpu_epilogue as G


@pytest.fixture(autouse=True)
def _oracle_built(oracle_mod):
    """The case builder imports the oracle itself: it is built first."""


def _loop(y, act, alpha, mul, add):
    """One element at a time, every operation on np.float32 scalars."""
    f = np.float32
    out = np.empty_like(y)
    with np.errstate(all="ignore"):
        for m in range(y.shape[0]):
            for n in range(y.shape[1]):
                v = f(y[m, n])
                if act == "prelu":
                    a = v if v > 0 else f(f(alpha[n]) * v)
                elif act in ("relu", "relu2"):
                    a = v if v > 0 else (v if v != v else f(0.0))
                    if act == "relu2":
                        a = f(a * a)
                else:
                    a = v
                if mul is not None:
                    a = f(a * f(mul[m, n]))
                if add is not None:
                    a = f(a + f(add[m, n]))
                out[m, n] = a
    return out


@pytest.mark.parametrize("act", G.ACTS)
@pytest.mark.parametrize("ops", ["mul", "add", "both", "neither"])
def test_epilogue_ref_is_the_scalar_loop(tsg, act, ops):
    rng = np.random.default_rng(G.ACTS.index(act) * 4 + len(ops))
    M, N = 7, 13
    y = (rng.uniform(0.5, 2.0, (M, N)) * rng.choice([-1.0, 1.0], (M, N)) * 32).astype(np.float32)
    y[0, :4] = (0.0, -0.0, np.inf, -np.inf)
    y[1, 0] = np.nan
    y[2, :2] = (1e30, -1e30)
    alpha = rng.uniform(-0.5, 0.5, N).astype(np.float32)
    mul = rng.uniform(-2.0, 2.0, (M, N)).astype(np.float32) if ops in ("mul", "both") else None
    add = rng.uniform(-64.0, 64.0, (M, N)).astype(np.float32) if ops in ("add", "both") else None
    got = tsg.epilogue_ref(y, act, alpha if act == "prelu" else None, mul, add)
    want = _loop(y, act, alpha, mul, add)
    assert got.dtype == np.float32 and got.shape == y.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def test_epilogue_ref_special_values(tsg):
    f = np.float32
    bits = lambda a: np.asarray(a, f).view(np.uint32)
    y = np.array([[-0.0, 0.0, np.nan, -3.0, 3.0, 2e19, -np.inf, np.inf]], f)
    r = tsg.epilogue_ref(y, "relu")
    assert np.array_equal(bits(r[0, :2]), bits([0.0, 0.0])), "relu(-0) is not +0"
    assert np.isnan(r[0, 2]) and r[0, 3] == 0 and not np.signbit(r[0, 3]) and r[0, 4] == 3
    assert r[0, 6] == 0 and np.isinf(r[0, 7])
    r2 = tsg.epilogue_ref(y, "relu2")
    assert np.isnan(r2[0, 2]) and r2[0, 4] == 9 and np.isposinf(r2[0, 5]), "relu2 does not overflow to +inf"
    assert np.array_equal(bits(r2[0, :2]), bits([0.0, 0.0]))
    # 0 * inf is NaN; inf + -inf is NaN
    g = np.full_like(y, np.inf)
    assert np.isnan(tsg.epilogue_ref(y, "relu", None, g)[0, 0])
    assert np.isnan(tsg.epilogue_ref(y, "none", None, None, np.full_like(y, -np.inf))[0, 7])
    # a None operand is not an operation: -0 survives where * 1 + 0 would not keep it
    n = tsg.epilogue_ref(y, "none")
    assert np.array_equal(bits(n)[~np.isnan(y)], bits(y)[~np.isnan(y)])
    one, zero = np.ones_like(y), np.zeros_like(y)
    assert bits(tsg.epilogue_ref(y, "none", None, one, zero))[0, 0] != bits(y)[0, 0]
    # PReLU is the other calls' rule
    alpha = np.full(8, 0.25, f)
    p = tsg.epilogue_ref(y, "prelu", alpha)
    assert p[0, 3] == f(-0.75) and p[0, 4] == 3
    # the multiply and the add are two roundings
    a = np.array([[1.0 + 2.0 ** -23]], f)
    m = np.array([[1.0 + 2.0 ** -23]], f)
    c = np.array([[-(1.0 + 2.0 ** -22)]], f)  # the rounded product: two roundings give 0, one gives 2^-46
    two = tsg.epilogue_ref(a, "none", None, m, c)
    fused = f(np.float64(a[0, 0]) * np.float64(m[0, 0]) + np.float64(c[0, 0]))
    assert two[0, 0] == 0 and fused == f(2.0 ** -46)
    for bad in (dict(y32=y.astype(np.float64), act="none"), dict(y32=y, act="silu"), dict(y32=y, act="prelu"),
                dict(y32=y, act="none", mul=np.ones((2, 8), f))):
        with pytest.raises(Exception):
            tsg.epilogue_ref(**bad)


BUILDS = G.all_builds()


@pytest.mark.parametrize("i", range(len(BUILDS)), ids=lambda i: "-".join(str(x) for x in BUILDS[i][1:]) + f"-{BUILDS[i][0][:3]}")
def test_gpu_case_builds(tsg, i):
    """expect() asserts the input conditions; here the shapes and types."""
    key, act, mt, at, yd = BUILDS[i]
    ex = G.expect(key, act, mt, at, yd)
    M, N = key[0], key[2]
    assert ex.bits.shape == (M, N) and ex.bits.dtype == (np.uint32 if yd == "float32" else np.uint16)
    assert (ex.Gt is None) == (mt is None) and (ex.Rt is None) == (at is None)
    if mt:
        assert str(ex.Gt.dtype) == "torch." + mt and tuple(ex.Gt.shape) == (M, N)
    if at:
        assert str(ex.Rt.dtype) == "torch." + at
        # the operand types show: R in its type is not R in the others
        assert float(np.abs(ex.Rw).max()) >= 1.0


@pytest.mark.parametrize("c", G.drawn_cases(), ids=G.draw_id)
def test_drawn_case_builds(tsg, c):
    ex = G.build_draw(c)
    assert ex.bits.shape == (c.M, c.N)
    if G.FAMILIES[c.family][0] == "pc":  # the one family whose kernel is the planner's own pick
        arrays = G.ecase(*G.draw_key(c)).arrays
        plan = tsg.call_plan(c.K, c.N, int(arrays[0][-1] + arrays[1][-1]), c.M)
        assert plan["kernel"] == G.KERNEL["pc"], (c, plan)


def test_drawn_list_is_deterministic_and_covers(tsg):
    assert tsg.tsg_gemm_ex and tsg.epilogue_ref  # (the draw is of calls of the descriptor)
    G.drawn_cases.cache_clear()
    a = G.drawn_cases()
    G.drawn_cases.cache_clear()
    assert a == G.drawn_cases() and len(a) == G.DRAWS
    assert {c.family for c in a} == set(G.FAMILIES)
    for name, fam in G.FAMILIES.items():  # several shapes per family, none of them the family's own
        shapes = {(c.M, c.K, c.N) for c in a if c.family == name}
        assert len(shapes) >= 3 and fam[1:4] not in shapes, (name, shapes)
        assert all(c.K >= fam[6] for c in a if c.family == name)
    assert len({c.N % 8 for c in a}) == 8 and any(c.N < 64 for c in a) and any(c.N > 512 for c in a)
    assert any(c.act == "prelu" for c in a if c.family == "blocked") or \
        ("prelu", "float32", "float32") in G.family_combos("blocked", "float32")
    assert {c.act for c in a} == set(G.ACTS) and {c.ydtype for c in a} == set(G.YDTYPES)
    assert {c.multype for c in a} == {None, *G.YDTYPES} == {c.addtype for c in a}


@pytest.mark.parametrize("ydtype", ["float32", "bfloat16"])
def test_other_builders(tsg, ydtype):
    """The in-place, alignment, graph, special and FFN builders."""
    other = "float16" if ydtype == "float32" else "float32"
    for name in ("walk-m16", "rows64-w128", "rx", "pc-m1", "rows128-w64"):
        G.expect(G.family_key(name), "relu2", other, ydtype, ydtype)
        G.expect(G.family_key(name), "relu2", ydtype, other, ydtype)
    for fam, M, K, N, width in G.ALIGN.values():
        for op in G.YDTYPES:
            G.expect((M, K, N, "float32", 0, op != "float32"), "relu2", op, op, op)
    for name in ("rows64-w16", "walk-m16"):
        for seed in (0, 1):
            G.expect(G.family_key(name, "bfloat16"), "relu2", "float16", "bfloat16", "bfloat16", seed)
    G.special_case()
    c = G.ffn_case()
    assert c.h_bits.shape == (33, 256)
