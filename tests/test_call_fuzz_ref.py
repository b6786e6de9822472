"""The case list of test_gpu_call_fuzz.py without a GPU: every case builds (the
input conditions of that file's module docstring hold -- edge dependence, a
finite expectation in the Y type, an all-zero W giving b, an empty column
where s = 64 asks for one), the list is deterministic and complete, it covers
what it claims to cover (computed from the tuples and printed once: run with
-s), and where a case leaves the kernel to the planner, tsg_call_plan names
the kernel the case expects -- a change of the planner's rules shows here
first."""
import collections

import numpy as np
import pytest

import test_gpu_call_fuzz as G


@pytest.fixture(autouse=True)
def _oracle_built(oracle_mod):
    """The case builder imports the oracle itself: it is built first."""


@pytest.mark.parametrize("c", G.cases(), ids=G.case_id)
def test_case_builds(tsg, c):
    """build() asserts the input conditions; here the shapes and types of what it returns."""
    bc = G.build(c)
    assert str(bc.Xt.dtype) == "torch." + c.xdtype and tuple(bc.Xt.shape) == (c.M, c.K)
    want_dtype = np.uint32 if c.ydtype == "float32" else np.uint16
    assert set(bc.want) == {"plain", "prelu"}
    assert all(w.shape == (c.M, c.N) and w.dtype == want_dtype for w in bc.want.values())
    assert (bc.deq is not None) == (c.kind in G.QUANT) and (bc.g is not None) == (c.gamma != "none")
    assert (bc.rs is not None) == c.rs and (bc.cs is not None) == c.cs
    if c.prelu:
        assert not np.array_equal(bc.want["plain"], bc.want["prelu"]), (c, "the PReLU does not show")


def test_case_list_is_deterministic_and_complete():
    counter = []
    again = tuple(G.directed_cases() + G.drawn_cases(counter))
    assert again == G.cases() and all(type(a) is G.Case for a in again)
    drawn = [c for c in G.cases() if c.name == "drawn"]
    assert len(counter) == len(drawn) == G.PER_PAIR * len(G.PAIRS)
    assert len(G.cases()) == len(counter) + len(G.directed_cases())
    assert len({c.seed for c in G.cases()}) == len(G.cases()) == len({G.case_id(c) for c in G.cases()})


def _chunked(c):
    """K above the chunk of the walk's tile (tsg_internal.h kEllMaxC, restated in G.ELL_MAX_C)."""
    return c.family == "walk" and c.K > G.ELL_MAX_C[G.walk_tile(c.M, c.K)]


def test_coverage():
    cs = G.cases()
    per_pair = collections.Counter((c.kind, c.family) for c in cs)
    narrow = [c for c in cs if c.ydtype != "float32"]
    table = [f"cases: {len(cs)} = {len(G.directed_cases())} directed + {sum(c.name == 'drawn' for c in cs)} drawn",
             "kind       " + " ".join(f"{f:>8}" for f in G.FAMILIES) + "  chunked  N<8,16-bit"]
    for k in G.KINDS:
        table.append(f"{k:<10} " + " ".join(f"{per_pair[(k, f)]:>8}" for f in G.FAMILIES) +
                     f"  {sum(_chunked(c) and c.kind == k for c in cs):>7}"
                     f"  {sum(c.N < 8 and c.kind == k for c in narrow):>10}")
    groups = collections.Counter(c.name for c in cs)
    table.append("groups: " + ", ".join(f"{n} {v}" for n, v in groups.items()))
    print("\n" + "\n".join(table))
    assert set(per_pair) == set(G.PAIRS) and min(per_pair.values()) >= 4, per_pair
    for k in G.KINDS:
        mine = [c for c in cs if c.kind == k]
        assert sum(_chunked(c) for c in mine) >= 2, (k, "chunked walk")
        assert sum(c.N < 8 and c.ydtype != "float32" for c in mine) >= 2, (k, "N < 8 with a 16-bit Y")
        missing = {(x, y) for x in G.xdtypes_of(k) for y in G.YDTYPES} - {(c.xdtype, c.ydtype) for c in mine}
        assert not missing, (k, "X and Y type pairs not run", missing)
    for x in G.XDTYPES:
        assert {c.xoff for c in cs if c.xdtype == x} == {0, 1, 2, 3}, (x, "X offsets")
    for y in G.YDTYPES:
        assert {c.c0 for c in cs if c.ydtype == y} == set(G.C0S), (y, "column offsets")
        assert {c.pad for c in cs if c.ydtype == y} == set(G.PADS), (y, "pads")
    # what the directed groups promise
    assert {c.s for c in cs if c.name == "unusual-w"} == {1, 4, 64} and any(c.w == "zero" for c in cs)
    assert {c.K for c in cs if c.name == "tiny-k"} == {1, 2, 3, 4, 5}
    assert all(c.knob is None for c in cs if c.name == "row-layout-chunk-edge")
    assert {c.knob for c in cs if c.family == "rows64"} >= {None, "TSG_JIT_HALF", "TSG_JIT_PAIR", "TSG_JIT_QBLOCK=16",
                                                              "TSG_JIT_QBLOCK=8"}
    assert {c.width for c in cs if c.family == "rows64"} == {128, 64, 32, 16, 8, 0}
    assert {c.width for c in cs if c.family == "rows128"} == {64, 32, 16, 8, 0}
    assert {c.B for c in cs if c.family == "blocked"} == {16, 64}
    assert all(not c.prelu for c in cs if c.family == "blocked")


def test_walk_tile_is_the_planners(tsg):
    """The chunk counts the directed cases are named for (tsg_internal.h kEllMaxC)."""
    assert G.ELL_TILE_M == (1, 4, 8, 16, 32) and G.ELL_MAX_C == (40956, 10236, 5116, 2556, 1276)
    got = {(c.M, c.K): (G.ELL_TILE_M[G.walk_tile(c.M, c.K)], G.walk_chunks(c)[0])
           for c in G.cases() if c.name == "chunked-walk"}
    assert got == {(16, 5120): (16, 3), (32, 5117): (32, 5), (3, 10240): (4, 2), (1, 41000): (1, 2)}
    # the image the library builds for such a tile has that chunk and that many of them
    for (M, K), (tile, nch) in got.items():
        c = next(c for c in G.cases() if c.name == "chunked-walk" and (c.M, c.K) == (M, K))
        C, n = tsg.ell_build(*G.build(c).arrays, K, c.N, G.ELL_MAX_C[G.ELL_TILE_M.index(tile)], tile)[2:4]
        assert (C, n) == (G.ELL_MAX_C[G.ELL_TILE_M.index(tile)], nch), (M, K, C, n)


AUTOMATIC = [c for c in G.cases() if c.mode == 0 and c.family in ("pc", "walk")]


@pytest.mark.parametrize("c", AUTOMATIC, ids=G.case_id)
def test_the_planner_names_the_expected_kernel(tsg, c):
    """set_small_m(0) leaves the kernel to the planner: tsg_call_plan names the
    one the case asserts."""
    plan = tsg.call_plan(c.K, c.N, G.build(c).nnz, c.M)
    assert plan["kernel"] == G.KERNEL[c.family], (c, plan)


def test_there_are_automatic_cases_of_both_walks():
    assert {c.family for c in AUTOMATIC} == {"pc", "walk"}


def test_a_wrong_bit_is_reported_with_the_case():
    c = G.cases()[0]
    want = G.build(c).want["plain"]
    got = want.copy()
    got[c.M - 1, c.N - 1] ^= 1
    with pytest.raises(AssertionError) as e:
        G.assert_bits(got, want, c, "plain")
    msg = str(e.value)
    assert repr(c) in msg and f"1 of {want.size} elements differ" in msg and f"({c.M - 1}, {c.N - 1}," in msg
    G.assert_bits(want.copy(), want, c, "plain")
