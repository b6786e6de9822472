"""The case list of test_gpu_ex_fuzz.py without a GPU: every case builds (the
input conditions of that file's module docstring hold -- edge dependence, the
magnitude bound, the expectation told apart from a fused multiply-add, from the
add before the multiply and from a 16-bit a, RELU and RELU2 told apart from
NONE, everything finite also in the Y type, the placements that the
vec-pattern letters promise), the shares of the cases too small to meet a
threshold alone meet it over their group's pool, the list is deterministic and
complete, it covers what it claims to cover (computed from the tuples and
printed once: run with -s), where a case leaves the kernel to the planner
tsg_call_plan names the kernel the case expects, an in-place operand is exactly
Y's view, and an operand read at the wrong (m, n) would change the expectation."""
import collections

import numpy as np
import pytest

import test_gpu_call_fuzz as CF
import test_gpu_ex_fuzz as G


@pytest.fixture(autouse=True)
def _oracle_built(oracle_mod):
    """The case builder imports the oracle itself: it is built first."""


@pytest.mark.parametrize("c", G.cases(), ids=G.case_id)
def test_case_builds(tsg, c):
    """build() asserts the input conditions; here the shapes and types of what it returns."""
    bc = G.build(c)
    assert str(bc.Xt.dtype) == "torch." + c.xdtype and tuple(bc.Xt.shape) == (c.M, c.K)
    assert bc.want.shape == (c.M, c.N) and bc.want.dtype == (np.uint32 if c.ydtype == "float32" else np.uint16)
    assert bc.want32.shape == bc.y32.shape == (c.M, c.N) and bc.want32.dtype == bc.y32.dtype == np.float32
    assert (bc.deq is not None) == (c.mode != "plain") and (bc.g is not None) == (c.gamma != "none")
    assert (bc.rs is not None) == c.rs and (bc.cs is not None) == c.cs
    for t, w, dtype in ((bc.Gt, bc.Gw, c.multype), (bc.Rt, bc.Rw, c.addtype)):
        assert (t is None) == (w is None) == (dtype is None)
        if dtype:
            assert str(t.dtype) == "torch." + dtype and tuple(t.shape) == (c.M, c.N) and w.dtype == np.float32
    assert not np.array_equal(bc.want32, bc.y32), (c, "the epilogue does not show")


def test_small_cases_meet_the_shares_over_their_group():
    """A case below G.SMALL elements cannot meet a share on its own: the counts
    of its group's small cases are added up and the same thresholds hold."""
    pool = collections.defaultdict(lambda: [0, 0])
    for c in G.cases():
        for name, (differ, total) in G.build(c).pooled.items():
            pool[(c.name, name)][0] += differ
            pool[(c.name, name)][1] += total
    assert pool, "no case is small"
    for (group, name), (differ, total) in pool.items():
        assert total > 0 and G.share_ok(name, differ, total), (group, name, differ, "of", total)


def test_case_list_is_deterministic_and_complete():
    counter = []
    again = tuple(G.directed_cases() + G.drawn_cases(counter))
    assert again == G.cases() and all(type(a) is G.Case for a in again)
    drawn = [c for c in G.cases() if c.name == "drawn"]
    assert len(counter) == len(drawn) == G.PER_PAIR * len(G.PAIRS) == 72
    assert len(G.cases()) == len(counter) + len(G.directed_cases())
    assert len({c.seed for c in G.cases()}) == len(G.cases()) == len({G.case_id(c) for c in G.cases()})


def _chunked(c):
    """K above the chunk of the walk's tile (tsg_internal.h kEllMaxC, restated in CF.ELL_MAX_C)."""
    return c.family == "walk" and c.K > CF.ELL_MAX_C[CF.walk_tile(c.M, c.K)]


def _ops16(c):
    return all(t in ("float16", "bfloat16") for t in (c.multype, c.addtype))


def test_coverage():
    cs = G.cases()
    per_pair = collections.Counter((c.mode, c.family) for c in cs)
    table = [f"cases: {len(cs)} = {len(G.directed_cases())} directed + {sum(c.name == 'drawn' for c in cs)} drawn",
             "mode   " + " ".join(f"{f:>8}" for f in G.FAMILIES) + "  chunked  N<8,16-bit ops  in place"]
    for m in G.MODES:
        table.append(f"{m:<6} " + " ".join(f"{per_pair[(m, f)]:>8}" for f in G.FAMILIES) +
                     f"  {sum(_chunked(c) and c.mode == m for c in cs):>7}"
                     f"  {sum(c.N < 8 and _ops16(c) and c.mode == m for c in cs):>14}"
                     f"  {sum(bool(c.inplace) and c.mode == m for c in cs):>8}")
    groups = collections.Counter(c.name for c in cs)
    table.append("groups: " + ", ".join(f"{n} {v}" for n, v in groups.items()))
    triples = collections.Counter((c.multype, c.addtype, c.ydtype) for c in cs if c.multype and c.addtype)
    table.append(f"(multype, addtype, ytype) triples: {len(triples)} of 27, fewest {min(triples.values())}; "
                 f"acts: " + ", ".join(f"{a} {sum(c.act == a for c in cs)}" for a in G.ACTS))
    print("\n" + "\n".join(table))
    assert set(per_pair) == set(G.PAIRS) and min(per_pair.values()) >= 4, per_pair
    for m in G.MODES:
        mine = [c for c in cs if c.mode == m]
        assert sum(_chunked(c) for c in mine) >= 2, (m, "chunked walk")
        assert sum(c.N < 8 and _ops16(c) for c in mine) >= 2, (m, "N < 8 with 16-bit operands")
        assert {c.xdtype for c in mine} == set(G.xdtypes_of(m)), (m, "X types with an epilogue")
        assert {c.inplace for c in mine} == {None, "add", "mul"}, (m, "in-place forms")
        assert {c.ydtype for c in mine if c.inplace} == set(G.YDTYPES), (m, "in-place Y types")
    assert set(triples) == set(G.TRIPLES), set(G.TRIPLES) - set(triples)
    for f in G.FAMILIES:
        assert {c.inplace for c in cs if c.family == f} == {None, "add", "mul"}, (f, "in-place forms")
        assert {c.yform for c in cs if c.family == f and c.inplace} == {"odd", "aligned"}, (f, "in-place views")
    # what the directed groups promise
    vec = [c for c in cs if c.name == "vec-pattern"]
    for family, width, M, N0 in G.VEC_SHAPES:
        for N in (N0, N0 + 8):
            got = {c.vec for c in vec if (c.family, c.width, c.M, c.N) == (family, width, M, N)}
            assert len(got) == 9 and {v for v in got if "s" not in v} == set(G.VEC_LAYOUTS[:8]) and \
                len([v for v in got if "s" in v]) == 1, (family, width, N, got)
    assert {v for c in vec for v in [c.vec] if "s" in v} == {"asa", "aas"}
    assert all(c.vec is None for c in cs if c.name != "vec-pattern")
    chunked = [c for c in cs if c.name == "chunked-walk-epi"]
    assert all(_chunked(c) and c.act == "relu2" and c.multype and c.addtype and c.ydtype != "float32" for c in chunked)
    for shape in {(c.M, c.K, c.N) for c in chunked}:
        mine = [c for c in chunked if (c.M, c.K, c.N) == shape]
        assert {c.mode for c in mine} == set(G.MODES) and sum(bool(c.inplace) for c in mine) == 1, shape
    small = [c for c in cs if c.name == "small-n-epi"]
    assert {(c.N, c.family) for c in small} == {(n, f) for n in (1, 7, 9, 17) for f in G.FAMILIES}
    assert all(_ops16(c) and c.ydtype != "float32" for c in small)
    assert {c.mode for c in small} == set(G.MODES) and {c.act for c in small} == set(G.ACTS)
    inpl = [c for c in cs if c.name == "in-place"]
    handles = {(c.family, c.knob, c.B) for c in inpl}
    assert handles == {("pc", None, 0), ("walk", None, 0), ("rows64", None, 0), ("rows64", "TSG_JIT_HALF", 0),
                       ("rows64", "TSG_JIT_PAIR", 0), ("rows64", "TSG_JIT_QBLOCK=16", 0), ("rows128", None, 0),
                       ("rx", None, 0), ("blocked", None, 16), ("blocked", None, 64)}
    for hd in handles:
        mine = [c for c in inpl if (c.family, c.knob, c.B) == hd]
        assert {(c.mode, c.inplace) for c in mine} == {(m, f) for m in G.MODES for f in ("add", "mul")}, hd
        assert {c.ydtype for c in mine} == set(G.YDTYPES) and {c.yform for c in mine} == {"odd", "aligned"}, hd
    many = [c for c in cs if c.name == "many-m-tiles"]
    assert {(c.family, c.M) for c in many} == {(f, m) for f in ("rows64", "rows128", "rx") for m in (257, 300)} | \
        {("walk", 300)} and all(c.rs_out for c in many)
    assert any((c.family, c.mode, c.M, c.K, c.N, c.smode) == ("walk", "act", 300, 388, 130, 2) for c in many)
    unusual = [c for c in cs if c.name == "unusual-w-epi"]
    assert {(c.w, c.s, c.family, c.mode) for c in unusual} == {(w, s, f, m) for w, s in (("zero", 4), ("rand", 64), ("rand", 1))
                                                               for f in ("walk", "rows64") for m in ("act", "plain")}
    xoff = [c for c in cs if c.name == "x-offset-epi"]
    assert {(c.mode != "plain", c.xdtype, c.xoff) for c in xoff} == \
        {(False, x, o) for x in ("float16", "bfloat16", "int8") for o in (2, 3)} | \
        {(True, x, o) for x in ("float16", "bfloat16") for o in (2, 3)}
    assert all(bool(c.multype) != bool(c.addtype) for c in xoff) and {c.family for c in xoff} == {"walk", "rows64"}
    # the width, knob and B sets, as in the call fuzz
    assert {c.knob for c in cs if c.family == "rows64"} >= {None, "TSG_JIT_HALF", "TSG_JIT_PAIR", "TSG_JIT_QBLOCK=16",
                                                              "TSG_JIT_QBLOCK=8"}
    assert {c.width for c in cs if c.family == "rows64"} == {128, 64, 32, 16, 8, 0}
    assert {c.width for c in cs if c.family == "rows128"} == {64, 32, 16, 8, 0}
    assert {c.B for c in cs if c.family == "blocked"} == {16, 64}
    drawn = [c for c in cs if c.name == "drawn"]
    assert {c.act for c in drawn} == set(G.ACTS) and {c.multype for c in drawn} == set(G.OPTYPES) == \
        {c.addtype for c in drawn}
    assert any(not (c.rs or c.cs) for c in drawn) and any(c.rs and not c.cs for c in drawn) and \
        any(c.rs and c.cs for c in drawn), "the scale combinations of a PLAIN call"
    assert {c.gamma for c in drawn if c.mode == "norm"} == {"none", "own", "slice"}


def test_walk_tile_is_the_planners():
    """The chunk counts the chunked-walk-epi cases are named for (tsg_internal.h kEllMaxC)."""
    got = {(c.M, c.K): (CF.ELL_TILE_M[CF.walk_tile(c.M, c.K)], CF.walk_chunks(G.as_call_case(c))[0])
           for c in G.cases() if c.name == "chunked-walk-epi"}
    assert got == {(16, 5120): (16, 3), (32, 5117): (32, 5), (3, 10240): (4, 2), (1, 41000): (1, 2)}


AUTOMATIC = [c for c in G.cases() if c.smode == 0 and c.family in ("pc", "walk")]


@pytest.mark.parametrize("c", AUTOMATIC, ids=G.case_id)
def test_the_planner_names_the_expected_kernel(tsg, c):
    """set_small_m(0) leaves the kernel to the planner: tsg_call_plan names the
    one the case asserts."""
    plan = tsg.call_plan(c.K, c.N, G.build(c).nnz, c.M)
    assert plan["kernel"] == G.KERNEL[c.family], (c, plan)


def test_there_are_automatic_cases():
    assert "pc" in {c.family for c in AUTOMATIC}


def test_in_place_operands_are_the_view_of_y():
    """The operand of an in-place case has Y's type, column offset and row
    stride (the GPU test passes the view itself), and the other operand does
    not alias it."""
    mine = [c for c in G.cases() if c.inplace]
    assert len(mine) >= 60
    for c in mine:
        lds = G.build(c).lds
        op = ("mul", c.multype, c.mc0, c.mpad) if c.inplace == "mul" else ("add", c.addtype, c.ac0, c.apad)
        assert op[1:] == (c.ydtype, c.yc0, c.ypad) and lds[op[0]] == lds["Y"] >= c.N, c


def test_operands_vary_along_rows_and_columns():
    """An operand read at the wrong (m, n) changes the expectation: no operand
    is constant along its rows or along its columns.  (Two bf16 gates of a
    two-row operand can be equal by chance, one column in some hundreds: with
    16 lines or more, nine in ten must vary; with fewer, one must.)"""
    def varies(lines, what):
        assert lines.mean() >= 0.9 if lines.size >= 16 else lines.any(), (what, float(lines.mean()))

    for c in G.cases():
        bc = G.build(c)
        for name, w in (("mul", bc.Gw), ("add", bc.Rw)):
            if w is None:
                continue
            if c.N > 1:
                varies((w != w[:, :1]).any(axis=1), (c, name, "is constant along its rows"))
            if c.M > 1:
                varies((w != w[:1, :]).any(axis=0), (c, name, "is constant along its columns"))


def test_a_wrong_bit_is_reported_with_the_case():
    c = G.cases()[0]
    want = G.build(c).want
    got = want.copy()
    got[c.M - 1, c.N - 1] ^= 1
    with pytest.raises(AssertionError) as e:
        CF.assert_bits(got, want, c, "descriptor")
    msg = str(e.value)
    assert repr(c) in msg and f"1 of {want.size} elements differ" in msg and f"({c.M - 1}, {c.N - 1}," in msg
    CF.assert_bits(want.copy(), want, c, "descriptor")
