"""The case lists of test_gpu_i8_fuzz.py without a GPU: every case builds (the
input conditions of that file's module docstring hold), the shares of the cases
too small to meet a threshold alone meet it over their group's pool, the list is
deterministic and complete, the inventory covers what the file claims (every S
of both picks, every (kernel, in_mode) pair, every operand type triple on every
kernel), the picks restated there are the library's, the structured-W and
isolation builders run, and the packed image of every structured W family
decodes back to W with its padding all zero-code."""
import collections

import numpy as np
import pytest

import test_gpu_i8_fuzz as G
from test_gpu_wstruct import FAMILY_NAMES, families


@pytest.fixture(autouse=True)
def _oracle_built(oracle_mod):
    """The case builder imports the oracle itself: it is built first."""


@pytest.mark.parametrize("c", G.cases(), ids=G.case_id)
def test_case_builds(tsg, c):
    bc = G.build(c)
    assert str(bc.Xt.dtype) == "torch." + c.xdtype and tuple(bc.Xt.shape) == (c.M, c.K)
    assert bc.want.shape == (c.M, c.N) and bc.want.dtype == (np.uint32 if c.ydtype == "float32" else np.uint16)
    assert (bc.deq is not None) == (c.mode != "plain") and (bc.g is not None) == (c.gamma != "none")
    assert (bc.rs is not None) == c.rs and (bc.cs is not None) == c.cs and (bc.csu is not None) == c.csu
    assert (bc.Wu is not None) == (bc.u32 is not None) == (bc.arrays_up is not None) == (c.family in G.GLU)
    for t, w, dtype in ((bc.Gt, bc.Gw, c.multype), (bc.Rt, bc.Rw, c.addtype)):
        assert (t is None) == (w is None) == (dtype is None)
        if dtype:
            assert str(t.dtype) == "torch." + dtype and tuple(t.shape) == (c.M, c.N)
    assert np.abs(bc.q.astype(np.int64) @ bc.Wg.astype(np.int64)).max(initial=0) <= 2 ** 24


def test_small_cases_meet_the_shares_over_their_group():
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
    assert collections.Counter((c.mode, c.family) for c in drawn) == {p: G.PER_PAIR for p in G.PAIRS}
    assert len({c.seed for c in G.cases()}) == len(G.cases()) == len({G.case_id(c) for c in G.cases()})


def test_the_picks_are_the_librarys(tsg):
    """gemv_pick / glu_pick restate tsg_internal.h: equal to the library's at every K and N the cases use
    and around every threshold."""
    Ks = {c.K for c in G.cases()} | {64 * s + d for s in (1, 2, 4, 8, 16, 32) for d in (-1, 0, 1)}
    for K in sorted(Ks):
        for N in (1, 32, 33, 577, 16383, 16384, 16390):
            assert tsg.i8gemv_pick(K, N) == G.gemv_pick(K, N), (K, N)
            assert tsg.i8glu_pick(K, N) == G.glu_pick(K), (K, N)


def test_inventory():
    cs = G.cases()
    per_pair = collections.Counter((c.mode, c.family) for c in cs)
    assert set(per_pair) == set(G.PAIRS), per_pair  # every (kernel, in_mode) pair
    # every S either pick can return, and the 64-column tile
    S = collections.defaultdict(set)
    for c in cs:
        if c.family in G.SPLITK:
            S[(c.family, G.pick_of(c)[0])].add(G.pick_of(c)[1])
    assert S[("i8gemv", 32)] == {1, 2, 4, 8, 16} and S[("glu_gemv", 32)] == {1, 2, 4, 8}, dict(S)
    tn64 = [c for c in cs if c.family == "i8gemv" and G.pick_of(c)[0] == 64]
    assert {c.N for c in tn64} == {16384, 16390} and all(c.K == 192 and c.ydtype != "float32" and c.multype and c.addtype
                                                         for c in tn64)
    assert all(c.N < 16384 for c in cs if c not in tn64) and max(c.M for c in cs) == 257
    for family in G.SPLITK:
        mine = [c for c in cs if c.family == family]
        steps = [G.wave_steps(c.K, G.pick_of(c)[1]) for c in mine if c.K]
        assert {n for s in steps for n in s} >= {1, 2, 3}, family            # waves with 1, 2 and 3 steps
        assert any(len(set(s)) == 1 for s in steps) and any(len(set(s)) > 1 for s in steps), family
        assert any(-(-c.K // 64) % G.pick_of(c)[1] == 1 and c.K > 64 for c in mine), family  # nks % S == 1
        assert {c.M for c in mine} >= set(G.SPLIT_MS) and {c.N for c in mine} >= set(G.SPLIT_NS), family
    for family in ("i8mfma", "glu_tile"):
        mine = [c for c in cs if c.family == family]
        assert {(c.M, c.N) for c in mine} >= {(m, n) for m in G.TILE_MS for n in G.TILE_NS}, family
        assert {c.K for c in mine} >= set(G.TILE_KS) | {0, 1} and {c.M for c in mine} >= {1, 5, 32, 257}, family
    for family in G.FAMILIES:
        mine = [c for c in cs if c.family == family]
        triples = {(c.multype, c.addtype, c.ydtype) for c in mine if c.multype and c.addtype}
        assert triples == set(G.TRIPLES), (family, set(G.TRIPLES) - triples)
        assert {c.act for c in mine} == set(G.ACTS) and {c.inplace for c in mine} == {None, "add", "mul"}, family
        assert {c.yform for c in mine if c.inplace} == {"odd", "aligned"}, family
        assert any(c.multype and not c.addtype for c in mine) and any(c.addtype and not c.multype for c in mine), family
        assert {(c.rs, c.cs) for c in mine if c.mode == "plain"} == {(a, b) for a in (False, True) for b in (False, True)}
        assert {(c.K % 16, c.xoff) for c in mine if c.name == "x-16-bytes" and c.mode == "plain"} == \
            {(k, o) for k in (0, 1, 15) for o in G.ALIGN_OFFS}, family
        assert {c.K % 16 for c in mine if c.name == "x-16-bytes" and c.mode != "plain"} == {0, 1, 15}, family
        assert {c.w for c in mine} >= {"rand", "zero", "emptycol", "signcols"}, family
        odd = [c for c in mine if not c.inplace and G.XF.ld_of(c.yc0, c.N, c.ypad) % 2 == 1 and c.yc0 % 2 == 1]
        m8 = [c for c in mine if not c.inplace and G.XF.ld_of(c.yc0, c.N, c.ypad) % 8 == 0]
        assert odd and m8, family
        assert {c.xdtype for c in mine if c.mode != "plain"} == set(G.QX), family
    for family in G.GLU:
        mine = [c for c in cs if c.family == family]
        assert {(c.cs, c.csu) for c in mine} >= {(True, True), (False, True), (True, False)}, family
        assert {c.w for c in mine} >= {"zero_up", "zero_gate"} and any(c.cross for c in mine), family
        crossable = [c for c in mine if c.multype is None]
        assert 0.15 <= sum(c.cross for c in crossable) / len(crossable) <= 0.4, family  # about one in four


def test_a_changed_pick_is_caught():
    """The inventory's S assertion sees a pick that allows S = 16 on the GLU kernel."""
    def wrong(K):
        nks, S = -(-K // 64), 1
        while 2 * S <= 16 and 2 * S <= nks:
            S *= 2
        return 32, S
    got = {wrong(c.K)[1] for c in G.cases() if c.family == "glu_gemv"}
    assert got != {1, 2, 4, 8} and 16 in got
    assert any(wrong(c.K) != G.glu_pick(c.K) for c in G.cases() if c.family == "glu_gemv")


# ---- structured W, isolation -----------------------------------------------------------------------

def _decode(img, Kp, Np):
    """The image back to W: I8Geom::word / shift of tsg_internal.h and the codes pos 0, neg 2, zero 3."""
    k, n = np.meshgrid(np.arange(Kp), np.arange(Np), indexing="ij")
    lane, f = 32 * (k % 32 // 16) + n % 32, 2 * (n % 64 // 32) + k % 64 // 32
    word = (((n // 64) * (Kp // 64) + k // 64) * 64 + lane) * 4 + f
    code = (img[word] >> (8 * (k % 4) + 2 * (k % 16 // 4)).astype(np.uint32)) & 3
    return code


@pytest.mark.parametrize("wname", FAMILY_NAMES)
def test_image_of_structured_w_decodes_to_w(tsg, oracle_mod, wname):
    for K in G.WS_KS:
        for N in (140, 1100):
            W = families(K, N)[wname]
            img, geom = tsg.i8_build(*oracle_mod.tcsc_encode(W).arrays, K, N)
            Kp, Np = -(-K // 64) * 64, -(-N // 128) * 128
            assert geom == (Kp, Np, G.I8_TILE_M, G.I8_TILE_N, G.I8_WAVE_N, G.I8_KSTEP) and img.size == Kp * Np // 16
            code = _decode(img, Kp, Np)
            assert not (code == 1).any()
            assert np.array_equal(np.array([1, 0, -1, 0])[code][:K, :N], W), (wname, K, N)
            pad = np.ones((Kp, Np), bool)
            pad[:K, :N] = False
            assert (code[pad] == 3).all() and (code[:K, :N][W == 0] == 3).all(), (wname, K, N, "padding is not zero-code")


def test_structured_builds():
    assert len(G.ws_cases()) == 4 * len(FAMILY_NAMES)
    for family, wname in G.ws_cases():
        for K in G.WS_KS:
            for M, N in G.WS_SHAPES[family]:
                assert (M <= 32) == (family in G.SPLITK) and M in (130, 5, 32)
                for swap in (False, True) if family in G.GLU else (False,):
                    Wg, Wu, X, b, bu, want = G.ws_build(family, wname, M, K, N, swap)
                    assert want.shape == (M, N) and np.abs(X).max() == 127 and (Wu is None) == (family not in G.GLU)


def test_isolation_builds():
    assert len(G.ISO_CASES) == 12  # M = 33: the two tile kernels; M = 5: all four
    for family, M, K, N in G.ISO_CASES:
        ic = G.iso_build(family, M, K, N)
        assert ic.want.shape == (M, N) and (ic.Wu is not None) == (family in G.GLU)
    for kind, quant in G.STALE:
        for M, scale in ((130, 300.0), (33, 3.0), (5, 3.0)):
            ic = G.stale_build(G.iso_family_of(kind, M), M, G.STALE_K, G.STALE_N, quant, scale)
            assert ic.want.shape == (M, G.STALE_N) and (ic.swapped is not None) == (kind == "glu")
            if kind == "glu":
                assert not np.array_equal(ic.want, ic.swapped)
