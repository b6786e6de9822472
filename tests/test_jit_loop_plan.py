"""The looping launch's host side (tsg_plan.cpp loop_wgs, tsg_call_grid; host
only): which calls loop, on what grid, that the ids a looping grid visits
cover the tile grid exactly once through the unchanged tile map, that
TSG_JIT_LOOP is parsed strictly, and that the plan dictionary is the one it
was (the loop is a launch decision, not part of the plan)."""
import pytest

G = 256  # an MI355X's compute units: the grid a one-workgroup-per-unit loop takes


@pytest.fixture(autouse=True)
def _no_loop_knob(monkeypatch):
    monkeypatch.delenv("TSG_JIT_LOOP", raising=False)


def _nnz(K, N, s=4):
    return K * N // s


def test_no_call_loops_by_default(tsg):
    """The A/B of DESIGN.md 4.2 (profiles/loop_ab.jsonl) does not reach the
    margin that would make the loop the default launch: without TSG_JIT_LOOP
    every call launches one workgroup per logical id."""
    for M, width in ((4096, 0), (4096, 128), (1088, 128), (1024, 128)):
        g, t = tsg.call_grid(4096, 16384, _nnz(4096, 16384), M, 64 if width else 0, width)
        assert g == t == (M // 64) * 16, (M, width, g, t)


def test_loop_wgs_rule(tsg, monkeypatch):
    monkeypatch.setenv("TSG_JIT_LOOP", str(G))
    # configs[2]: 64 M tiles x 16 column tiles of the 64-row image's 128 x 8
    assert tsg.call_grid(4096, 16384, _nnz(4096, 16384), 4096) == (G, 1024)
    # one round and less: the launch it was
    assert tsg.call_grid(4096, 16384, _nnz(4096, 16384), 1024, 64, 128) == (256, 256)
    assert tsg.call_grid(4096, 16384, _nnz(4096, 16384), 960, 64, 128) == (240, 240)
    # one id more than the grid loops
    assert tsg.call_grid(4096, 16384, _nnz(4096, 16384), 1088, 64, 128) == (G, 272)
    # the 128-row image never loops
    g, t = tsg.call_grid(4096, 16384, _nnz(4096, 16384), 4096, 128, 64)
    assert g == t == 32 * 32
    # nor do the 64-row image's 4-wave shapes: (64, 4096, 16384) is 16 x 4 (test_call_plan.py)
    monkeypatch.setenv("TSG_JIT_LOOP", "8")
    assert tsg.call_plan(4096, 16384, _nnz(4096, 16384), 64)["waves"] == 4
    g, t = tsg.call_grid(4096, 16384, _nnz(4096, 16384), 64, 64, 0)
    assert g == t == 256


def test_loop_knob(tsg, monkeypatch):
    args = (4096, 16384, _nnz(4096, 16384), 4096, 64, 128)
    monkeypatch.setenv("TSG_JIT_LOOP", "0")
    assert tsg.call_grid(*args) == (1024, 1024)
    for cap in (1, 3, 8, 1000, 4096):
        monkeypatch.setenv("TSG_JIT_LOOP", str(cap))
        assert tsg.call_grid(*args) == (min(cap, 1024), 1024)
        # the cap does not make other images loop
        assert tsg.call_grid(4096, 16384, _nnz(4096, 16384), 4096, 128, 64) == (1024, 1024)
    for bad in ("", "-1", "4097", "8x", "0x8", "8 ", "1,2", "on"):
        monkeypatch.setenv("TSG_JIT_LOOP", bad)
        assert "TSG_JIT_LOOP" in tsg.knob_check() and "expected" in tsg.knob_check(), bad
        with pytest.raises(tsg.TSGError):
            tsg.call_grid(*args)
    monkeypatch.setenv("TSG_JIT_LOOP", "8")
    assert tsg.knob_check() == ""


def test_malformed_loop_knob_is_refused_at_registration(tsg, monkeypatch):
    import numpy as np
    monkeypatch.setenv("TSG_JIT_LOOP", "many")
    z = np.zeros(5, np.int32)
    with pytest.raises(tsg.TSGError, match="TSG_JIT_LOOP"):
        tsg.TCSCDevice(z, z, np.zeros(0, np.int32), np.zeros(0, np.int32), 8, 4)


@pytest.mark.parametrize("gn,gm", [(2, 16), (4, 8), (1, 32)])
@pytest.mark.parametrize("mtiles,ntiles,G", [(64, 16, 256), (63, 16, 256), (33, 5, 64), (7, 3, 8), (9, 2, 16),
                                             (4, 3, 3), (2, 2, 1), (40, 1, 8), (1, 40, 24), (17, 17, 256)])
def test_looped_ids_cover_the_grid_once(tsg, gn, gm, mtiles, ntiles, G):
    """Workgroup b of G runs ids b, b + G, ... below the tile count; through
    tsg_jit_tile those are a bijection onto mtiles x ntiles, for tile counts
    that are and are not multiples of G, and each id keeps its XCD when G is a
    multiple of 8."""
    T = mtiles * ntiles
    g_n, g_m = min(gn, ntiles), min(gm, mtiles)  # a group never exceeds the grid (pick_jit_map)
    seen = set()
    for b in range(min(G, T)):
        for L in range(b, T, G):
            if G % 8 == 0:
                assert L % 8 == b % 8
            nt, mt = tsg.jit_tile_map(L, mtiles, ntiles, g_n, g_m)
            assert 0 <= nt < ntiles and 0 <= mt < mtiles
            assert (nt, mt) not in seen
            seen.add((nt, mt))
    assert len(seen) == T


def test_call_plan_dictionary_unchanged(tsg, monkeypatch):
    keys = {"kernel", "width", "waves", "far", "map", "tmask"}
    want = dict(kernel="tsg_jit64_kernel", width=128, waves=8, far=False, map=(2, 16), tmask=3)
    for knob in (None, "0", "8"):
        if knob is not None:
            monkeypatch.setenv("TSG_JIT_LOOP", knob)
        got = tsg.call_plan(4096, 16384, _nnz(4096, 16384), 4096)
        assert set(got) == keys and got == want, (knob, got)
