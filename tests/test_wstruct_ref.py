"""The structured W of test_gpu_wstruct.py without a GPU.

Every family's defining property holds on the W families() returns; removing a
family's last entry (the highest k of its last populated column) changes the
expected Y of every GPU case, so a dropped entry cannot go unseen; every jit
stream a GPU case runs is emulated here first (tests/test_jit_codegen.py's
workgroup emulator: the waves' barrier counts agree, no LDS read before its data
landed, no DMA over rows read since its issue, one add per nonzero, Y equal to
the oracle bit for bit on order-sensitive X), and the sliced-ELL images of the
walks are replayed (tests/test_ell_format.py); per (tile, wave) stream the adds
equal the nonzeros of the stream's columns and the barrier counts of a tile's
waves agree, which is where a family's mechanism shows in the emitted code: a
stream without entries runs to every barrier, quad_row* emits ds_read_b32 only,
neg_only no add that is not negated.  The registration paths (dense, packed CSC,
validation, column slices) round-trip every family.

The emulated shapes: the 64-row image at (width, waves) = (128, 8), (64, 8),
(16, 8), (16, 4), (8, 8) in the row layout and with TSG_JIT_QBLOCK=16, its half
ring at width 16, the 128-row image at (64, 8), (16, 4), (8, 8), blocked B = 64,
all at K = 600 and 601, N = 140 (emulated() names the few left out at K = 601);
the shapes the GPU runs at N = 1100 (64-row width 128, 128-row width 64) there
too; the ELL image at (Cmax, MT) = (256, 32), (2556, 16), (128, 8), (40956, 1)."""
import numpy as np
import pytest

import test_ell_format as E
import test_gpu_wstruct as G
import test_jit_codegen as J

M_EMU = 5

# (image rows, width, waves, layout): layout "rows" / "16" (TSG_JIT_QBLOCK) / "half" for the 64-row
# image, "pairs" for the 128-row image, "B64" blocked
JIT_CONFIGS = ([(64, width, waves, layout) for width, waves in ((128, 8), (64, 8), (16, 8), (16, 4), (8, 8))
                for layout in ("rows", "16")] +
               [(64, 16, 4, "half"), (128, 64, 8, "pairs"), (128, 16, 4, "pairs"), (128, 8, 8, "pairs"),
                (128, 64, 8, f"B{G.B_BLOCKED}")])
WIDE_CONFIGS = [(64, 128, 8, "rows"), (128, 64, 8, "pairs")]
ELL_CONFIGS = [(256, 32), (2556, 16), (128, 8), (40956, 1)]


def _gpu_configs():
    return {G.jit_config(c) for c in G.cases()} - {None}


def emulated():
    """Every (family, K, N, config) test_emulated_stream runs.  Left out, to keep the file's run
    time down: at K = 601 the shapes whose chunks do not depend on K % 4 (every layout but the row
    layout) and that no GPU case runs -- K = 600 emulates them."""
    gpu = _gpu_configs()
    out = [(w, K, G.N_SMALL, cfg) for w in G.FAMILY_NAMES for K in G.KS for cfg in JIT_CONFIGS
           if K % 4 == 0 or cfg[3] == "rows" or cfg in gpu]
    out += [(w, K, G.N_WIDE, cfg) for w in G.FAMILY_NAMES for K in G.KS for cfg in WIDE_CONFIGS]
    return out


def _emu_id(p):
    w, K, N, (rows, width, waves, layout) = p
    return f"{w}-{K}x{N}-r{rows}-w{width}x{waves}-{layout}"


@pytest.fixture(autouse=True)
def _oracle_built(oracle_mod):
    """G.families imports the oracle itself: it is built first."""


def _codegen(tsg, O, monkeypatch, W, K, N, cfg):
    rows, width, waves, layout = cfg
    monkeypatch.delenv("TSG_JIT_QBLOCK", raising=False)
    if layout == "16":
        monkeypatch.setenv("TSG_JIT_QBLOCK", "16")
    if layout.startswith("B"):
        arrays = O.blocked_tcsc_encode(G.blocked_w(W, int(layout[1:])), int(layout[1:]))
        return arrays, tsg.jit_codegen(*arrays, K, N, B=int(layout[1:]))
    arrays = O.tcsc_encode(W).arrays
    if rows == 64:
        return arrays, tsg.jit_codegen64(*arrays, K, N, width=width, waves=waves, half=layout == "half")
    return arrays, tsg.jit_codegen(*arrays, K, N, width=width, waves=waves)


def _streams(code, wcode, G_):
    """Per (tile, wave): the decoded instructions of its stream, up to its return."""
    out = []
    for off in wcode:
        pc, ins = int(off) // 4, []
        while True:
            kind, f, n = J._decode(code, pc, G_)
            ins.append((kind, f))
            pc += n
            if kind == "ret":
                break
        out.append(ins)
    return out


def _reach(w, W, K, N, cfg, code, wcode):
    """The family's mechanism in the emitted code."""
    rows, width, waves, layout = cfg
    geom = J.Geom(code)
    if layout == "rows":
        assert geom.rowlay and geom.chunk == G.CHUNK_ROWLAY
    elif layout in ("16", "half"):
        assert not geom.rowlay and geom.chunk == (G.CHUNK_128 if layout == "half" else G.CHUNK_QBLOCK)
    else:
        assert not geom.r64 and geom.chunk == G.CHUNK_128
    streams = _streams(code, wcode, geom)
    S = geom.streams
    assert S == waves and geom.nw == width and len(streams) == -(-N // (S * width)) * S
    Wp = np.zeros((K, len(streams) * width), np.int32)
    Wp[:, :N] = G.blocked_w(W, geom.B) if geom.B else W
    adds = [[f for kind, f in ins if kind in ("vadd", "add", "first")] for ins in streams]
    bars = [sum(kind == "barrier" for kind, _ in ins) for ins in streams]
    for i, ins in enumerate(streams):
        # one add per nonzero of the stream's columns, the negated ones its -1 entries
        cols = Wp[:, i * width:(i + 1) * width]
        assert len(adds[i]) == np.count_nonzero(cols) and sum(f[2] for f in adds[i]) == np.count_nonzero(cols == -1), \
            (w, cfg, "stream", i)
        # every wave of a tile meets every barrier, whatever its own work
        assert bars[i] == bars[i // S * S] and bars[i] > 0, (w, cfg, "stream", i, bars[i], bars[i // S * S])
    reads = [f[3] for ins in streams for kind, f in ins if kind == "read"]
    if w in G.QUAD_FAMILIES and rows == 64:
        assert reads and set(reads) == {1}, (w, cfg, "ds_read_b32 only", sorted(set(reads)))
    if w in G.QUAD_FAMILIES and rows == 128:
        assert reads and set(reads) == {2}, (w, cfg, "ds_read_b64 only", sorted(set(reads)))
    if w == "neg_only":
        assert all(f[2] for a in adds for f in a) and any(adds), (w, cfg, "an add that is not negated")
    if w == "pos_only":
        assert not any(f[2] for a in adds for f in a) and any(adds), (w, cfg, "a negated add")
    nws = G._wave_columns(N, False)[1]
    if w in ("wave0_only", "wave_last_only") and width in nws:
        only = S - 1 if w == "wave_last_only" else 0
        busy = {i % S for i in range(len(streams)) if adds[i]}
        assert busy == {only}, (w, cfg, "waves with adds", busy)
        for i in range(len(streams)):  # the seven others: no add, no read, and every barrier of the busy wave's
            if i % S != only:
                assert not adds[i] and not any(kind == "read" for kind, _ in streams[i])
                assert bars[i] == bars[i // S * S + only]


@pytest.mark.parametrize("p", emulated(), ids=_emu_id)
def test_emulated_stream(tsg, oracle_mod, monkeypatch, p):
    w, K, N, cfg = p
    rows, width, waves, layout = cfg
    O = oracle_mod
    W = G.families(K, N)[w]
    (_, (code, wcode)) = _codegen(tsg, O, monkeypatch, W, K, N, cfg)
    _reach(w, W, K, N, cfg, code, wcode)
    if layout.startswith("B"):
        J._check_blocked(tsg, O, M_EMU, K, N, 0, int(layout[1:]), 3, True, W=G.blocked_w(W, int(layout[1:])))
    else:
        J._check(tsg, O, M_EMU, K, N, 0, 3, True, W=W, width=width, waves=waves, rows64=rows == 64,
                 half=layout == "half")


def test_gpu_jit_cases_are_emulated_first():
    """No generated stream reaches a GPU without the emulator having accepted it."""
    done = set(emulated())
    jit = [c for c in G.cases() if G.jit_config(c) is not None]
    assert jit and {c.family for c in jit} == {"rows64", "rows128", "blocked"}
    missing = [c for c in jit if (c.w, c.K, c.N, G.jit_config(c)) not in done]
    assert not missing, missing[:5]


@pytest.mark.parametrize("Cmax,MT", ELL_CONFIGS)
@pytest.mark.parametrize("K", G.KS)
@pytest.mark.parametrize("w", G.FAMILY_NAMES)
def test_ell_replay(tsg, oracle_mod, w, K, Cmax, MT):
    """The walks' sliced-ELL image: one chunk (2556, 40956) and chunked (256, 128) walks."""
    O = oracle_mod
    N = G.N_SMALL
    W = G.families(K, N)[w]
    t = O.tcsc_encode(W)
    ent, tab, C, nch = tsg.ell_build(*t.arrays, K, N, Cmax, MT)
    assert (nch > 1) == (Cmax < K) and C % 4 == 0
    X = O.init_x_frac(3, K, 4)
    b = np.linspace(-1, 2, N).astype(np.float32)
    Y = E.replay(ent, tab, C, nch, X, K, N, MT) + b
    assert np.array_equal(Y.view(np.uint32), O.base_tcsc(X, t, b).view(np.uint32))
    used = ent[128:int((tab[:, 0] + (tab[:, 1] & 0xFFFF)).max(initial=1)) * 128]
    assert np.count_nonzero(used != C * MT) == np.count_nonzero(W)
    if w == "one_dense_column" and nch == 1:
        # the dense column's slice is padded 15 / 16: K entries among 16 lists of K rounded up to 8
        assert len(used) - np.count_nonzero(used != C * MT) >= 15 * K


# ---- the families -----------------------------------------------------------------------------------

SHAPES = [(K, N) for K in G.KS for N in (G.N_SMALL, G.N_WIDE)] + [(G.K_WALK_CHUNKED, G.N_SMALL)]


@pytest.mark.parametrize("K,N", SHAPES)
def test_family_properties(K, N):
    fams, base = G._families(K, N, G.SEED)
    assert tuple(fams) == G.FAMILY_NAMES
    for name, W in fams.items():
        G.assert_family(name, W, K, N, base)
    again = G._families.__wrapped__(K, N, G.SEED)[0]  # deterministic in its arguments
    assert all(np.array_equal(again[name], W) for name, W in fams.items())
    assert len({W.tobytes() for W in fams.values()}) == len(fams)


def test_case_list():
    cs = G.cases()
    assert len(cs) == len(set(cs)) == len({G.case_id(c) for c in cs})
    per = {}
    for c in cs:
        per.setdefault(c.w, []).append(c)
    assert tuple(per) == G.FAMILY_NAMES
    for w, mine in per.items():
        assert {c.family for c in mine} == set(G.KERNEL)
        assert {(c.width, c.knob) for c in mine if c.family == "rows64"} == {
            (128, None), (16, None), (8, None), (16, "TSG_JIT_HALF"), (16, "TSG_JIT_PAIR"), (16, "TSG_JIT_QBLOCK=16")}
        assert {c.width for c in mine if c.family == "rows128"} == {64, 8}
        assert {c.K for c in mine if c.family != "walk"} == set(G.KS)
        assert sorted(c.K for c in mine if c.family == "walk") == sorted(G.KS + (G.K_WALK_CHUNKED,))
        assert {(c.family, c.width) for c in mine if c.N == G.N_WIDE} == {("rows64", 128), ("rows128", 64), ("rx", 0)}
        assert {c.M for c in mine} == {2, 16, 65, 130, 70}
    print(f"\n{len(cs)} GPU cases = {len(per)} families x {len(cs) // len(per)}")


def test_walk_shapes_are_the_planners(tsg):
    """The chunked walk case runs three LDS chunks of the 16-row tile; pc and the walk at K = 600
    one chunk (tsg_internal.h kEllMaxC, as test_gpu_call_fuzz restates it)."""
    import test_gpu_call_fuzz as CF
    assert CF.ELL_TILE_M[CF.walk_tile(16, G.K_WALK_CHUNKED)] == 16
    assert -(-G.K_WALK_CHUNKED // CF.ELL_MAX_C[CF.walk_tile(16, G.K_WALK_CHUNKED)]) == 3
    assert all(K <= CF.ELL_MAX_C[CF.walk_tile(16, K)] for K in G.KS)
    for K in G.KS:
        nnz = int(np.count_nonzero(G.families(K, G.N_SMALL)["last_row_only"]))
        assert tsg.call_plan(K, G.N_SMALL, nnz, 2)["kernel"] == G.KERNEL["pc"]


def _distinct_builds():
    return sorted({(c.w, c.K, c.N, c.M, c.B) for c in G.cases()})


@pytest.mark.parametrize("w", G.FAMILY_NAMES)
def test_a_dropped_last_entry_changes_y(oracle_mod, w):
    """Sensitivity: without the family's last entry the expected Y of every GPU case differs."""
    O = oracle_mod
    for _, K, N, M, B in (b for b in _distinct_builds() if b[0] == w):
        arrays, X, b, want = G.build(w, K, N, M, B)
        W = G.families(K, N)[w]
        W = G.blocked_w(W, B) if B else W
        if not W.any():  # (a blocked handle of a family that lives in the rows past the last block: Y = b)
            assert B and w == "last_row_only"
            assert np.array_equal(want, np.ascontiguousarray(np.broadcast_to(b, (M, N))).view(np.uint32))
            continue
        k, n = G.last_entry(W)
        W2 = W.copy()
        W2[k, n] = 0
        if B:
            got = O.base_blocked_tcsc(X, O.blocked_tcsc_encode(W2, B), b, K, N, B)
        else:
            got = O.base_tcsc(X, O.tcsc_encode(W2), b)
        diff = got.view(np.uint32) != want
        assert diff[:, n].any() and not np.delete(diff, n, axis=1).any(), (w, K, N, M, B, k, n)


def test_a_wrong_bit_is_reported_with_the_case():
    c = G.cases()[0]
    want = G.build(c.w, c.K, c.N, c.M, c.B)[3]
    got = want.copy()
    got[c.M - 1, c.N - 1] ^= 1
    with pytest.raises(AssertionError) as e:
        G.assert_bits(got, want, c, "aligned")
    assert repr(tuple(c)) in str(e.value) and f"1 of {want.size} elements differ" in str(e.value)
    G.assert_bits(want.copy(), want, c, "aligned")


# ---- registration paths (host side) -----------------------------------------------------------------

@pytest.mark.parametrize("w", G.FAMILY_NAMES)
def test_host_registration_paths(tsg, oracle_mod, w):
    """validate, packed-CSC round trip and column slices of every family at (600, 140)."""
    O = oracle_mod
    K, N = G.KS[0], G.N_SMALL
    W = G.families(K, N)[w]
    t = O.tcsc_encode(W)
    tsg.validate(*t.arrays, K, N)
    packed = tsg.tcsc_to_csc_packed(*t.arrays, N)
    for a, b in zip(packed, O.csc_packed_encode(W)):
        assert np.array_equal(a, b)
    for a, b in zip(tsg.csc_packed_to_tcsc(*packed, N), t.arrays):
        assert np.array_equal(a, b)
    cuts = [0, N // 3, 2 * N // 3, N]
    for n0, n1 in zip(cuts, cuts[1:]):
        got = tsg.tcsc_slice(*t.arrays, N, n0, n1)
        for a, b in zip(got, O.tcsc_encode(W[:, n0:n1]).arrays):
            assert np.array_equal(a, b), (w, n0, n1)
        tsg.validate(*got, K, n1 - n0)
        if w == "empty_shard" and n0 == N // 3:
            assert len(got[2]) == 0 and len(got[3]) == 0 and not got[0].any() and not got[1].any()
    whole = tsg.tcsc_slice(*t.arrays, N, 0, N)
    for a, b in zip(whole, t.arrays):
        assert np.array_equal(a, b)
