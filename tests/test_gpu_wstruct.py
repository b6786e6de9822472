"""Skewed, banded and pruned W through every kernel family on the GPU.

Everything else in this suite that depends on the structure of W draws it from
oracle.gen_ternary / tsg_gen_tcsc (generateSparseMatrix): every
row of W holds exactly N / s nonzeros at uniform random columns, so no row is
empty, every wave of a workgroup has the same work in every step, every quad of
a chunk is used, every ELL slice has lists of nearly equal length, both passes
are populated in every chunk and no column exceeds the rx stream's 8 entries
per block by much.  families() below is the list of W that are not like that:
pruned rows and whole chunks of them, dead columns and column shards, one pass
only, one wave only, power-law columns, bands.  Each family asserts its
defining property, with the layout constants restated from tsg_internal.h next
to it.

The GPU cases: every family x kernel family (pc, walk, rows64 at its widths and
knobs, rows128, rx, blocked) at the smallest M with a ragged second M tile.
Per case the plain fp32 gemm_torch runs twice on order-sensitive X
(init_x_frac) -- once 16-byte aligned (the 64-row image reads X directly where
K % 4 == 0) and once one element off alignment (the staged copy) -- and every
element is compared as uint32 with base_tcsc / base_blocked_tcsc.  No
tolerance, no case skipped or redrawn.  The typed, scaled, quantising and
epilogue calls are not repeated: W's structure reaches them only through the
chain checked here.

tests/test_wstruct_ref.py is the CPU twin: it runs the property, reach and
sensitivity assertions, emulates every jit stream that jit_config() below names and
asserts that each jit case of cases() is among them, so no generated stream
reaches a GPU without the emulator having accepted its barrier structure."""
import collections
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32

# ---- the layout constants (tsg_internal.h) ----------------------------------------------------------
PAIR, QUAD = 2, 4              # K rows per LDS unit of the 128-row / 64-row image
CHUNK_128 = 96                 # kJitChunk; the half ring's kJit64HalfChunk too
CHUNK_ROWLAY = 188             # kJit64RowChunk: the 64-row image's row layout (the default)
CHUNK_QBLOCK = 192             # kJit64Chunk: its blocked layouts (TSG_JIT_QBLOCK)
CHUNK_RX = 64                  # kRxChunk
CHUNKS = (CHUNK_RX, CHUNK_128, CHUNK_ROWLAY, CHUNK_QBLOCK)
RX_BLOCK_ROWS, RX_CAP = 24, 8  # kRxBlockRows, kRxCap: rows per block, entries per column and block
RX_NW, RX_WAVES = 32, 8        # kRxNW, kRxWaves
ELL_SLICE, ELL_PAD = 16, 8     # an ELL slice's columns; its lists are padded in blocks of 8 entries
WAVES = 8                      # kJitWaves
# the stream widths the one-wave families hold for (every nw listed: (n // nw) % WAVES is the wave);
# 128 joins where W is wider than one 1024-column tile of the 128-wide streams
WAVE_NWS = (8, 16)
WAVE_NWS_WIDE = (8, 16, 128)

SEED = 4242
KS = (600, 601)                # four row-layout chunks; K % 4 == 0 (shifted last chunk, direct X) and not
N_SMALL, N_WIDE = 140, 1100    # two 64-column tiles and a ragged third; one 1024-column tile and a ragged one
K_WALK_CHUNKED = 5120          # the 16-row walk tile's chunk is 2556 rows: three LDS chunks
B_BLOCKED = 64

QUAD_FAMILIES = tuple(f"quad_row{r}" for r in range(QUAD))


def _signs(base):
    """base where it is nonzero, a fixed +-1 checkerboard elsewhere: a sign for every (k, n)."""
    K, N = base.shape
    alt = np.where((np.add.outer(np.arange(K), np.arange(N)) & 1) == 0, 1, -1)
    return np.where(base != 0, base, alt).astype(np.int32)


def _wave_columns(N, last):
    """Columns whose wave (n // nw) % WAVES is 0 (last: WAVES - 1) at every nw of the list."""
    nws = WAVE_NWS_WIDE if N > 1024 else WAVE_NWS
    n = np.arange(N)
    keep = np.ones(N, bool)
    for nw in nws:
        keep &= (n // nw) % WAVES == (WAVES - 1 if last else 0)
    return keep, nws


def powerlaw_counts(K, N):
    return np.rint(K * (1.0 + np.arange(N)) ** -1.2).astype(np.int64)


def chunk_last_mask(K):
    k = np.arange(K)
    m = np.zeros(K, bool)
    for C in CHUNKS:
        m |= k % C == C - 1
    return m


def dense_column(N):
    return N // 3


def _populated_chunks(W, C, sign):
    return set(np.flatnonzero((W == sign).any(axis=1)) // C)


def assert_family(name, W, K, N, base):
    """The defining property of the family, on the W families() returns."""
    assert W.shape == (K, N) and W.dtype == np.int32 and np.isin(W, (-1, 0, 1)).all(), name
    rows = np.flatnonzero(np.abs(W).sum(axis=1))
    cols = np.flatnonzero(np.abs(W).sum(axis=0))
    assert len(rows) and len(cols), (name, "W is empty")
    if name in ("neg_only", "pos_only"):
        sign = -1 if name == "neg_only" else 1
        assert np.array_equal(W, sign * np.abs(base)) and (W == sign).any() and not (W == -sign).any()
    elif name == "pos_head_neg_tail":
        assert (W[:K // 3] >= 0).all() and (W[K - K // 3:] <= 0).all() and not W[K // 3:K - K // 3].any()
        assert (W == 1).any() and (W == -1).any()
        for C in CHUNKS:  # each pass populated in different chunks, and an empty step between them
            pos, neg = _populated_chunks(W, C, 1), _populated_chunks(W, C, -1)
            assert pos and neg and max(pos) < min(neg), (C, pos, neg)
            assert C > CHUNK_128 or max(pos) + 1 < min(neg), (C, pos, neg)
    elif name == "zero_rows_188_384":
        assert not W[188:384].any() and np.array_equal(W[:188], base[:188]) and np.array_equal(W[384:], base[384:])
        assert W[187].any() and W[384].any()
        empty = {C: sorted(set(range(-(-K // C))) - set(rows // C)) for C in CHUNKS}
        assert empty == {CHUNK_RX: [3, 4, 5], CHUNK_128: [2, 3], CHUNK_ROWLAY: [1], CHUNK_QBLOCK: [1]}, empty
    elif name == "only_tail_rows":
        k0 = K - K // 3
        assert not W[:k0].any() and np.array_equal(W[k0:], base[k0:]) and W[k0].any()
        assert all(k0 // C >= 1 for C in CHUNKS)  # every stream starts with an empty step
    elif name == "last_row_only":
        assert list(rows) == [K - 1]
    elif name == "first_and_last_row":
        assert list(rows) == [0, K - 1]
    elif name in QUAD_FAMILIES:
        r = QUAD_FAMILIES.index(name)
        assert (rows % QUAD == r).all() and len(rows) == len(range(r, K, QUAD))
        assert (rows % PAIR == r % PAIR).all()  # one row of every pair too
    elif name == "chunk_last_rows":
        assert np.array_equal(rows, np.flatnonzero(chunk_last_mask(K)))
        assert all((rows % C == C - 1).any() for C in CHUNKS)
        assert (rows % QUAD == QUAD - 1).all()  # (every chunk size is a multiple of a quad)
    elif name == "rowlay_overlap":
        assert list(rows) == list(range(K - 192, K - 184)) and K - 192 >= 0
        # ... which straddle the first row of the shifted last chunk (jit64_row_kbase: K - 188)
        assert rows[0] < K - CHUNK_ROWLAY <= rows[-1]
    elif name in ("wave0_only", "wave_last_only"):
        keep, nws = _wave_columns(N, name == "wave_last_only")
        assert np.array_equal(cols, np.flatnonzero(keep))
        for nw in nws:
            assert set((cols // nw) % WAVES) == {WAVES - 1 if name == "wave_last_only" else 0}, (name, nw)
    elif name == "powerlaw_cols":
        cnt = np.abs(W).sum(axis=0)
        assert np.array_equal(cnt, powerlaw_counts(K, N)) and cnt[0] == K and (np.diff(cnt) <= 0).all()
        assert cnt[0] >= 100 * max(cnt[-1], 1)  # column norms over orders of magnitude
        # an ELL slice with one long list beside short ones, an rx block at its cap beside empty columns
        assert cnt[0] > 4 * cnt[ELL_SLICE - 1] + ELL_PAD and (cnt[RX_NW - 1] < K // RX_BLOCK_ROWS or cnt[-1] == 0)
    elif name == "one_dense_column":
        c = dense_column(N)
        assert list(cols) == [c] and np.array_equal(W[:, c], np.where(np.arange(K) % 2 == 0, 1, -1))
        assert c % ELL_SLICE != 0 and RX_BLOCK_ROWS // PAIR > RX_CAP  # 12 entries of a pass per 24 rows: cap splits
    elif name == "banded":
        k, n = np.arange(K)[:, None], np.arange(N)[None, :]
        assert np.array_equal(W != 0, np.abs(k * N - n * K) <= 3 * K)
        assert np.abs(W).sum(axis=0).max() <= 7 * -(-K // N) + 1
    elif name == "empty_shard":
        a, b = N // 3, 2 * N // 3
        assert not W[:, a:b].any() and np.array_equal(W[:, :a], base[:, :a]) and np.array_equal(W[:, b:], base[:, b:])
        assert b - a >= 2 * ELL_SLICE  # whole slices (and whole 8-column tiles) without an entry
    else:
        raise AssertionError(f"no property for family {name}")


@functools.lru_cache(maxsize=None)
def _families(K, N, seed):
    import oracle as O
    assert K >= 400 and N >= 48, (K, N)
    base = O.gen_ternary(K, N, 2, seed)
    S = _signs(base)
    k, n = np.arange(K)[:, None], np.arange(N)[None, :]
    zero = np.zeros((K, N), np.int32)
    out = {}

    def rows_of(mask, src=base):
        return np.where(np.broadcast_to(np.asarray(mask).reshape(K, 1), (K, N)), src, 0).astype(np.int32)

    out["neg_only"] = -np.abs(base)
    out["pos_only"] = np.abs(base)
    out["pos_head_neg_tail"] = np.where((k < K // 3) & (base == 1), 1, np.where((k >= K - K // 3) & (base == -1), -1, 0))
    out["zero_rows_188_384"] = rows_of((k < 188) | (k >= 384))
    out["only_tail_rows"] = rows_of(k >= K - K // 3)
    out["last_row_only"] = rows_of(k == K - 1)
    out["first_and_last_row"] = rows_of((k == 0) | (k == K - 1))
    for r, name in enumerate(QUAD_FAMILIES):
        out[name] = rows_of(k % QUAD == r)
    out["chunk_last_rows"] = rows_of(chunk_last_mask(K))
    out["rowlay_overlap"] = rows_of((k >= K - 192) & (k < K - 184))
    out["wave0_only"] = np.where(_wave_columns(N, False)[0][None, :], S, 0)
    out["wave_last_only"] = np.where(_wave_columns(N, True)[0][None, :], S, 0)
    rng = np.random.default_rng(seed)
    W = zero.copy()
    for c, cnt in enumerate(powerlaw_counts(K, N)):
        pick = np.sort(rng.permutation(K)[:cnt])
        W[pick, c] = S[pick, c]
    out["powerlaw_cols"] = W
    W = zero.copy()
    W[:, dense_column(N)] = np.where(np.arange(K) % 2 == 0, 1, -1)
    out["one_dense_column"] = W
    out["banded"] = np.where(np.abs(k * N - n * K) <= 3 * K, S, 0)
    out["empty_shard"] = np.where((n >= N // 3) & (n < 2 * N // 3), 0, base)
    for name in out:
        out[name] = np.ascontiguousarray(out[name], np.int32)
        assert_family(name, out[name], K, N, base)
        out[name].setflags(write=False)
    return out, base


def families(K, N, seed=SEED):
    """{name: W [K, N] int32}, deterministic in its arguments; oracle.gen_ternary(K, N, 2, seed)
    is the sign source.  The arrays are shared and read-only."""
    return dict(_families(K, N, seed)[0])


FAMILY_NAMES = ("neg_only", "pos_only", "pos_head_neg_tail", "zero_rows_188_384", "only_tail_rows", "last_row_only",
                "first_and_last_row") + QUAD_FAMILIES + ("chunk_last_rows", "rowlay_overlap", "wave0_only",
                                                         "wave_last_only", "powerlaw_cols", "one_dense_column",
                                                         "banded", "empty_shard")


def last_entry(W):
    """(k, n) of the highest k of W's last populated column."""
    n = int(np.flatnonzero(np.abs(W).sum(axis=0))[-1])
    return int(np.flatnonzero(W[:, n])[-1]), n


def blocked_w(W, B=B_BLOCKED):
    """W as a BlockedTCSC<B> handle holds it: the rows past the last whole block are not encoded."""
    Wb = W.copy()
    Wb[W.shape[0] // B * B:] = 0
    return Wb


# ---- the cases --------------------------------------------------------------------------------------

KERNEL = {"pc": "tsg_tcsc_ell_pc_kernel", "walk": "tsg_tcsc_ell_kernel", "rows64": "tsg_jit64_kernel",
          "rows128": "tsg_jit_kernel", "rx": "tsg_tcsc_rx_kernel", "blocked": "tsg_jit_kernel"}
KNOBS = ("TSG_JIT_HALF", "TSG_JIT_PAIR", "TSG_JIT_QBLOCK", "TSG_JIT_XDIRECT", "TSG_KERNEL")

Case = collections.namedtuple("Case", "w family M K N mode width knob B")

# (kernel family, M, small_m mode, width, knob, B, also at N_WIDE): the smallest M with a ragged
# second M tile (the walks: of their row tiles), as test_gpu_call_fuzz._FAMILY_SHAPE
_KERNELS = [("pc", 2, 0, 0, None, 0, False),
            ("walk", 16, 2, 0, None, 0, False),
            ("rows64", 65, 1, 128, None, 0, True),
            ("rows64", 65, 1, 16, None, 0, False),
            ("rows64", 65, 1, 8, None, 0, False),
            ("rows64", 65, 1, 16, "TSG_JIT_HALF", 0, False),
            ("rows64", 65, 1, 16, "TSG_JIT_PAIR", 0, False),
            ("rows64", 65, 1, 16, "TSG_JIT_QBLOCK=16", 0, False),
            ("rows128", 130, 1, 64, None, 0, True),
            ("rows128", 130, 1, 8, None, 0, False),
            ("rx", 70, 1, 0, None, 0, True),
            ("blocked", 70, 1, 0, None, B_BLOCKED, False)]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for w in FAMILY_NAMES:
        for family, M, mode, width, knob, B, wide in _KERNELS:
            for N in (N_SMALL, N_WIDE) if wide else (N_SMALL,):
                for K in KS:
                    out.append(Case(w, family, M, K, N, mode, width, knob, B))
            if family == "walk":
                out.append(Case(w, family, M, K_WALK_CHUNKED, N_SMALL, mode, width, knob, B))
    return tuple(out)


def case_id(c):
    tail = f"-w{c.width}" if c.width else ""
    tail += f"-{c.knob}" if c.knob else ""
    return f"{c.w}-{c.family}{tail}-{c.M}x{c.K}x{c.N}"


def jit_config(c):
    """The generated stream a jit case runs, as test_wstruct_ref.py emulates it: (image rows,
    width, waves, layout).  A pinned width runs 8 waves (tsg_plan.cpp pick_jit_shape), where
    TSG_JIT_HALF and TSG_JIT_PAIR -- knobs of the 4-wave shapes -- leave the stream as it is."""
    if c.family == "rows64":
        return (64, c.width, WAVES, "16" if c.knob == "TSG_JIT_QBLOCK=16" else "rows")
    if c.family == "rows128":
        return (128, c.width, WAVES, "pairs")
    if c.family == "blocked":
        return (128, 64, WAVES, f"B{c.B}")
    return None


def the_w(c):
    W = families(c.K, c.N)[c.w]
    return blocked_w(W, c.B) if c.B else W


@functools.lru_cache(maxsize=None)
def build(w, K, N, M, B):
    """(arrays, X, b, expected Y as uint32) of a case, computed once and read-only."""
    import oracle as O
    W = families(K, N)[w]
    X = O.init_x_frac(M, K, SEED + M)
    b = np.linspace(-3, 3, N).astype(F)
    if B:
        arrays = O.blocked_tcsc_encode(blocked_w(W, B), B)
        ref = O.base_blocked_tcsc(X, arrays, b, K, N, B)
    else:
        t = O.tcsc_encode(W)
        arrays = t.arrays
        ref = O.base_tcsc(X, t, b, threads=8 if M >= 8 else 0)
    want = ref.view(np.uint32)
    for a in (X, b, want):
        a.setflags(write=False)
    return arrays, X, b, want


def assert_bits(got, want, c, what):
    """The failure names the case's tuple, how many elements differ and the first few."""
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    first = [(int(m), int(n), hex(int(got[m, n])), hex(int(want[m, n]))) for m, n in bad[:6]]
    raise AssertionError(f"{tuple(c)}: {what} X: {len(bad)} of {want.size} elements differ; "
                         f"first (row, column, got, want): {first}")


def _handle(tsg, c, arrays):
    from test_gpu_ldy import _jit_handle
    M, K, N = c.M, c.K, c.N
    if c.family in ("rows64", "rows128"):
        rows = 64 if c.family == "rows64" else 128
        h = _jit_handle(tsg, arrays, K, N, rows, c.width)
        assert h.call_kernel(M) == KERNEL[c.family] and h.call_tile_rows(M) == rows, (c, h.call_kernel(M))
        assert h.jit_width(M) == c.width and h.jit_waves(M) == WAVES, (c, h.jit_width(M), h.jit_waves(M))
        return h
    if c.family == "blocked":
        h = tsg.TCSCDevice.from_blocked(*arrays, K, N, c.B)
    else:
        h = tsg.TCSCDevice(*arrays, K, N)
    h.set_small_m(c.mode)
    if c.family == "rx":
        assert h.kernel_name() == KERNEL["rx"], (c, h.kernel_name())
    assert h.call_kernel(M) == KERNEL[c.family], (c, h.call_kernel(M))
    if c.family in ("pc", "walk"):
        assert h.call_tile_rows(M) == 0, c
    return h


def _set_knobs(monkeypatch, c):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if c.family == "rx":
        monkeypatch.setenv("TSG_KERNEL", "rx")
    if c.knob:
        name, _, value = c.knob.partition("=")
        monkeypatch.setenv(name, value or "1")


@pytest.fixture(autouse=True)
def _oracle_built(oracle_mod):
    """The cached builders import the oracle themselves: it is built first."""


@pytest.mark.parametrize("c", cases(), ids=case_id)
def test_structured_w(tsg, monkeypatch, c):
    import torch
    from test_gpu_xtype import _x_on_device
    _set_knobs(monkeypatch, c)
    arrays, X, b, want = build(c.w, c.K, c.N, c.M, c.B)
    h = _handle(tsg, c, arrays)
    bd = torch.from_numpy(np.array(b)).cuda()
    Xt = torch.from_numpy(np.array(X))
    for xoff, what in ((0, "aligned"), (1, "one element off alignment")):
        Xd = _x_on_device(Xt, xoff)
        assert Xd.data_ptr() % 16 == 4 * xoff
        Y = h.gemm_torch(Xd, bd)
        torch.cuda.synchronize()
        assert_bits(Y.cpu().numpy().view(np.uint32), want, c, what)
        if c.family == "rows64" and c.knob != "TSG_JIT_QBLOCK=16":
            # the row layout reads an aligned X directly when K % 4 == 0 (one launch), else the staged copy
            assert h.call_launches(Xd, c.M) == (1 if c.K % 4 == 0 and xoff == 0 else 2), (c, what)
    h.close()


# ---- registration paths ----------------------------------------------------------------------------

ENCODER_FAMILIES = ("powerlaw_cols", "one_dense_column", "empty_shard", "last_row_only")


@pytest.mark.parametrize("w", ENCODER_FAMILIES)
def test_gpu_encoder_on_structured_w(tsg, oracle_mod, w):
    """tcsc_hip_encode_dense_dev == the host constructor's arrays, bit for bit."""
    import torch
    for K in KS:
        W = families(K, N_SMALL)[w]
        t = oracle_mod.tcsc_encode(W)
        g = tsg.encode_dense_torch(torch.from_numpy(np.array(W)).cuda())
        for a, d in zip(t.arrays, g):
            assert np.array_equal(np.asarray(a, np.int32), d.cpu().numpy()), (w, K)


@pytest.mark.parametrize("w", FAMILY_NAMES)
def test_registration_round_trips(tsg, oracle_mod, w):
    """from_dense, from_csc_packed (tcsc_hip_create_csc_packed) and to_dense give W back."""
    K, N = KS[0], N_SMALL
    W = families(K, N)[w]
    for h in (tsg.TCSCDevice.from_dense(W), tsg.TCSCDevice.from_csc_packed(*oracle_mod.csc_packed_encode(W), K, N)):
        assert np.array_equal(h.to_dense(), W), w
        info = h.info()
        assert (info["nnz_pos"], info["nnz_neg"]) == (np.count_nonzero(W == 1), np.count_nonzero(W == -1))
        h.close()


@pytest.mark.parametrize("M,mode", [(2, 0), (16, 2), (65, 1)])
def test_empty_slice_handle_gives_the_bias(tsg, oracle_mod, M, mode):
    """A handle registered from empty_shard's middle column slice -- a shard of W
    without an entry -- gives Y = b on the producer/consumer walk, the walk and
    the weight-compiled kernel."""
    import torch
    K, N = KS[0], N_SMALL
    t = oracle_mod.tcsc_encode(families(K, N)["empty_shard"])
    n0, n1 = N // 3, 2 * N // 3
    sl = tsg.tcsc_slice(*t.arrays, N, n0, n1)
    assert len(sl[2]) == 0 and len(sl[3]) == 0
    h = tsg.TCSCDevice(*sl, K, n1 - n0)
    h.set_small_m(mode)
    X = oracle_mod.init_x_frac(M, K, 5)
    b = np.linspace(-3, 3, n1 - n0).astype(F)
    Y = h.gemm_torch(torch.from_numpy(X).cuda(), torch.from_numpy(b).cuda())
    torch.cuda.synchronize()
    want = np.ascontiguousarray(np.broadcast_to(b, (M, n1 - n0)))
    assert np.array_equal(Y.cpu().numpy().view(np.uint32), want.view(np.uint32)), h.call_kernel(M)
    h.close()
