"""What lies next to X, b and alpha, and what the previous call left behind,
never reaches a result -- through every kernel family on the GPU, bit for bit
against the CPU oracle (no tolerance anywhere).

Poison is the quiet NaN 0x7FC5A5A5 (test_gpu_ldy.SENT), written through an
int32 view: one poisoned float that reaches an accumulator makes that output
NaN, while the oracle's output for init_x_frac X and finite b and alpha has
none (asserted once per shape).

A. Device-pointer calls whose X, b and alpha are views inside poisoned arenas
   (place), at every 4-byte offset from a 16-B boundary: a read past the last
   row of X, past b[N-1] or at k >= K of the last row that reached a result
   would show; the offsets run the scalar (misaligned-base) branches of the
   staging passes with K % 4 == 0.  Guards of 128 K + 1024 floats around X and
   4096 around b and alpha keep a tile's worth of dropped pad-row reads inside
   the allocation.
B. One handle, a call whose X is all NaN and has more rows, then the checked
   call: every real slot of the X^T work buffer (and LDS on the CUs that ran
   the first call) holds NaN, so a slot the second call reads without having
   written it shows.
C. The same through the host-pointer calls, whose device copies of X and Y
   persist across calls; and host operands at a 4-byte offset inside poisoned
   numpy arenas.

Every case asserts the path it names (call_kernel, jit_width, jit_waves,
call_tile_rows, call_launches), so that a planner change cannot turn it into
a copy of another case.

The tests establish that no value from outside [X, X + M K), [b, b + N),
[alpha, alpha + N) and no value of an earlier call reaches Y.  They do not
establish that no address outside those ranges is ever loaded."""
import functools

import numpy as np
import pytest

from test_gpu_ldy import SENT, _bits, _case, _dev
from test_gpu_special import _same

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _oracle_built(oracle_mod):
    """The cached cases below import the oracle themselves: it is built first."""


X_GUARD_ROWS, X_GUARD_EXTRA, VEC_GUARD = 128, 1024, 4096
SHIFTS = (0, 1, 2, 3)


# ---- arenas ----------------------------------------------------------------------

def place(arena, data, shift):
    """A device copy of `data` inside its own poisoned allocation: one 1-D
    float32 tensor filled with SENT, `data` at [g + shift, g + shift + size), g
    a multiple of 4 floats at least the guard size (so shift alone decides the
    16-B alignment), the same guard behind it.  The allocation is appended to
    the list `arena` for assert_inputs_untouched; returns the view, reshaped."""
    import torch
    data = np.asarray(data, np.float32)
    guard = X_GUARD_ROWS * data.shape[1] + X_GUARD_EXTRA if data.ndim == 2 else VEC_GUARD
    g = (guard + 3) // 4 * 4
    lo, hi = g + shift, g + shift + data.size
    buf = torch.empty(hi + g + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf.view(torch.int32).fill_(SENT)
    buf[lo:hi].copy_(torch.from_numpy(np.array(data).ravel()))
    arena.append((buf, lo, hi, data))
    view = buf[lo:hi].view(data.shape)
    assert view.data_ptr() % 16 == 4 * shift and view.is_contiguous()
    return view


def assert_inputs_untouched(arena, what):
    """Inputs are never written: every guard float still holds SENT and every
    payload its data."""
    import torch
    for buf, lo, hi, data in arena:
        bits = buf.view(torch.int32)
        assert bool((bits[:lo] == SENT).all()) and bool((bits[hi:] == SENT).all()), (what, "an input's guard was written")
        assert np.array_equal(_bits(buf[lo:hi]), data.ravel().view(np.uint32)), (what, "an input was written")


@functools.lru_cache(maxsize=None)
def _finite_case(M, K, N, B=0):
    """test_gpu_ldy._case, its oracle results checked once to hold no NaN."""
    case = _case(M, K, N, B)
    for ref in case[4:]:
        assert ref is None or not np.isnan(ref).any()
    return case


def run_placed(h, case, shift, what, launches=None):
    """One plain and one PReLU gemm_torch call with X, b and alpha placed
    (X at `shift`, b and alpha at the next two offsets); Y against the oracle."""
    import torch
    arrays, X, b, alpha, ref, ref_p = case
    M = X.shape[0]
    arena = []
    Xd = place(arena, X, shift)
    bd = place(arena, b, (shift + 1) % 4)
    ad = place(arena, alpha, (shift + 2) % 4)
    if launches is not None:
        assert h.call_launches(Xd, M) == launches, (what, shift, "launches")
    Y = h.gemm_torch(Xd, bd)
    Yp = h.gemm_torch(Xd, bd, alpha=ad)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Y), ref.view(np.uint32)), (what, shift, "plain != oracle",
                                                           int(np.isnan(Y.cpu().numpy()).sum()), "NaN outputs")
    if ref_p is not None:
        assert np.array_equal(_bits(Yp), ref_p.view(np.uint32)), (what, shift, "prelu != oracle",
                                                                  int(np.isnan(Yp.cpu().numpy()).sum()), "NaN outputs")
    assert_inputs_untouched(arena, (what, shift))
    return Y, Yp


# ---- A. operands inside a poisoned arena --------------------------------------------

@pytest.mark.parametrize("M,K,N", [(1, 384, 301), (4, 384, 301), (1, 385, 301), (4, 385, 700)])
def test_placed_pc_walk(tsg, M, K, N):
    """The producer/consumer walk: ell_stage's vector loads (K = 384, shift 0),
    its scalar loads on a misaligned base (shifts 1..3) and on K % 4 != 0."""
    case = _finite_case(M, K, N)
    h = tsg.TCSCDevice(*case[0], K, N)
    assert h.call_kernel(M) == "tsg_tcsc_ell_pc_kernel" and h.call_tile_rows(M) == 0
    for shift in SHIFTS:
        run_placed(h, case, shift, ("pc walk", M, K, N), launches=1)
    h.close()


@pytest.mark.parametrize("M,mode,K,N", [(16, 0, 384, 301), (4, 3, 384, 301), (16, 0, 385, 301), (4, 3, 385, 700),
                                        (16, 0, 384, 700)])
def test_placed_ell_walk(tsg, M, mode, K, N):
    """The ELL walk: M = 16 as planned, M = 4 with the producer/consumer walk
    switched off."""
    case = _finite_case(M, K, N)
    h = tsg.TCSCDevice(*case[0], K, N)
    h.set_small_m(mode)
    assert h.call_kernel(M) == "tsg_tcsc_ell_kernel" and h.call_tile_rows(M) == 0
    for shift in SHIFTS:
        run_placed(h, case, shift, ("ell walk", M, K, N), launches=1)
    h.close()


def _direct_k_ok(K, piece_rows):
    """K lets the 64-row image read X itself: the row layout (piece_rows 0)
    needs K >= 188 and K % 4 == 0, the blocked layout no piece across K."""
    return (K >= 188 and K % 4 == 0) if piece_rows == 0 else K % (256 // piece_rows) == 0


# (stream shape, M, K, N, TSG_JIT_QBLOCK): a width runs 8 waves; "auto", "half"
# and "pair" are the automatic 4-wave shape, plain, with TSG_JIT_HALF=1 and
# with TSG_JIT_PAIR=1.  Row layout: K = 380 (last chunk moved back to K - 188),
# 188 (one chunk), 376 (two whole chunks), 385 (staged only, the k >= K tail
# next to poison); blocked layout (QBLOCK 16 / 8): K = 384.
ROWS64 = [
    (128, 63, 380, 301, None), (64, 64, 380, 301, None), (32, 65, 380, 301, None), (16, 130, 380, 301, None),
    (8, 63, 380, 301, None), ("auto", 65, 380, 301, None), ("half", 130, 380, 301, None), ("pair", 64, 380, 301, None),
    (64, 65, 380, 700, None),
    (64, 65, 188, 301, None), ("pair", 63, 188, 301, None), (128, 64, 376, 301, None), (32, 130, 376, 301, None),
    (16, 65, 385, 301, None), ("auto", 130, 385, 301, None), (128, 63, 385, 301, None),
    (64, 63, 384, 301, "16"), ("auto", 65, 384, 301, "16"), (8, 130, 384, 301, "16"),
    (32, 64, 384, 301, "8"), ("auto", 65, 384, 301, "8"), (128, 130, 384, 301, "8"),
    ("half", 63, 384, 301, None),  # the half ring's 16-row pieces straight from X
]


@pytest.mark.parametrize("shape,M,K,N,qblock", ROWS64)
def test_placed_rows64(tsg, monkeypatch, shape, M, K, N, qblock):
    """The 64-row image, X read by its own DMA (TSG_JIT_XDIRECT=1, shift 0, K
    allows it: one launch -- rows past M clamped to M-1, the base 3 KiB below
    X, the last row-layout chunk moved back) and through the staged copy
    (TSG_JIT_XDIRECT=0, or X at a 4-byte offset: two launches)."""
    for k in ("TSG_JIT_HALF", "TSG_JIT_PAIR", "TSG_JIT_QBLOCK", "TSG_JIT_XDIRECT"):
        monkeypatch.delenv(k, raising=False)
    if qblock:
        monkeypatch.setenv("TSG_JIT_QBLOCK", qblock)
    if shape in ("half", "pair"):
        monkeypatch.setenv("TSG_JIT_" + shape.upper(), "1")
    case = _finite_case(M, K, N)
    h = tsg.TCSCDevice(*case[0], K, N)
    h.set_small_m(1)
    h.set_tile_rows(64)
    if isinstance(shape, int):
        h.set_jit_width(shape)
        assert h.jit_width(M) == shape and h.jit_waves(M) == 8
    else:
        assert h.jit_waves(M) == 4, (h.jit_width(M), h.jit_waves(M))
    assert h.call_kernel(M) == "tsg_jit64_kernel" and h.call_tile_rows(M) == 64
    # the half ring has no row layout: 16-row pieces unless TSG_JIT_QBLOCK says 8
    piece_rows = int(qblock) if qblock else 16 if shape == "half" else 0
    for direct in ("1", "0"):
        monkeypatch.setenv("TSG_JIT_XDIRECT", direct)
        for shift in (0, 1):
            one = direct == "1" and shift == 0 and _direct_k_ok(K, piece_rows)
            run_placed(h, case, shift, ("rows64", shape, M, K, N, qblock, "direct=" + direct),
                       launches=1 if one else 2)
    h.close()


# (width, far, M, K, N): width 0 = the automatic 4-wave shape
ROWS128 = [(64, 0, 127, 384, 301), (32, 0, 128, 384, 301), (16, 0, 130, 384, 301), (8, 0, 127, 384, 301),
           (0, 0, 130, 384, 301), (64, 2, 130, 384, 301), (64, 0, 130, 385, 301), (0, 0, 127, 385, 301),
           (32, 0, 130, 384, 700), (64, 2, 127, 385, 700)]


@pytest.mark.parametrize("width,far,M,K,N", ROWS128)
def test_placed_rows128(tsg, width, far, M, K, N):
    """The 128-row image and its far-X^T image: the k-pair staging pass, vector
    (shift 0, K = 384) and scalar (shifts 1 and 3; K = 385)."""
    case = _finite_case(M, K, N)
    h = tsg.TCSCDevice(*case[0], K, N)
    h.set_small_m(1)
    h.set_tile_rows(128)
    if width:
        h.set_jit_width(width)
    h.set_far(far)
    assert h.call_kernel(M) == "tsg_jit_kernel" and h.call_tile_rows(M) == 128
    assert h.call_far(M) == (far == 2)
    if width:
        assert h.jit_width(M) == width and h.jit_waves(M) == 8
    else:
        assert h.jit_waves(M) == 4, (h.jit_width(M), h.jit_waves(M))
    for shift in (0, 1, 3):
        run_placed(h, case, shift, ("rows128", width, far, M, K, N), launches=2)
    h.close()


@pytest.mark.parametrize("M,K,N", [(5, 384, 301), (130, 384, 301), (130, 385, 301), (5, 385, 700)])
def test_placed_rx_kernel(tsg, monkeypatch, M, K, N):
    """The rx kernel behind its plain X^T pass (float4 at shift 0 and K = 384,
    scalar otherwise)."""
    monkeypatch.setenv("TSG_KERNEL", "rx")
    case = _finite_case(M, K, N)
    h = tsg.TCSCDevice(*case[0], K, N)
    h.set_small_m(1)
    assert h.kernel_name() == "tsg_tcsc_rx_kernel" and h.call_kernel(M) == "tsg_tcsc_rx_kernel"
    assert h.call_tile_rows(M) == 0 and h.jit_width(M) == 0
    for shift in (0, 1):
        run_placed(h, case, shift, ("rx", M, K, N), launches=2)
    h.close()


@functools.lru_cache(maxsize=None)
def _blocked_int_case(M, K, N, B):
    """The blocked shape's W with integer X and b, for the PReLU check: with
    integer data every partial sum is exact, so the block order cannot change a
    bit and the plain TCSC of W's encoded rows (BlockedTCSC drops the rows past
    (K / B) B) computes BaseBlockedTCSC bit for bit -- asserted here on the
    CPU -- and base_tcsc_prelu on it pins the blocked PReLU result."""
    import oracle as O
    W = O.gen_ternary(K, N, 4, 1000 * M + K + N)  # _case's W
    blk = O.blocked_tcsc_encode(W, B)
    assert all(np.array_equal(a, c) for a, c in zip(blk, _case(M, K, N, B)[0]))
    Wt = W.copy()
    Wt[(K // B) * B:] = 0
    t = O.tcsc_encode(Wt)
    X = O.init_x_int(M, K, M + 13)
    b = (np.arange(N) % 13 - 6).astype(np.float32)
    alpha = np.linspace(-0.5, 0.5, N).astype(np.float32)
    ref, ref_p = O.base_tcsc(X, t, b), O.base_tcsc_prelu(X, t, b, alpha)
    assert np.array_equal(O.base_blocked_tcsc(X, blk, b, K, N, B).view(np.uint32), ref.view(np.uint32))
    assert not np.isnan(ref_p).any() and (ref_p != ref).any()
    for a in (X, b, alpha, ref, ref_p):
        a.setflags(write=False)
    return t.arrays, X, b, alpha, ref, ref_p


@pytest.mark.parametrize("M,K,N,B", [(130, 384, 301, 64), (130, 385, 301, 64), (130, 384, 700, 64)])
def test_placed_blocked_handle(tsg, M, K, N, B):
    """BlockedTCSC: the plain call against base_blocked_tcsc (fractional X);
    the PReLU call, for integer X and b, against base_tcsc_prelu and the
    plain-TCSC handle's PReLU result (_blocked_int_case)."""
    import torch
    case = _finite_case(M, K, N, B)
    h = tsg.TCSCDevice.from_blocked(*case[0], K, N, B)
    h.set_small_m(1)
    assert h.call_kernel(M) == "tsg_jit_kernel" and h.call_tile_rows(M) == 128
    assert h.jit_width(M) == 64 and h.jit_waves(M) == 8
    icase = _blocked_int_case(M, K, N, B)
    hp = tsg.TCSCDevice(*icase[0], K, N)
    hp.set_small_m(1)
    hp.set_tile_rows(128)
    assert hp.call_kernel(M) == "tsg_jit_kernel"
    for shift in (0, 1):
        run_placed(h, case, shift, ("blocked", M, K, N, B), launches=2)   # plain: oracle; PReLU: runs, no reference
        blocked = run_placed(h, (None,) + icase[1:], shift, ("blocked, integer X", M, K, N, B), launches=2)
        plain = run_placed(hp, icase, shift, ("plain TCSC, integer X", M, K, N), launches=2)
        for yb, yp in zip(blocked, plain):
            assert torch.equal(yb.view(torch.int32), yp.view(torch.int32)), (shift, "blocked != plain TCSC handle")
    h.close()
    hp.close()


# ---- B. a NaN call before the checked call ------------------------------------------

PM = 300  # the poisoner's rows


@functools.lru_cache(maxsize=None)
def _weights(K, N, B=0):
    import oracle as O
    W = O.gen_ternary(K, N, 4, 7 * K + N)
    return (O.blocked_tcsc_encode(W, B), None) if B else (O.tcsc_encode(W).arrays, O.tcsc_encode(W))


@functools.lru_cache(maxsize=None)
def _shared_case(M, K, N, B=0, nan=False):
    """X (init_x_frac, or all SENT), b, alpha and the oracle's results for M
    rows against the one W of (K, N): the cases of one handle."""
    import oracle as O
    arrays, t = _weights(K, N, B)
    X = np.full((M, K), SENT, np.uint32).view(np.float32) if nan else O.init_x_frac(M, K, M + 11)
    b = np.linspace(-3, 3, N).astype(np.float32)
    alpha = np.linspace(-0.5, 0.5, N).astype(np.float32)
    if B:
        ref, ref_p = O.base_blocked_tcsc(X, arrays, b, K, N, B), None
    else:
        ref, ref_p = O.base_tcsc(X, t, b), O.base_tcsc_prelu(X, t, b, alpha)
    if nan:
        assert np.isnan(ref).any()
    else:
        assert not np.isnan(ref).any() and (ref_p is None or not np.isnan(ref_p).any())
    for a in (X, b, alpha, ref) + ((ref_p,) if ref_p is not None else ()):
        a.setflags(write=False)
    return X, b, alpha, ref, ref_p


def _cfg(kernel, M, rows=0, width=0, far=0, small_m=1, direct=None, half=False, waves=None, launches=None, bare=False):
    return dict(kernel=kernel, M=M, rows=rows, width=width, far=far, small_m=small_m, direct=direct, half=half,
                waves=waves, launches=launches, bare=bare)


def r64(M, width=0, direct="0", **kw):
    return _cfg("tsg_jit64_kernel", M, rows=64, width=width, direct=direct, **kw)


def r128(M, width=0, far=0, **kw):
    return _cfg("tsg_jit_kernel", M, rows=128, width=width, far=far, **kw)


def walk(M):
    return _cfg("tsg_tcsc_ell_pc_kernel" if M <= 4 else "tsg_tcsc_ell_kernel", M, small_m=0, launches=1)


def _apply(h, monkeypatch, c, Xd=None):
    """Set the handle (and the per-call knobs) to configuration c and assert
    that a call with c's M then runs what c names."""
    M = c["M"]
    h.set_small_m(c["small_m"])
    if not c["bare"]:
        h.set_tile_rows(c["rows"])
        h.set_jit_width(c["width"])
        h.set_far(c["far"])
    for knob, v in (("TSG_JIT_XDIRECT", c["direct"]), ("TSG_JIT_HALF", "1" if c["half"] else None)):
        if v is None:
            monkeypatch.delenv(knob, raising=False)
        else:
            monkeypatch.setenv(knob, v)
    assert h.call_kernel(M) == c["kernel"], (c, h.call_kernel(M))
    if not c["bare"]:
        assert h.call_tile_rows(M) == c["rows"], c
        assert h.call_far(M) == (c["far"] == 2), c
        if c["width"]:
            assert h.jit_width(M) == c["width"] and h.jit_waves(M) == 8, c
        elif c["rows"]:
            assert h.jit_waves(M) == (c["waves"] or 4), (c, h.jit_width(M), h.jit_waves(M))
    if c["launches"] is not None and Xd is not None:
        assert h.call_launches(Xd, M) == c["launches"], c


def poison_then_check(h, monkeypatch, K, N, poisoner, victims, B=0):
    """For each victim: the poisoner's call (X all NaN, PM rows; its own Y
    checked the first time, NaN positions against the oracle), then the victim's
    call on the same handle, bit for bit against the oracle; plain, then the
    same again for PReLU."""
    import torch
    Xn, b, alpha, refn, _ = _shared_case(poisoner["M"], K, N, B, True)
    Xnd, bd, ad = _dev(Xn), _dev(b), _dev(alpha)
    _apply(h, monkeypatch, poisoner, Xnd)
    h.reserve(poisoner["M"])  # the work buffer at its final size: no victim gets a fresh one
    checked = False
    for v in victims:
        X, _, _, ref, ref_p = _shared_case(v["M"], K, N, B)
        Xd = _dev(X)
        for al, want in ((None, ref), (ad, ref_p)):
            if want is None:
                continue
            _apply(h, monkeypatch, poisoner, Xnd)
            Yn = h.gemm_torch(Xnd, bd)
            _apply(h, monkeypatch, v, Xd)
            Y = h.gemm_torch(Xd, bd, alpha=al)
            torch.cuda.synchronize()
            if not checked:
                _same(Yn.cpu().numpy(), refn)
                checked = True
            got = Y.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (
                "after", poisoner, "the call", v, "prelu" if al is not None else "plain", "!= oracle",
                int(np.isnan(got).sum()), "NaN outputs")


def _plain_handle(tsg, K, N):
    return tsg.TCSCDevice(*_weights(K, N)[0], K, N)


KS = (380, 385)
N_B = 301


@pytest.mark.parametrize("K", KS)
def test_stale_rows128_then_rows64_staged(tsg, monkeypatch, K):
    """k-pair X^T of 300 NaN rows, then the 64-row image's staged layout."""
    h = _plain_handle(tsg, K, N_B)
    poison_then_check(h, monkeypatch, K, N_B, r128(PM, width=64), [r64(M, launches=2) for M in (1, 63, 65, 130)])
    h.close()


@pytest.mark.parametrize("K", KS)
def test_stale_rows64_staged_then_rows128(tsg, monkeypatch, K):
    h = _plain_handle(tsg, K, N_B)
    poison_then_check(h, monkeypatch, K, N_B, r64(PM, width=64, launches=2), [r128(M) for M in (5, 127, 130)])
    h.close()


@pytest.mark.parametrize("K", KS)
def test_stale_rows128_wide_then_narrow(tsg, monkeypatch, K):
    """The same k-pair layout with a smaller Mp, read by other stream shapes."""
    h = _plain_handle(tsg, K, N_B)
    poison_then_check(h, monkeypatch, K, N_B, r128(PM, width=64), [r128(130, width=8), r128(130)])
    h.close()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("far_first", [True, False])
def test_stale_far_and_regular_image(tsg, monkeypatch, K, far_first):
    h = _plain_handle(tsg, K, N_B)
    a, c = (2, 1) if far_first else (1, 2)
    poison_then_check(h, monkeypatch, K, N_B, r128(PM, width=64, far=a), [r128(130, width=64, far=c)])
    h.close()


@pytest.mark.parametrize("K", KS)
def test_stale_rows64_row_layout_smaller_mp(tsg, monkeypatch, K):
    """The staged row layout, then the same layout with a smaller Mp."""
    monkeypatch.delenv("TSG_JIT_QBLOCK", raising=False)
    h = _plain_handle(tsg, K, N_B)
    poison_then_check(h, monkeypatch, K, N_B, r64(PM, width=64, launches=2), [r64(65, width=64, launches=2),
                                                                             r64(65, launches=2)])
    h.close()


@pytest.mark.parametrize("K", KS)
def test_stale_rx_handle(tsg, monkeypatch, K):
    monkeypatch.setenv("TSG_KERNEL", "rx")
    h = _plain_handle(tsg, K, N_B)
    assert h.kernel_name() == "tsg_tcsc_rx_kernel"
    rx = functools.partial(_cfg, "tsg_tcsc_rx_kernel", bare=True, launches=2)
    poison_then_check(h, monkeypatch, K, N_B, rx(PM), [rx(5), rx(130)])
    h.close()


@pytest.mark.parametrize("K", KS)
def test_stale_blocked_handle(tsg, monkeypatch, K):
    B = 64
    h = tsg.TCSCDevice.from_blocked(*_weights(K, N_B, B)[0], K, N_B, B)
    blocked = functools.partial(_cfg, "tsg_jit_kernel", bare=True, launches=2)
    poison_then_check(h, monkeypatch, K, N_B, blocked(PM), [blocked(130)], B=B)
    h.close()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows", [128, 64])
def test_stale_lds_then_walks_and_direct_x(tsg, monkeypatch, K, rows):
    """Victims that use no work buffer, right after a kernel that filled LDS
    with NaN on every CU it ran on: the walks (zero rows, never-staged ring
    slots) and the 64-row image reading X itself (K = 380; K = 385 cannot)."""
    monkeypatch.delenv("TSG_JIT_QBLOCK", raising=False)
    h = _plain_handle(tsg, K, N_B)
    poisoner = r128(PM, width=64) if rows == 128 else r64(PM, width=128, launches=2)
    victims = [walk(1), walk(4), walk(16)]
    if _direct_k_ok(K, 0):
        victims += [r64(65, width=64, direct="1", launches=1), r64(130, direct="1", launches=1),
                    r64(63, width=128, direct="1", launches=1)]
    poison_then_check(h, monkeypatch, K, N_B, poisoner, victims)
    h.close()


@pytest.mark.parametrize("K", KS)
def test_stale_work_buffer_under_graph_replay(tsg, monkeypatch, K):
    """A captured staged 64-row call (M = 65, after reserve(300)), an
    uncaptured NaN call with 300 rows on the same handle, then the replay."""
    import torch
    M = 65
    h = _plain_handle(tsg, K, N_B)
    X, b, alpha, ref, ref_p = _shared_case(M, K, N_B)
    Xn, _, _, refn, _ = _shared_case(PM, K, N_B, 0, True)
    Xd, Xnd, bd, ad = _dev(X), _dev(Xn), _dev(b), _dev(alpha)
    victim, poisoner = r64(M, width=64, launches=2), r128(PM, width=64)
    _apply(h, monkeypatch, poisoner, Xnd)
    h.reserve(PM)
    _apply(h, monkeypatch, victim, Xd)
    h.reserve(PM)
    Y = torch.empty((M, N_B), device="cuda")
    Yp = torch.empty((M, N_B), device="cuda")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        h.gemm_torch(Xd, bd, Y)  # warm
        h.gemm_torch(Xd, bd, Yp, alpha=ad)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            h.gemm_torch(Xd, bd, Y)
            h.gemm_torch(Xd, bd, Yp, alpha=ad)
    torch.cuda.synchronize()
    _apply(h, monkeypatch, poisoner, Xnd)
    Yn = h.gemm_torch(Xnd, bd)
    torch.cuda.synchronize()
    _same(Yn.cpu().numpy(), refn)
    Y.view(torch.int32).fill_(SENT)
    Yp.view(torch.int32).fill_(SENT)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Y), ref.view(np.uint32)), "replay after a NaN call != oracle"
    assert np.array_equal(_bits(Yp), ref_p.view(np.uint32)), "PReLU replay after a NaN call != oracle"
    h.close()


# ---- C. host-pointer path ------------------------------------------------------------

HOST_PM = 700


@pytest.mark.parametrize("chunks", [3, 1])
@pytest.mark.parametrize("direct", [False, True])
def test_host_calls_after_nan_call(tsg, monkeypatch, chunks, direct):
    """The handle's device copies of X and Y keep the largest call's size: after
    a 700-row NaN call (chunked pipeline, and unchunked) smaller calls find NaN
    behind their X -- read by the 64-row image's own DMA when `direct` -- and in
    the rest of Y."""
    K, N = 380, N_B
    monkeypatch.delenv("TSG_JIT_QBLOCK", raising=False)
    h = _plain_handle(tsg, K, N)
    if direct:
        monkeypatch.setenv("TSG_JIT_XDIRECT", "1")
        h.set_small_m(1)
        h.set_tile_rows(64)
    else:
        monkeypatch.delenv("TSG_JIT_XDIRECT", raising=False)
        h.set_small_m(0)
    h.set_host_chunks(chunks)
    assert (h.host_chunk_rows(HOST_PM) < HOST_PM) == (chunks > 1)
    Xn, b, alpha, refn, _ = _shared_case(HOST_PM, K, N, 0, True)
    for M in (1, 5, 63, 300):
        if direct:  # the device copy of X is 16-B aligned (address 0 stands for it)
            assert h.call_kernel(M) == "tsg_jit64_kernel" and h.call_launches(0, M) == 1
        X, _, _, ref, ref_p = _shared_case(M, K, N)
        _same(h.gemm(Xn, b), refn)
        Y = h.gemm(X, b)
        assert np.array_equal(Y.view(np.uint32), ref.view(np.uint32)), (M, chunks, direct, int(np.isnan(Y).sum()))
        _same(h.gemm(Xn, b), refn)
        Yp = h.gemm_prelu(X, b, alpha)
        assert np.array_equal(Yp.view(np.uint32), ref_p.view(np.uint32)), (M, chunks, direct, int(np.isnan(Yp).sum()))
    h.close()


def _host_place(data, extra=64):
    """A C-contiguous float32 view of `data` at a 4-byte offset from a 16-B
    boundary inside a SENT-filled numpy arena; returns (arena bits, view, lo)."""
    data = np.asarray(data, np.float32)
    bits = np.full(data.size + 2 * extra, SENT, np.uint32)
    lo = extra + (1 - (bits.ctypes.data // 4 + extra)) % 4
    view = bits[lo:lo + data.size].view(np.float32).reshape(data.shape)
    view[...] = data
    assert view.ctypes.data % 16 == 4 and view.flags.c_contiguous
    return bits, view, lo


@pytest.mark.parametrize("M", [5, 130])
def test_host_operands_at_4_byte_offset(tsg, M):
    K, N = 380, N_B
    h = _plain_handle(tsg, K, N)
    X, b, alpha, ref, ref_p = _shared_case(M, K, N)
    arenas = [_host_place(a) for a in (X, b, alpha, np.zeros((M, N), np.float32))]
    (_, Xv, _), (_, bv, _), (_, av, _), (ybits, Yv, ylo) = arenas
    for want, call in ((ref, lambda: h(Xv, bv, Yv, M, N, K)), (ref_p, lambda: h.prelu(Xv, bv, av, Yv, M, N, K))):
        Yv.view(np.uint32)[...] = SENT
        call()
        assert np.array_equal(Yv.view(np.uint32), want.view(np.uint32)), (M, int(np.isnan(Yv).sum()))
        assert (ybits[:ylo] == SENT).all() and (ybits[ylo + M * N:] == SENT).all(), "wrote outside Y"
    for (bits, view, lo), data in zip(arenas[:3], (X, b, alpha)):
        assert (bits[:lo] == SENT).all() and (bits[lo + data.size:] == SENT).all()
        assert np.array_equal(view.view(np.uint32), data.view(np.uint32)), "an input was written"
    h.close()
