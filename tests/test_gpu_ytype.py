"""fp16 and bf16 Y on the device-pointer calls (tcsc_hip_gemm_dev_xy,
TCSCDevice.gemm_torch_xy) through every kernel family on the GPU.

The contract: Y equals, bit for bit, the element-wise round-to-nearest-even
cast of the fp32 call's Y.  So the expectation everywhere is the CPU oracle's
fp32 result (on the widened X) cast with torch's CPU .to(dtype), compared as
16-bit integers with no tolerance; the fp32 call on the same handle is checked
against the oracle too, so a mismatch can be told apart: the chain or the
rounding.

Inputs.  X is test_gpu_xtype's (init_x_frac, order-sensitive, rounded to the X
type; int8 draws).  init_x_frac reaches 2^23, so for an fp16 Y the source of X
is first scaled by a power of two -- exact, the chain's roundings do not move
-- chosen from the unscaled oracle result so that the expected array holds no
inf and no NaN (asserted).  In every general case at least a quarter of the
fp32 results are not representable in the Y type (asserted): the case rounds.

Each case asserts the kernel family that ran, then runs a plain and a PReLU
call into: a dense [M, N] output (N = 700: rows alternate between 16-byte
aligned and 8-byte offset starts, so both store widths run; N = 301 more so),
the view rows 1..M, columns 1..N+1 of an [M + 2, N + 3] buffer filled with a
16-bit NaN pattern (odd ldY, odd element offset: every edge of the view shares
a dword with a sentinel), and an all-aligned view (ldY = 704, column 0).  Only
the view may change."""
import functools

import numpy as np
import pytest

from test_gpu_ldy import _bits, _case, _dev, _jit_handle
from test_gpu_xtype import _identity_tcsc, _tdtype

pytestmark = pytest.mark.gpu

YDTYPES = ("float16", "bfloat16")
XDTYPES = ("float32", "float16", "bfloat16", "int8")
XY = [(x, y) for x in ("float32", "bfloat16") for y in YDTYPES]
XY_ALL = [(x, y) for x in XDTYPES for y in YDTYPES]

# a NaN in both 16-bit types with a payload no arithmetic produces
SENT16 = 0x7FC5
# the largest finite value of the Y type
YMAX = {"float16": 65504.0, "bfloat16": float(np.uint32(0x7F7F0000).view(np.float32))}


@pytest.fixture(autouse=True)
def _oracle_built(oracle_mod):
    """The cached cases below import the oracle themselves: it is built first."""


def _cast_bits(a32, ydtype):
    """fp32 numpy -> the Y type with torch's CPU cast, as uint16 bits."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a32)).to(_tdtype(ydtype))
    return t.view(torch.int16).numpy().view(np.uint16)


def _ybits(t):
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _exact_fraction(a32, ydtype):
    """Share of the fp32 values that the Y type holds exactly."""
    import torch
    back = torch.from_numpy(np.ascontiguousarray(a32)).to(_tdtype(ydtype)).to(torch.float32).numpy()
    return float(np.mean(back == a32))


def _x_for(M, K, xdtype, seed, shift):
    """(X in its type as a CPU tensor, X widened to fp32): init_x_frac * 2^-shift
    rounded to the type; int8: integer draws (never scaled)."""
    import torch
    import oracle as O
    if xdtype == "int8":
        Xt = torch.from_numpy(np.random.default_rng(seed).integers(-127, 128, size=(M, K)).astype(np.int8))
    else:
        X = O.init_x_frac(M, K, seed)
        s = shift + (8 if xdtype == "float16" else 0)  # fp16 X: |X| <= 2^15 fits the type
        X = X * np.float32(2.0 ** -s)                  # exact
        Xt = torch.from_numpy(X) if xdtype == "float32" else torch.from_numpy(X).to(_tdtype(xdtype))
    Xw = Xt.to(torch.float32).numpy()
    assert Xw.shape == (M, K) and np.isfinite(Xw).all()
    return Xt, Xw


@functools.lru_cache(maxsize=None)
def _ycase(M, K, N, xdtype, ydtype, B=0):
    """W (test_gpu_ldy._case's for the shape), X in its type, b, alpha, the
    oracle's fp32 results on the widened X and their casts to the Y type:
    computed once, never modified.  The input conditions of the module
    docstring are asserted here (CPU only)."""
    import oracle as O
    W = O.gen_ternary(K, N, 4, 1000 * M + K + N)
    b = np.linspace(-3, 3, N).astype(np.float32)
    alpha = np.linspace(-0.5, 0.5, N).astype(np.float32)
    if B:
        arrays = O.blocked_tcsc_encode(W, B)
        run = lambda Xw: (O.base_blocked_tcsc(Xw, arrays, b, K, N, B), None)  # (the oracle has no blocked PReLU)
    else:
        t = O.tcsc_encode(W)
        arrays = t.arrays
        run = lambda Xw: (O.base_tcsc(Xw, t, b), O.base_tcsc_prelu(Xw, t, b, alpha))
    shift = 0
    if ydtype == "float16" and xdtype != "int8":
        # the power of two that brings the unscaled result's largest magnitude
        # under 2^15 (the bias, |b| <= 3, is not scaled: 2^15 + 3 < 65504)
        ref0, _ = run(_x_for(M, K, xdtype, M + 11, 0)[1])
        top = float(np.abs(ref0.astype(np.float64)).max())
        shift = max(0, int(np.ceil(np.log2(top / 2.0 ** 15)))) if top > 0 else 0
    Xt, Xw = _x_for(M, K, xdtype, M + 11, shift)
    ref, ref_p = run(Xw)
    want = {}
    for name, r in (("plain", ref), ("prelu", ref_p)):
        if r is None:
            continue
        assert np.isfinite(r).all() and float(np.abs(r).max()) <= YMAX[ydtype], (name, "expected array overflows")
        wb = _cast_bits(r, ydtype)
        back = torch_from_bits(wb, ydtype)
        assert np.isfinite(back).all(), (name, "expected array holds inf or NaN")
        assert _exact_fraction(r, ydtype) <= 0.75, (name, "the case exercises no rounding", _exact_fraction(r, ydtype))
        wb.setflags(write=False)
        want[name] = wb
    for a in (Xw, b, alpha, ref) + ((ref_p,) if ref_p is not None else ()):
        a.setflags(write=False)
    return arrays, Xt, Xw, b, alpha, ref, ref_p, want


def torch_from_bits(bits16, ydtype):
    """uint16 bits of the Y type -> fp32 numpy."""
    import torch
    return torch.from_numpy(bits16.view(np.int16).copy()).view(_tdtype(ydtype)).to(torch.float32).numpy()


def _fill16(buf):
    import torch
    buf.view(torch.int16).fill_(SENT16)


def _assert_only_view_written16(buf, r0, r1, c0, c1, what):
    """Every 16-bit element of buf outside buf[r0:r1, c0:c1] still holds the sentinel."""
    import torch
    bits = buf.view(torch.int16).clone()
    bits[r0:r1, c0:c1] = SENT16
    wrong = (bits != SENT16).nonzero()
    assert wrong.numel() == 0, (what, "wrote outside the view at (row, col)", wrong[:8].tolist())


def _views(M, N, ydtype):
    """name -> (buffer, view, (r0, r1, c0, c1)): the three outputs of a case."""
    import torch
    dt = _tdtype(ydtype)
    la = 704 if N <= 704 else 8 * ((N + 7) // 8)
    out = {}
    dense = torch.empty((M + 2, N), dtype=dt, device="cuda")
    out["dense"] = (dense, dense[1:M + 1], (1, M + 1, 0, N))
    odd = torch.empty((M + 2, N + 3), dtype=dt, device="cuda")
    out["odd"] = (odd, odd[1:M + 1, 1:N + 1], (1, M + 1, 1, N + 1))
    al = torch.empty((M + 2, la), dtype=dt, device="cuda")
    assert al.data_ptr() % 16 == 0 and (la * 2) % 16 == 0
    out["aligned"] = (al, al[1:M + 1, 0:N], (1, M + 1, 0, N))
    return out


def check_y(h, case, ydtype, what):
    """The shared scheme (module docstring) for one handle and one case."""
    import torch
    arrays, Xt, Xw, b, alpha, ref, ref_p, want = case
    M, N = Xt.shape[0], b.shape[0]
    Xd, bd, ad = Xt.cuda(), _dev(b), _dev(alpha)
    keep = Xd.clone()
    # the chain: the fp32 call on the same handle is the oracle's
    Y32 = h.gemm_torch_x(Xd, bd)
    Y32p = h.gemm_torch_x(Xd, bd, alpha=ad)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Y32), ref.view(np.uint32)), (what, "fp32 call != oracle")
    if ref_p is not None:
        assert np.array_equal(_bits(Y32p), ref_p.view(np.uint32)), (what, "fp32 PReLU call != oracle")
    dt = _tdtype(ydtype)
    for al, key, y32 in ((None, "plain", Y32), (ad, "prelu", Y32p)):
        # (blocked handles: the oracle has no PReLU; the fp32 call's cast stands in)
        wb = want[key] if key in want else _cast_bits(y32.cpu().numpy(), ydtype)
        tag0 = (what, ydtype, key)
        Y = h.gemm_torch_xy(Xd, bd, alpha=al, out_dtype=dt)
        torch.cuda.synchronize()
        assert Y.dtype == dt and tuple(Y.shape) == (M, N) and Y.is_contiguous()
        got = _ybits(Y)
        assert np.array_equal(got, wb), (tag0, "new dense Y", int((got != wb).sum()), "elements differ")
        for name, (buf, view, box) in _views(M, N, ydtype).items():
            tag = tag0 + (name,)
            _fill16(buf)
            out = h.gemm_torch_xy(Xd, bd, view, alpha=al)
            torch.cuda.synchronize()
            assert out is view
            got = _ybits(view)
            assert np.array_equal(got, wb), (tag, int((got != wb).sum()), "elements differ")
            _assert_only_view_written16(buf, *box, tag)
    assert torch.equal(Xd.view(torch.int8), keep.view(torch.int8)), (what, "X was written")


# ---- every kernel family ----------------------------------------------------

@pytest.mark.parametrize("xdtype,ydtype", XY)
@pytest.mark.parametrize("M,K,N,mode,kernel", [(1, 193, 301, 0, "tsg_tcsc_ell_pc_kernel"),
                                               (4, 388, 700, 0, "tsg_tcsc_ell_pc_kernel"),
                                               (4, 388, 700, 3, "tsg_tcsc_ell_kernel"),
                                               (16, 193, 301, 0, "tsg_tcsc_ell_kernel")])
def test_ytype_small_m_walks(tsg, xdtype, ydtype, M, K, N, mode, kernel):
    """The producer/consumer walk and the ELL walk: one 2-byte store per element."""
    case = _ycase(M, K, N, xdtype, ydtype)
    h = tsg.TCSCDevice(*case[0], K, N)
    h.set_small_m(mode)
    assert h.call_kernel(M) == kernel and h.call_tile_rows(M) == 0
    check_y(h, case, ydtype, (kernel, M, K, N, xdtype))
    h.close()


@pytest.mark.parametrize("xdtype,ydtype", XY)
@pytest.mark.parametrize("width,M,K,N", [(128, 63, 193, 700), (16, 65, 388, 700), (8, 130, 193, 301)])
def test_ytype_rows64_widths(tsg, xdtype, ydtype, width, M, K, N):
    """The 64-row image at widths 128, 16 and 8 (8 waves); width 8 is exactly
    one 16-byte store per row segment."""
    case = _ycase(M, K, N, xdtype, ydtype)
    h = _jit_handle(tsg, case[0], K, N, 64, width)
    assert h.call_kernel(M) == "tsg_jit64_kernel" and h.jit_width(M) == width and h.jit_waves(M) == 8
    check_y(h, case, ydtype, ("rows64", width, M, K, N, xdtype))
    h.close()


@pytest.mark.parametrize("xdtype,ydtype", XY)
@pytest.mark.parametrize("knob", [None, "TSG_JIT_HALF", "TSG_JIT_PAIR"])
def test_ytype_rows64_four_wave_shape(tsg, monkeypatch, xdtype, ydtype, knob):
    """The 64-row image's automatic 4-wave shape, its half ring (TSG_JIT_HALF=1)
    and its wave pairs (TSG_JIT_PAIR=1: each wave stores its half of the rows)."""
    M, K, N = 65, 193, 700
    for k in ("TSG_JIT_HALF", "TSG_JIT_PAIR"):
        monkeypatch.delenv(k, raising=False)
    if knob:
        monkeypatch.setenv(knob, "1")
    case = _ycase(M, K, N, xdtype, ydtype)
    h = _jit_handle(tsg, case[0], K, N, 64, 0)
    assert h.call_kernel(M) == "tsg_jit64_kernel" and h.jit_waves(M) == 4, (h.jit_width(M), h.jit_waves(M))
    check_y(h, case, ydtype, ("rows64 4-wave", knob, M, K, N, xdtype))
    h.close()


@pytest.mark.parametrize("xdtype,ydtype", XY)
@pytest.mark.parametrize("width", [64, 0])
def test_ytype_rows128(tsg, xdtype, ydtype, width):
    """The 128-row image at width 64 (8 waves, two rows per lane) and, with
    width 0, its automatic 4-wave shape."""
    M, K, N = 130, 388, 700
    case = _ycase(M, K, N, xdtype, ydtype)
    h = _jit_handle(tsg, case[0], K, N, 128, width)
    assert h.call_kernel(M) == "tsg_jit_kernel" and h.call_tile_rows(M) == 128
    if width:
        assert h.jit_width(M) == width and h.jit_waves(M) == 8
    else:
        assert h.jit_waves(M) == 4, (h.jit_width(M), h.jit_waves(M))
    check_y(h, case, ydtype, ("rows128", width, M, K, N, xdtype))
    h.close()


@pytest.mark.parametrize("xdtype,ydtype", XY)
def test_ytype_rx_kernel(tsg, monkeypatch, xdtype, ydtype):
    M, K, N = 130, 193, 301
    monkeypatch.setenv("TSG_KERNEL", "rx")
    case = _ycase(M, K, N, xdtype, ydtype)
    h = tsg.TCSCDevice(*case[0], K, N)
    h.set_small_m(1)
    assert h.kernel_name() == "tsg_tcsc_rx_kernel" and h.call_kernel(M) == "tsg_tcsc_rx_kernel"
    check_y(h, case, ydtype, ("rx", M, K, N, xdtype))
    h.close()


@pytest.mark.parametrize("xdtype,ydtype", XY)
def test_ytype_blocked_handle(tsg, xdtype, ydtype):
    M, K, N, B = 130, 388, 700, 64
    case = _ycase(M, K, N, xdtype, ydtype, B)
    h = tsg.TCSCDevice.from_blocked(*case[0], K, N, B)
    h.set_small_m(1)
    assert h.call_kernel(M) == "tsg_jit_kernel"
    check_y(h, case, ydtype, ("blocked", M, K, N, B, xdtype))
    h.close()


# ---- xtype x ytype --------------------------------------------------------------------

@pytest.mark.parametrize("xdtype,ydtype", XY_ALL)
@pytest.mark.parametrize("family", ["walk", "rows64"])
def test_ytype_full_type_product(tsg, xdtype, ydtype, family):
    """xtype and ytype are independent: the whole product on one walk case and
    one 64-row case."""
    M, K, N = (16, 193, 301) if family == "walk" else (65, 388, 700)
    case = _ycase(M, K, N, xdtype, ydtype)
    if family == "walk":
        h = tsg.TCSCDevice(*case[0], K, N)
        assert h.call_kernel(M) == "tsg_tcsc_ell_kernel"
    else:
        h = _jit_handle(tsg, case[0], K, N, 64, 16)
        assert h.call_kernel(M) == "tsg_jit64_kernel" and h.jit_width(M) == 16
    check_y(h, case, ydtype, ("product", family, M, K, N, xdtype))
    h.close()


# ---- direct X -------------------------------------------------------------------------

def test_ytype_direct_x_stays_one_launch(tsg):
    """An aligned fp32 X at M = 64 is read by the 64-row image itself: still
    one launch, and the bf16 Y is right."""
    import torch
    M, K, N = 64, 388, 700
    arrays, Xt, Xw, b, alpha, ref, ref_p, want = _ycase(M, K, N, "float32", "bfloat16")
    h = tsg.TCSCDevice(*arrays, K, N)
    assert h.call_kernel(M) == "tsg_jit64_kernel"
    Xd, bd = Xt.cuda(), _dev(b)
    assert Xd.data_ptr() % 16 == 0
    Y = h.gemm_torch_xy(Xd, bd, out_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert h.call_launches(Xd, M) == 1
    assert np.array_equal(_ybits(Y), want["plain"])
    h.close()


# ---- rounding boundaries ------------------------------------------------------------------

def _magnitude(i, ydtype):
    """|value| (float64, exact) of the magnitude pattern i of the type, continued
    one step past the largest finite pattern (fp16: 65536, bf16: 2^128)."""
    i = np.asarray(i, dtype=np.int64)
    if ydtype == "float16":
        mb, bias = 10, 15
    else:
        mb, bias = 7, 127
    e, m = i >> mb, i & ((1 << mb) - 1)
    sub = np.ldexp(m.astype(np.float64), 1 - bias - mb)
    nor = np.ldexp(((1 << mb) + m).astype(np.float64), e - bias - mb)
    return np.where(e == 0, sub, nor)


@functools.lru_cache(maxsize=None)
def _boundary_values(ydtype, ties_only):
    """fp32 x values around every finite pattern p of the type: widen(p), the
    midpoint between p and its neighbour of larger magnitude (a tie), that
    midpoint's fp32 predecessor and successor; then +-inf, NaN, +-FLT_MAX, the
    smallest fp32 subnormal and +-0."""
    top = 0x7C00 if ydtype == "float16" else 0x7F80  # first non-finite magnitude pattern
    i = np.arange(top)
    lo, hi = _magnitude(i, ydtype), _magnitude(i + 1, ydtype)
    mid64 = (lo + hi) / 2
    mid = mid64.astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), mid64) and np.isfinite(mid).all()  # every tie is an fp32
    parts = [mid]
    if not ties_only:
        same = lo.astype(np.float32)
        assert np.array_equal(same.astype(np.float64), lo)
        parts += [same, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))]
    pos = np.concatenate(parts)
    fmax = np.finfo(np.float32).max
    extra = np.array([np.inf, -np.inf, np.nan, fmax, -fmax, 1e-45, -1e-45, 0.0, -0.0], np.float32)
    x = np.concatenate([pos, -pos, extra])
    x.setflags(write=False)
    return x


def _check_boundaries(h, ydtype, M, n, ties_only):
    """W = identity, b = 0: Y[m, k] = round((0 + X[m, k]) + 0)."""
    import torch
    vals = _boundary_values(ydtype, ties_only)
    assert vals.size <= M * n
    X = np.zeros(M * n, np.float32)
    X[:vals.size] = vals
    X = X.reshape(M, n)
    with np.errstate(invalid="ignore"):
        y32 = (np.float32(0) + X) + np.float32(0)
    want = _cast_bits(y32, ydtype)
    nan = np.isnan(y32)
    assert nan.sum() == 1
    # what the cast must show somewhere: ties both ways, overflow, subnormals
    wf = torch_from_bits(want, ydtype)
    assert np.isinf(wf[~np.isinf(y32)]).any(), "no finite value rounds to inf"
    if ydtype == "float16":
        at = lambda v: int(want.ravel()[np.flatnonzero(X.ravel() == v)[0]])
        assert at(np.float32(65520.0)) == 0x7C00, "65520 is the first value that rounds to inf"
        if not ties_only:
            assert at(np.nextafter(np.float32(65520.0), np.float32(0))) == 0x7BFF
        assert ((want.ravel()[:vals.size] & 0x7C00) == 0).sum() > 1024, "no fp16 subnormal results"
    Y = h.gemm_torch_xy(torch.from_numpy(X).cuda(), torch.zeros(n, device="cuda"), out_dtype=_tdtype(ydtype))
    Y32 = h.gemm_torch_x(torch.from_numpy(X).cuda(), torch.zeros(n, device="cuda"))
    torch.cuda.synchronize()
    g32 = Y32.cpu().numpy()
    assert np.array_equal(np.isnan(g32), nan) and np.array_equal(g32.view(np.uint32)[~nan], y32.view(np.uint32)[~nan]), \
        (ydtype, "the fp32 call differs")
    got = _ybits(Y)
    got_nan = np.isnan(torch_from_bits(got, ydtype))
    assert np.array_equal(got_nan, nan), (ydtype, "NaN-ness differs")
    bad = np.flatnonzero((got != want).ravel() & ~nan.ravel())
    assert bad.size == 0, (ydtype, bad.size, "elements differ; first (x bits, got, want)",
                           [(hex(int(X.ravel()[k:k + 1].view(np.uint32)[0])), hex(int(got.ravel()[k])),
                             hex(int(want.ravel()[k]))) for k in bad[:8]])


@pytest.mark.parametrize("ydtype", YDTYPES)
@pytest.mark.parametrize("family", ["rows64", "rows128", "rx"])
def test_ytype_rounding_boundaries_images(tsg, monkeypatch, ydtype, family):
    """Every finite pattern of the type, its tie and the tie's two fp32
    neighbours as a [512, 512] X against the 512 identity: ties to even,
    overflow to inf (fp16: from 65520), fp16 subnormals, bf16's carry into the
    exponent -- through the 16-byte stores of the images and rx."""
    n, M = 512, 512
    if family == "rx":
        monkeypatch.setenv("TSG_KERNEL", "rx")
        h = tsg.TCSCDevice(*_identity_tcsc(n), n, n)
        h.set_small_m(1)
        assert h.call_kernel(M) == "tsg_tcsc_rx_kernel"
    else:
        rows = 64 if family == "rows64" else 128
        h = _jit_handle(tsg, _identity_tcsc(n), n, n, rows, 0)
        assert h.call_kernel(M) == ("tsg_jit64_kernel" if rows == 64 else "tsg_jit_kernel")
        assert h.call_tile_rows(M) == rows
    _check_boundaries(h, ydtype, M, n, ties_only=False)
    h.close()


@pytest.mark.parametrize("ydtype", YDTYPES)
def test_ytype_rounding_boundaries_ell_walk(tsg, ydtype):
    """The ties alone as a [32, 2048] X against the 2048 identity on the ELL
    walk (2-byte stores)."""
    n, M = 2048, 32
    h = tsg.TCSCDevice(*_identity_tcsc(n), n, n)
    h.set_small_m(2)
    assert h.call_kernel(M) == "tsg_tcsc_ell_kernel"
    _check_boundaries(h, ydtype, M, n, ties_only=True)
    h.close()


# ---- the fp32 type through the new calls ---------------------------------------------------

def test_ytype_f32_is_the_x_call(tsg):
    """TSG_Y_F32 through gemm_dev_xy is tcsc_hip_gemm_dev_x: the same bits, ldY in floats."""
    import torch
    M, K, N = 65, 388, 700
    arrays, X, b, alpha, ref, ref_p = _case(M, K, N)
    h = tsg.TCSCDevice(*arrays, K, N)
    Xd, bd, ad = _dev(X), _dev(b), _dev(alpha)
    for al, want in ((None, ref), (ad, ref_p)):
        Yx = h.gemm_torch_x(Xd, bd, alpha=al)
        buf = torch.full((M + 2, N + 1), float("nan"), device="cuda")
        view = buf[1:M + 1, 0:N]
        h.gemm_dev_xy(Xd.data_ptr(), tsg.TSG_X_F32, bd.data_ptr(), view.data_ptr(), tsg.TSG_Y_F32, M,
                      dalpha=None if al is None else al.data_ptr(), ldY=N + 1)
        Yt = h.gemm_torch_xy(Xd, bd, alpha=al)  # out_dtype defaults to float32
        torch.cuda.synchronize()
        assert Yt.dtype == torch.float32
        assert np.array_equal(_bits(Yx), want.view(np.uint32))
        assert torch.equal(view.view(torch.int32), Yx.view(torch.int32))
        assert torch.equal(Yt.view(torch.int32), Yx.view(torch.int32))
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[M + 1]).all()) and \
            bool(torch.isnan(buf[:, N]).all())
    h.close()


# ---- errors and empty calls ------------------------------------------------------------------

def test_ytype_unknown_type_is_refused(tsg):
    import torch
    M, K, N = 16, 193, 301
    arrays, Xt, Xw, b, alpha, ref, ref_p, want = _ycase(M, K, N, "bfloat16", "bfloat16")
    h = tsg.TCSCDevice(*arrays, K, N)
    Xd, bd, ad = Xt.cuda(), _dev(b), _dev(alpha)
    buf = torch.empty((M + 2, 2 * N), dtype=torch.bfloat16, device="cuda")
    _fill16(buf)
    for ytype in (3, -1):
        for dalpha in (None, ad.data_ptr()):
            with pytest.raises(tsg.TSGError, match="is not a tsg_ytype") as e:
                h.gemm_dev_xy(Xd.data_ptr(), tsg.TSG_X_BF16, bd.data_ptr(), buf[1:].data_ptr(), ytype, M, 0, dalpha)
            assert e.value.code == 1  # TSG_ERR_ARG
    # rows that would overlap: ldY counts elements of the Y type
    with pytest.raises(tsg.TSGError, match="is less than N") as e:
        h.gemm_dev_xy(Xd.data_ptr(), tsg.TSG_X_BF16, bd.data_ptr(), buf[1:].data_ptr(), tsg.TSG_Y_BF16, M, ldY=N - 1)
    assert e.value.code == 1
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int16) == SENT16).all())
    h.close()


@pytest.mark.parametrize("ydtype", YDTYPES)
def test_ytype_empty_calls(tsg, ydtype):
    """M = 0 is TSG_OK and writes nothing; K = 0 gives round(b) -- with a PReLU
    of slope -1 also round(-b) for b <= 0, so +0 becomes -0 and stays -0 -- on
    a walk (M = 5) and an image (M = 70)."""
    import torch
    dt = _tdtype(ydtype)
    K, N = 193, 301
    arrays = _case(16, K, N)[0]
    h = tsg.TCSCDevice(*arrays, K, N)
    bd = _dev(np.zeros(N, np.float32))
    buf = torch.empty((4, N), dtype=dt, device="cuda")
    _fill16(buf)
    Y0 = h.gemm_torch_xy(torch.empty((0, K), device="cuda"), bd, buf[2:2])
    torch.cuda.synchronize()
    assert tuple(Y0.shape) == (0, N) and bool((buf.view(torch.int16) == SENT16).all())
    assert tuple(h.gemm_torch_xy(torch.empty((0, K), device="cuda"), bd, out_dtype=dt).shape) == (0, N)
    h.close()
    bn = np.array([1.5, -2.0, 0.0, 1.0009765625, 65520.0, -1e-7, 3.0e38, 0.1, -0.1], np.float32)
    an = np.full(bn.size, -1.0, np.float32)
    n = bn.size
    y = np.float32(0) + bn
    with np.errstate(over="ignore"):
        yp = np.where(y > 0, y, an * y).astype(np.float32)
    assert np.signbit(yp[2]) and yp[2] == 0  # -0
    h = tsg.TCSCDevice(np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32), [], [], 0, n)
    for M in (5, 70):
        X = torch.empty((M, 0), device="cuda")
        Y = h.gemm_torch_xy(X, _dev(bn), out_dtype=dt)
        Yp = h.gemm_torch_xy(X, _dev(bn), alpha=_dev(an), out_dtype=dt)
        torch.cuda.synchronize()
        assert np.array_equal(_ybits(Y), np.tile(_cast_bits(y, ydtype), (M, 1))), M
        assert np.array_equal(_ybits(Yp), np.tile(_cast_bits(yp, ydtype), (M, 1))), M
        assert int(_ybits(Yp)[0, 2]) == 0x8000
    h.close()


# ---- graph capture ------------------------------------------------------------------------

def test_ytype_graph_capture_after_reserve(tsg):
    """A captured bf16-in, bf16-out call into the odd view: nothing is
    allocated after reserve(130), two replays are right and write only the view."""
    import torch
    M, K, N = 64, 388, 700
    arrays, Xt, Xw, b, alpha, ref, ref_p, want = _ycase(M, K, N, "bfloat16", "bfloat16")
    h = tsg.TCSCDevice(*arrays, K, N)
    assert h.call_kernel(M) == "tsg_jit64_kernel"
    h.reserve(130)
    work = h.info()["work_bytes"]
    assert work > 0
    Xd, bd = Xt.cuda(), _dev(b)
    buf = torch.empty((M + 2, N + 3), dtype=torch.bfloat16, device="cuda")
    view = buf[1:M + 1, 1:N + 1]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture
        h.gemm_torch_xy(Xd, bd, view)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        h.gemm_torch_xy(Xd, bd, view)
    assert h.info()["work_bytes"] == work
    for replay in range(2):
        _fill16(buf)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_ybits(view), want["plain"]), replay
        _assert_only_view_written16(buf, 1, M + 1, 1, N + 1, ("graph replay", replay))
    assert h.info()["work_bytes"] == work
    h.close()


# ---- argument checks of the torch wrapper ----------------------------------------------------

def test_gemm_torch_xy_argument_checks(tsg):
    import torch
    M, K, N = 16, 193, 301
    arrays, Xt, Xw, b, alpha, ref, ref_p, want = _ycase(M, K, N, "bfloat16", "bfloat16")
    h = tsg.TCSCDevice(*arrays, K, N)
    Xd, bd = Xt.cuda(), _dev(b)
    bf = torch.bfloat16
    bad = {
        "float64 Y": dict(Y=torch.empty((M, N), dtype=torch.float64, device="cuda")),
        "Y device": dict(Y=torch.empty((M, N), dtype=bf)),
        "Y overlapping": dict(Y=torch.empty(M * N, dtype=bf, device="cuda").as_strided((M, N), (N - 1, 1))),
        "Y column-strided": dict(Y=torch.empty((M, 2 * N), dtype=bf, device="cuda")[:, ::2]),
        "Y shape": dict(Y=torch.empty((M, N + 1), dtype=bf, device="cuda")),
        "out_dtype != Y": dict(Y=torch.empty((M, N), dtype=bf, device="cuda"), out_dtype=torch.float16),
        "int8 out_dtype": dict(out_dtype=torch.int8),
        "float64 out_dtype": dict(out_dtype=torch.float64),
    }
    for name, kw in bad.items():
        with pytest.raises(tsg.TSGError):
            h.gemm_torch_xy(Xd, bd, **kw)
    # the fp32-only wrappers keep refusing a 16-bit Y
    Y16 = torch.empty((M, N), dtype=bf, device="cuda")
    with pytest.raises(tsg.TSGError):
        h.gemm_torch_x(Xd, bd, Y16)
    with pytest.raises(tsg.TSGError):
        h.gemm_torch_into(_dev(Xw), bd, Y16)
    # Y and out_dtype that agree are fine
    Y = h.gemm_torch_xy(Xd, bd, Y16, out_dtype=bf)
    torch.cuda.synchronize()
    assert Y is Y16 and np.array_equal(_ybits(Y), want["plain"])
    h.close()
