"""Per-row and per-column scales in the epilogue of the device-pointer calls
(tcsc_hip_gemm_dev_scaled, TCSCDevice.gemm_torch_scaled) through every kernel
family on the GPU.

The contract (include/ternary_spgemm.h): all fp32, one rounding per operation,
no fused multiply-add,

    t = chain;  t = t * rs[m];  t = t * cs[n];  y = t + b[n];  PReLU;  cast

with a NULL scale's multiply not performed.  The chain starts at +0 and is
never -0, so the oracle's base_tcsc(Xw, t, zeros) IS the chain bit for bit; the
expected Y is numpy fp32 arithmetic in that order (each line one rounding),
base_tcsc_prelu's rule, then test_gpu_ytype._cast_bits for a 16-bit Y.
Everything is compared as integers, no tolerance.

Inputs (asserted on the CPU in the case builder, _scase).  X is init_x_frac
with test_gpu_ytype's power-of-two shift for an fp16 Y (int8: integer draws),
b = linspace(-3, 3, N), cs = U[0.5, 2), rs = U[0.5, 2) * 2^-12.  Only for
int8 X, rs = U[0.5, 2) * 2^-4: its chains are integers below 2^12 in these
shapes (at most 127 * nnz(column)) where init_x_frac's reach 2^25, so 2^-12
would bring t below 1, under |b| <= 3; the last addition would then round away
the low bits in which the multiplies' roundings differ, and a wrong order or a
contraction could pass.  2^-4 keeps t near 2^7, well above b and, at most
2^12 * 2 * 2 * 2^-4 = 2^10, finite in fp16.  The builder then asserts that
the fp32 expectation with both scales differs, in at least 10 % of its elements
each, from (a) the fused fp32(float64(t) * float64(cs) + b), (b) chain * (rs *
cs) + b and (c) the column scale applied before the row scale -- and that it is
finite, also after the cast to the Y type.

Each family case asserts the kernel that ran, then runs the plain and the PReLU
call with both scales, the row scale only and the column scale only, into a
dense output and into the odd-stride sentinel view of test_gpu_ytype /
test_gpu_ldy (rows 1..M, columns 1..N+1 of an [M + 2, N + 3] buffer of NaN
patterns), where only the view may change."""
import functools
import os

import numpy as np
import pytest

from test_gpu_ldy import SENT, _assert_only_view_written, _bits, _dev, _fill, _jit_handle
from test_gpu_xtype import _tdtype
from test_gpu_ytype import (SENT16, YMAX, _assert_only_view_written16, _cast_bits, _fill16, _x_for, _ybits,
                            torch_from_bits)

pytestmark = pytest.mark.gpu

YDTYPES = ("float32", "float16", "bfloat16")
XDTYPES = ("float32", "float16", "bfloat16", "int8")
MODES = ("both", "row", "col")


@pytest.fixture(autouse=True)
def _oracle_built(oracle_mod):
    """The cached cases below import the oracle themselves: it is built first."""


def expect32(chain, rs, cs, b, alpha=None):
    """The contract in numpy fp32, one rounding per line; rs / cs None = no multiply."""
    t = chain
    if rs is not None:
        t = t * rs[:, None]
    if cs is not None:
        t = t * cs[None, :]
    y = t + b
    if alpha is not None:
        y = np.where(y > 0, y, alpha * y)  # comp_prelu.h:57-67
    assert y.dtype == np.float32
    return y


def _ybits_of(y32, ydtype):
    return y32.view(np.uint32) if ydtype == "float32" else _cast_bits(y32, ydtype)


def _draw_scales(M, N, e, seed):
    rng = np.random.default_rng(seed)
    rs = (rng.uniform(0.5, 2.0, M).astype(np.float32) * np.float32(2.0 ** -e)).astype(np.float32)
    cs = rng.uniform(0.5, 2.0, N).astype(np.float32)
    return rs, cs


@functools.lru_cache(maxsize=None)
def _chains(M, K, N, xdtype, ydtype, B=0):
    """W's arrays, X in its type, its widened copy and the oracle's chain
    (zero b), with test_gpu_ytype's shift for an fp16 Y."""
    import oracle as O
    W = O.gen_ternary(K, N, 4, 1000 * M + K + N)
    zeros = np.zeros(N, np.float32)
    if B:
        arrays = O.blocked_tcsc_encode(W, B)
        run = lambda Xw: O.base_blocked_tcsc(Xw, arrays, zeros, K, N, B)
    else:
        t = O.tcsc_encode(W)
        arrays = t.arrays
        run = lambda Xw: O.base_tcsc(Xw, t, zeros)
    shift = 0
    if ydtype == "float16" and xdtype != "int8":
        top = float(np.abs(run(_x_for(M, K, xdtype, M + 11, 0)[1]).astype(np.float64)).max())
        shift = max(0, int(np.ceil(np.log2(top / 2.0 ** 15)))) if top > 0 else 0
    Xt, Xw = _x_for(M, K, xdtype, M + 11, shift)
    chain = run(Xw)
    assert np.isfinite(chain).all() and not np.signbit(chain[chain == 0]).any()
    for a in (Xw, chain):
        a.setflags(write=False)
    return arrays, Xt, Xw, chain


@functools.lru_cache(maxsize=None)
def _scase(M, K, N, xdtype="float32", ydtype="float32", B=0):
    """One shape's inputs and expectations, computed once, never modified:
    (arrays, Xt, b, alpha, rs, cs, want) with want[(mode, 'plain' | 'prelu')] =
    the bits of the Y type.  The module docstring's input conditions are
    asserted here."""
    arrays, Xt, Xw, chain = _chains(M, K, N, xdtype, ydtype, B)
    b = np.linspace(-3, 3, N).astype(np.float32)
    alpha = np.linspace(-0.5, 0.5, N).astype(np.float32)
    e = 4 if xdtype == "int8" else 12  # (module docstring)
    rs, cs = _draw_scales(M, N, e, 7 * M + N)
    both = expect32(chain, rs, cs, b)
    t = (chain * rs[:, None]).astype(np.float32)
    alts = {
        "fused": (t.astype(np.float64) * cs[None, :].astype(np.float64) + b.astype(np.float64)).astype(np.float32),
        "scales multiplied first": chain * (rs[:, None] * cs[None, :]) + b,
        "column scale first": (chain * cs[None, :]) * rs[:, None] + b,
    }
    for name, alt in alts.items():
        frac = float(np.mean(alt.view(np.uint32) != both.view(np.uint32)))
        assert frac >= 0.10, (name, "is told apart from the contract in only", frac, (M, K, N, xdtype, ydtype, e))
    want = {}
    for mode, r, c in (("both", rs, cs), ("row", rs, None), ("col", None, cs)):
        for key, al in (("plain", None), ("prelu", alpha)):
            y = expect32(chain, r, c, b, al)
            assert np.isfinite(y).all(), (mode, key, "expected array is not finite")
            if ydtype != "float32":
                assert float(np.abs(y).max()) <= YMAX[ydtype], (mode, key, "expected array overflows the Y type")
            wb = _ybits_of(y, ydtype)
            wb.setflags(write=False)
            want[(mode, key)] = wb
    for a in (b, alpha, rs, cs):
        a.setflags(write=False)
    return arrays, Xt, b, alpha, rs, cs, want


def _got_bits(t, ydtype):
    return _bits(t) if ydtype == "float32" else _ybits(t)


def _outputs(M, N, ydtype, c0=None, pad=0):
    """name -> (buffer, view, box, fill, only_view): a dense output and the odd
    view.  With a column offset c0: one output instead, "view" = rows 1..M,
    columns c0..c0+N of an [M + 2, c0 + N + pad] buffer (test_gpu_call_fuzz)."""
    import torch
    dt = _tdtype(ydtype)
    f32 = ydtype == "float32"
    fill, only = (_fill, _assert_only_view_written) if f32 else (_fill16, _assert_only_view_written16)
    if c0 is not None:
        buf = torch.empty((M + 2, c0 + N + pad), dtype=dt, device="cuda")
        return {"view": (buf, buf[1:M + 1, c0:c0 + N], (1, M + 1, c0, c0 + N), fill, only)}
    dense = torch.empty((M + 2, N), dtype=dt, device="cuda")
    odd = torch.empty((M + 2, N + 3), dtype=dt, device="cuda")
    return {"dense": (dense, dense[1:M + 1], (1, M + 1, 0, N), fill, only),
            "odd": (odd, odd[1:M + 1, 1:N + 1], (1, M + 1, 1, N + 1), fill, only)}


def check_scaled(h, case, ydtype, what, prelu=True, modes=MODES):
    """The shared scheme (module docstring) for one handle and one case."""
    import torch
    arrays, Xt, b, alpha, rs, cs, want = case
    M, N = Xt.shape[0], b.shape[0]
    Xd, bd, ad, rd, cd = Xt.cuda(), _dev(b), _dev(alpha), _dev(rs), _dev(cs)
    keep = [t.clone() for t in (Xd, bd, ad, rd, cd)]
    outs = _outputs(M, N, ydtype)
    for mode in modes:
        r = rd if mode in ("both", "row") else None
        c = cd if mode in ("both", "col") else None
        for key, al in (("plain", None), ("prelu", ad)):
            if key == "prelu" and not prelu:
                continue
            wb = want[(mode, key)]
            for name, (buf, view, box, fill, only) in outs.items():
                tag = (what, ydtype, mode, key, name)
                fill(buf)
                out = h.gemm_torch_scaled(Xd, bd, view, alpha=al, row_scale=r, col_scale=c)
                torch.cuda.synchronize()
                assert out is view
                got = _got_bits(view, ydtype)
                assert np.array_equal(got, wb), (tag, int((got != wb).sum()), "of", wb.size, "elements differ")
                only(buf, *box, tag)
    for t, k, n in zip((Xd, bd, ad, rd, cd), keep, ("X", "b", "alpha", "row_scale", "col_scale")):
        assert torch.equal(t.view(torch.int8), k.view(torch.int8)), (what, n, "was written")


# ---- every kernel family ----------------------------------------------------

@pytest.mark.parametrize("ydtype", YDTYPES)
@pytest.mark.parametrize("M,K,N,mode,kernel", [(1, 193, 301, 0, "tsg_tcsc_ell_pc_kernel"),
                                               (4, 193, 301, 0, "tsg_tcsc_ell_kernel"),
                                               (16, 193, 301, 0, "tsg_tcsc_ell_kernel")])
def test_scaled_small_m_walks(tsg, ydtype, M, K, N, mode, kernel):
    """The producer/consumer walk and the ELL walk."""
    case = _scase(M, K, N, "float32", ydtype)
    h = tsg.TCSCDevice(*case[0], K, N)
    h.set_small_m(3 if (M == 4) else mode)  # (M = 4: the producer/consumer walk switched off, as test_gpu_ldy)
    assert h.call_kernel(M) == kernel and h.call_tile_rows(M) == 0
    check_scaled(h, case, ydtype, (kernel, M, K, N))
    h.close()


@pytest.mark.parametrize("ydtype", YDTYPES)
@pytest.mark.parametrize("width,M,K,N", [(128, 63, 193, 700), (16, 65, 388, 700), (8, 130, 193, 301)])
def test_scaled_rows64_widths(tsg, ydtype, width, M, K, N):
    """The 64-row image at widths 128, 16 and 8 (8 waves)."""
    case = _scase(M, K, N, "float32", ydtype)
    h = _jit_handle(tsg, case[0], K, N, 64, width)
    assert h.call_kernel(M) == "tsg_jit64_kernel" and h.jit_width(M) == width and h.jit_waves(M) == 8
    check_scaled(h, case, ydtype, ("rows64", width, M, K, N))
    h.close()


@pytest.mark.parametrize("ydtype", YDTYPES)
@pytest.mark.parametrize("knob", [None, "TSG_JIT_HALF", "TSG_JIT_PAIR"])
def test_scaled_rows64_four_wave_shape(tsg, monkeypatch, ydtype, knob):
    """The 64-row image's automatic 4-wave shape, its half ring and its wave pairs."""
    M, K, N = 65, 193, 700
    for k in ("TSG_JIT_HALF", "TSG_JIT_PAIR"):
        monkeypatch.delenv(k, raising=False)
    if knob:
        monkeypatch.setenv(knob, "1")
    case = _scase(M, K, N, "float32", ydtype)
    h = _jit_handle(tsg, case[0], K, N, 64, 0)
    assert h.call_kernel(M) == "tsg_jit64_kernel" and h.jit_waves(M) == 4, (h.jit_width(M), h.jit_waves(M))
    check_scaled(h, case, ydtype, ("rows64 4-wave", knob, M, K, N))
    h.close()


@pytest.mark.parametrize("ydtype", YDTYPES)
@pytest.mark.parametrize("width", [64, 0])
def test_scaled_rows128(tsg, ydtype, width):
    """The 128-row image at width 64 (8 waves, two rows per lane: two row
    scales per lane) and, with width 0, its automatic 4-wave shape."""
    M, K, N = 130, 388, 700
    case = _scase(M, K, N, "float32", ydtype)
    h = _jit_handle(tsg, case[0], K, N, 128, width)
    assert h.call_kernel(M) == "tsg_jit_kernel" and h.call_tile_rows(M) == 128
    if width:
        assert h.jit_width(M) == width and h.jit_waves(M) == 8
    else:
        assert h.jit_waves(M) == 4, (h.jit_width(M), h.jit_waves(M))
    check_scaled(h, case, ydtype, ("rows128", width, M, K, N))
    h.close()


@pytest.mark.parametrize("ydtype", YDTYPES)
def test_scaled_rx_kernel(tsg, monkeypatch, ydtype):
    M, K, N = 130, 193, 301
    monkeypatch.setenv("TSG_KERNEL", "rx")
    case = _scase(M, K, N, "float32", ydtype)
    h = tsg.TCSCDevice(*case[0], K, N)
    h.set_small_m(1)
    assert h.kernel_name() == "tsg_tcsc_rx_kernel" and h.call_kernel(M) == "tsg_tcsc_rx_kernel"
    check_scaled(h, case, ydtype, ("rx", M, K, N))
    h.close()


@pytest.mark.parametrize("ydtype", YDTYPES)
def test_scaled_blocked_handle(tsg, ydtype):
    """A blocked handle: the scales apply to the chain after the last block
    (the plain call only: the oracle has no blocked PReLU)."""
    M, K, N, B = 130, 385, 700, 64
    case = _scase(M, K, N, "float32", ydtype, B)
    h = tsg.TCSCDevice.from_blocked(*case[0], K, N, B)
    h.set_small_m(1)
    assert h.call_kernel(M) == "tsg_jit_kernel"
    check_scaled(h, case, ydtype, ("blocked", M, K, N, B), prelu=False)
    h.close()


# ---- xtype x ytype --------------------------------------------------------------------

@pytest.mark.parametrize("ydtype", YDTYPES)
@pytest.mark.parametrize("xdtype", XDTYPES)
@pytest.mark.parametrize("family", ["walk", "rows64"])
def test_scaled_full_type_product(tsg, xdtype, ydtype, family):
    """xtype, ytype and the scales are independent: the whole product on one
    walk case and one 64-row case."""
    M, K, N = (16, 193, 301) if family == "walk" else (65, 388, 700)
    case = _scase(M, K, N, xdtype, ydtype)
    if family == "walk":
        h = tsg.TCSCDevice(*case[0], K, N)
        assert h.call_kernel(M) == "tsg_tcsc_ell_kernel"
    else:
        h = _jit_handle(tsg, case[0], K, N, 64, 16)
        assert h.call_kernel(M) == "tsg_jit64_kernel" and h.jit_width(M) == 16
    check_scaled(h, case, ydtype, ("product", family, M, K, N, xdtype))
    h.close()


# ---- the motivating case ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _motivating_case():
    """K = 1040, N = 8: column 0 holds +1 in all 1040 rows, the others a few
    entries each; int8 X whose row 2 is all 127.  Unscaled, Y[2, 0] = 132080
    overflows fp16; with rs[2] = 1/127 it is 1040 + b."""
    import torch
    import oracle as O
    K, N, M = 1040, 8, 5
    W = np.zeros((K, N), np.int32)
    W[:, 0] = 1
    rng = np.random.default_rng(5)
    for n in range(1, N):
        rows = rng.choice(K, size=2 + n, replace=False)
        W[rows, n] = rng.choice([-1, 1], size=rows.size)
    t = O.tcsc_encode(W)
    X = rng.integers(-127, 128, size=(M, K)).astype(np.int8)
    X[2, :] = 127
    Xw = X.astype(np.float32)
    b = np.linspace(-3, 3, N).astype(np.float32)
    chain = O.base_tcsc(Xw, t, np.zeros(N, np.float32))
    assert chain[2, 0] == 127.0 * 1040
    unscaled16 = torch_from_bits(_cast_bits(chain + b, "float16"), "float16")
    assert np.isinf(unscaled16).any() and np.isinf(unscaled16[2, 0]), "the unscaled fp16 Y does not overflow"
    rs = rng.uniform(0.5, 2.0, M).astype(np.float32) * np.float32(2.0 ** -6)
    rs[2] = np.float32(1.0) / np.float32(127.0)
    cs = rng.uniform(0.5, 2.0, N).astype(np.float32)
    cs[0] = np.float32(1.0)
    y = expect32(chain, rs, cs, b)
    want = _cast_bits(y, "float16")
    assert np.isfinite(torch_from_bits(want, "float16")).all()
    return t.arrays, torch.from_numpy(X), b, rs, cs, want, K, N, M


def test_scaled_motivating_int8_in_fp16_out(tsg):
    """int8 in, fp16 out in one call: finite and the oracle's, where the
    unscaled call overflows (asserted on the CPU and seen on the GPU)."""
    import torch
    arrays, Xt, b, rs, cs, want, K, N, M = _motivating_case()
    h = tsg.TCSCDevice(*arrays, K, N)
    Xd, bd, rd, cd = Xt.cuda(), _dev(b), _dev(rs), _dev(cs)
    Yu = h.gemm_torch_xy(Xd, bd, out_dtype=torch.float16)
    Y = h.gemm_torch_scaled(Xd, bd, out_dtype=torch.float16, row_scale=rd, col_scale=cd)
    torch.cuda.synchronize()
    assert bool(torch.isinf(Yu[2, 0]))
    assert bool(torch.isfinite(Y).all())
    assert np.array_equal(_ybits(Y), want)
    h.close()


# ---- NULL scales -----------------------------------------------------------------------

@pytest.mark.parametrize("ydtype", YDTYPES)
@pytest.mark.parametrize("family", ["walk", "rows64", "rows128"])
def test_scaled_null_and_unit_scales(tsg, ydtype, family):
    """Both scales None is gemm_torch_xy bit for bit; a scale of all 1.0f
    (either one, or both) gives the same bits on finite data."""
    import torch
    M, K, N = {"walk": (16, 193, 301), "rows64": (65, 388, 700), "rows128": (130, 388, 700)}[family]
    arrays, Xt, b, alpha, rs, cs, want = _scase(M, K, N, "float32", ydtype)
    if family == "walk":
        h = tsg.TCSCDevice(*arrays, K, N)
    else:
        h = _jit_handle(tsg, arrays, K, N, 64 if family == "rows64" else 128, 0)
    dt = _tdtype(ydtype)
    Xd, bd, ad = Xt.cuda(), _dev(b), _dev(alpha)
    ones_m, ones_n = torch.ones(M, device="cuda"), torch.ones(N, device="cuda")
    for al in (None, ad):
        ref = h.gemm_torch_xy(Xd, bd, alpha=al, out_dtype=dt)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(ref.float()).all())
        for r, c in ((None, None), (ones_m, None), (None, ones_n), (ones_m, ones_n)):
            Y = h.gemm_torch_scaled(Xd, bd, alpha=al, out_dtype=dt, row_scale=r, col_scale=c)
            torch.cuda.synchronize()
            assert Y.dtype == dt
            assert np.array_equal(_got_bits(Y, ydtype), _got_bits(ref, ydtype)), (family, ydtype, r is None, c is None)
    h.close()


# ---- special scales ----------------------------------------------------------------------

@pytest.mark.parametrize("family", ["walk", "rows64"])
def test_scaled_special_scale_values(tsg, family):
    """0, -1, a subnormal, inf and NaN at fixed positions of both scale
    vectors: the IEEE result of the contract's operations, non-NaN results by
    bits, NaN positions by isnan."""
    import torch
    M, K, N = (16, 193, 301) if family == "walk" else (65, 388, 700)
    arrays, Xt, Xw, chain = _chains(M, K, N, "float32", "float32")
    b = np.linspace(-3, 3, N).astype(np.float32)
    alpha = np.linspace(-0.5, 0.5, N).astype(np.float32)
    rs, cs = (a.copy() for a in _draw_scales(M, N, 12, 3))
    special = np.array([0.0, -1.0, 1e-40, np.inf, np.nan, -0.0, -np.inf], np.float32)
    assert special[2] != 0 and abs(special[2]) < np.finfo(np.float32).tiny  # a subnormal
    rs[1:1 + special.size] = special
    cs[3:3 + special.size] = special
    cs[N - 1] = np.float32(np.nan)  # the last column, where the bias index is clamped in ragged tiles
    if family == "walk":
        h = tsg.TCSCDevice(*arrays, K, N)
        assert h.call_kernel(M) == "tsg_tcsc_ell_kernel"
    else:
        h = _jit_handle(tsg, arrays, K, N, 64, 16)
        assert h.call_kernel(M) == "tsg_jit64_kernel"
    Xd, bd, ad, rd, cd = Xt.cuda(), _dev(b), _dev(alpha), _dev(rs), _dev(cs)
    for al_np, al in ((None, None), (alpha, ad)):
        with np.errstate(all="ignore"):
            y = expect32(chain, rs, cs, b, al_np)
        nan = np.isnan(y)
        assert nan.any() and np.isinf(y).any()
        if al_np is None:  # row 1: the scale 0 leaves +-0 + b wherever the column scale is finite
            fin = np.isfinite(cs)
            assert fin.sum() == N - 4 and np.array_equal(y[1][fin], b[fin])
        Y = h.gemm_torch_scaled(Xd, bd, alpha=al, row_scale=rd, col_scale=cd)
        torch.cuda.synchronize()
        g = Y.cpu().numpy()
        assert np.array_equal(np.isnan(g), nan), (family, "NaN positions differ")
        bad = (g.view(np.uint32) != y.view(np.uint32)) & ~nan
        assert not bad.any(), (family, int(bad.sum()), "elements differ", np.argwhere(bad)[:8].tolist())
    h.close()


# ---- isolation -------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["walk", "rows64"])
def test_scaled_isolation(tsg, family):
    """The scales as interior slices, at an odd float offset, of NaN-filled
    buffers, after an all-NaN-scale call on the same handle: Y is the oracle's
    and the scale buffers are unchanged.  The 64-row image still reads an
    aligned fp32 X itself: call_launches (a query of the plan, which takes no
    scale) says one launch, and -- what sees the scaled calls themselves -- the
    fresh handle still has no work buffer after them, where a staged call
    allocates one (shown with a bf16 X at the end)."""
    import torch
    M, K, N = (16, 193, 301) if family == "walk" else (64, 388, 700)
    arrays, Xt, b, alpha, rs, cs, want = _scase(M, K, N, "float32", "float32")
    h = tsg.TCSCDevice(*arrays, K, N)
    assert h.call_kernel(M) == ("tsg_tcsc_ell_kernel" if family == "walk" else "tsg_jit64_kernel")
    Xd, bd = Xt.cuda(), _dev(b)
    launches = h.call_launches(Xd, M)
    if family == "rows64":
        assert Xd.data_ptr() % 16 == 0 and launches == 1
    nan_m, nan_n = torch.full((M,), float("nan"), device="cuda"), torch.full((N,), float("nan"), device="cuda")
    Y0 = h.gemm_torch_scaled(Xd, bd, row_scale=nan_m, col_scale=nan_n)
    torch.cuda.synchronize()
    assert bool(torch.isnan(Y0).all())
    rbuf = torch.full((M + 11,), float("nan"), device="cuda")
    cbuf = torch.full((N + 11,), float("nan"), device="cuda")
    rbuf.view(torch.int32).fill_(SENT)
    cbuf.view(torch.int32).fill_(SENT)
    rd, cd = rbuf[3:3 + M], cbuf[5:5 + N]
    assert (rd.data_ptr() // 4) % 2 == 1 and (cd.data_ptr() // 4) % 2 == 1 and rd.is_contiguous()
    rd.copy_(_dev(rs))
    cd.copy_(_dev(cs))
    keep_r, keep_c = rbuf.clone(), cbuf.clone()
    Y = h.gemm_torch_scaled(Xd, bd, row_scale=rd, col_scale=cd)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Y), want[("both", "plain")])
    assert torch.equal(rbuf.view(torch.int32), keep_r.view(torch.int32)), "the row-scale buffer was written"
    assert torch.equal(cbuf.view(torch.int32), keep_c.view(torch.int32)), "the column-scale buffer was written"
    assert h.call_launches(Xd, M) == launches
    if family == "rows64":
        assert h.info()["work_bytes"] == 0, "a scaled call on an aligned fp32 X was staged"
        h.gemm_torch_scaled(Xd.to(torch.bfloat16), bd, row_scale=rd, col_scale=cd)
        torch.cuda.synchronize()
        assert h.info()["work_bytes"] > 0  # (a staged call does allocate it)
    h.close()


# ---- graph capture ----------------------------------------------------------------------------

def test_scaled_graph_capture_after_reserve(tsg):
    """A captured scaled bf16-in, bf16-out call into the odd view: nothing is
    allocated after reserve(130); a replay is right, and so is one after X and
    both scale tensors were rewritten in place."""
    import torch
    M, K, N = 64, 388, 700
    arrays, Xt, b, alpha, rs, cs, want = _scase(M, K, N, "bfloat16", "bfloat16")
    import oracle as O
    Xt2, Xw2 = _x_for(M, K, "bfloat16", 4321, 0)  # the second replay's X and scales
    chain2 = O.base_tcsc(Xw2, O.TCSC(*arrays, K, N), np.zeros(N, np.float32))
    rs2, cs2 = _draw_scales(M, N, 12, 99)
    want2 = _cast_bits(expect32(chain2, rs2, cs2, b), "bfloat16")
    assert not np.array_equal(want2, want[("both", "plain")])
    h = tsg.TCSCDevice(*arrays, K, N)
    assert h.call_kernel(M) == "tsg_jit64_kernel"
    h.reserve(130)
    work = h.info()["work_bytes"]
    assert work > 0
    Xd, bd, rd, cd = Xt.cuda(), _dev(b), _dev(rs), _dev(cs)
    buf = torch.empty((M + 2, N + 3), dtype=torch.bfloat16, device="cuda")
    view = buf[1:M + 1, 1:N + 1]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture
        h.gemm_torch_scaled(Xd, bd, view, row_scale=rd, col_scale=cd)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        h.gemm_torch_scaled(Xd, bd, view, row_scale=rd, col_scale=cd)
    assert h.info()["work_bytes"] == work
    for replay, wb in enumerate((want[("both", "plain")], want2)):
        if replay:
            Xd.copy_(Xt2.cuda())
            rd.copy_(_dev(rs2))
            cd.copy_(_dev(cs2))
        _fill16(buf)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_ybits(view), wb), replay
        _assert_only_view_written16(buf, 1, M + 1, 1, N + 1, ("graph replay", replay))
    assert h.info()["work_bytes"] == work
    h.close()


# ---- refusals ------------------------------------------------------------------------------------

def test_scaled_bad_arguments_are_refused(tsg):
    """A bad ytype, a bad xtype and ldY < N: TSG_ERR_ARG, nothing written."""
    import torch
    M, K, N = 16, 193, 301
    arrays, Xt, b, alpha, rs, cs, want = _scase(M, K, N, "bfloat16", "bfloat16")
    h = tsg.TCSCDevice(*arrays, K, N)
    Xd, bd, ad, rd, cd = Xt.cuda(), _dev(b), _dev(alpha), _dev(rs), _dev(cs)
    buf = torch.empty((M + 2, 2 * N), dtype=torch.bfloat16, device="cuda")
    _fill16(buf)
    args = dict(drow_scale=rd.data_ptr(), dcol_scale=cd.data_ptr())
    for dalpha in (None, ad.data_ptr()):
        for ytype in (3, -1):
            with pytest.raises(tsg.TSGError, match="is not a tsg_ytype") as e:
                h.gemm_dev_scaled(Xd.data_ptr(), tsg.TSG_X_BF16, bd.data_ptr(), buf[1:].data_ptr(), ytype, M, 0,
                                  dalpha, **args)
            assert e.value.code == 1  # TSG_ERR_ARG
        for xtype in (4, -1):
            with pytest.raises(tsg.TSGError, match="is not a tsg_xtype") as e:
                h.gemm_dev_scaled(Xd.data_ptr(), xtype, bd.data_ptr(), buf[1:].data_ptr(), tsg.TSG_Y_BF16, M, 0,
                                  dalpha, **args)
            assert e.value.code == 1
        with pytest.raises(tsg.TSGError, match="is less than N") as e:
            h.gemm_dev_scaled(Xd.data_ptr(), tsg.TSG_X_BF16, bd.data_ptr(), buf[1:].data_ptr(), tsg.TSG_Y_BF16, M, 0,
                              dalpha, ldY=N - 1, **args)
        assert e.value.code == 1
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int16) == SENT16).all())
    h.close()


def test_gemm_torch_scaled_argument_checks(tsg):
    import torch
    M, K, N = 16, 193, 301
    arrays, Xt, b, alpha, rs, cs, want = _scase(M, K, N, "bfloat16", "bfloat16")
    h = tsg.TCSCDevice(*arrays, K, N)
    Xd, bd, rd, cd = Xt.cuda(), _dev(b), _dev(rs), _dev(cs)
    bad = {
        "row_scale": [rd.double(), rd.half(), torch.ones(M + 1, device="cuda"), torch.ones(M), rd.reshape(M, 1),
                      torch.ones(2 * M, device="cuda")[::2], [1.0] * M],
        "col_scale": [cd.double(), cd.to(torch.bfloat16), torch.ones(N - 1, device="cuda"), torch.ones(N),
                      torch.ones(2 * N, device="cuda")[::2], torch.ones(M, device="cuda")],
    }
    for name, values in bad.items():
        for v in values:
            with pytest.raises(tsg.TSGError, match=name) as e:
                h.gemm_torch_scaled(Xd, bd, out_dtype=torch.bfloat16, **{name: v})
            assert e.value.code == 1
    # the Y checks of gemm_torch_xy apply
    with pytest.raises(tsg.TSGError):
        h.gemm_torch_scaled(Xd, bd, torch.empty((M, N + 1), dtype=torch.bfloat16, device="cuda"), row_scale=rd)
    with pytest.raises(tsg.TSGError):
        h.gemm_torch_scaled(Xd, bd, out_dtype=torch.int8, col_scale=cd)
    Y = h.gemm_torch_scaled(Xd, bd, out_dtype=torch.bfloat16, row_scale=rd, col_scale=cd)
    torch.cuda.synchronize()
    assert np.array_equal(_ybits(Y), want[("both", "plain")])
    h.close()


# ---- the dispatcher marker ----------------------------------------------------------------------

def test_template_without_scale_marker_is_refused(tsg, monkeypatch, tmp_path, capfd):
    """A dispatcher template that lacks the tsg_jit_args_scale marker (built
    before the argument list grew by the two scale pointers; here: the
    marker's name patched out of a copy) is refused by the loader like a
    missing one -- the registration falls back to rx with a warning, a pinned
    jit fails -- and is never launched."""
    libdir = os.path.dirname(tsg.LIB_PATH)
    for f in os.listdir(libdir):
        if f.endswith(".co"):
            data = open(os.path.join(libdir, f), "rb").read()
            assert b"tsg_jit_args_scale" in data, f
            (tmp_path / f).write_bytes(data.replace(b"tsg_jit_args_scale", b"tsg_jit_args_unscl"))
    monkeypatch.setenv("TSG_JIT_DIR", str(tmp_path))
    M, K, N = 130, 193, 301
    case = _scase(M, K, N, "float32", "float32")
    h = tsg.TCSCDevice(*case[0], K, N)
    assert h.kernel_name() == "tsg_tcsc_rx_kernel"
    assert "falling back to the rx kernel" in capfd.readouterr().err
    h.set_small_m(1)
    check_scaled(h, case, "float32", ("rx fallback", M, K, N), modes=("both",))
    h.close()
    monkeypatch.setenv("TSG_KERNEL", "jit")
    with pytest.raises(tsg.TSGError, match="predates the dispatcher's scale arguments"):
        tsg.TCSCDevice(*case[0], K, N)


# ---- ShardedTCSC -----------------------------------------------------------------------------------

def test_scaled_sharded_forward_into(tsg):
    """ShardedTCSC.forward_into with scales for world 3, the ranks looped on one
    GPU (col_scale_full sliced [n0:n1] like b_full), equals the unsplit handle
    and the oracle; forward (a new local block) likewise."""
    import torch
    import tsg_dist
    M, K, N, world = 65, 388, 700, 3
    arrays, Xt, b, alpha, rs, cs, want = _scase(M, K, N, "float32", "float32")
    Xd, bd, rd, cd = Xt.cuda(), _dev(b), _dev(rs), _dev(cs)
    h = tsg.TCSCDevice(*arrays, K, N)
    whole = h.gemm_torch_scaled(Xd, bd, row_scale=rd, col_scale=cd)
    h.close()
    Y = torch.empty((M, N), device="cuda")
    _fill(Y)
    for rank in range(world):
        sh = tsg_dist.ShardedTCSC.from_tcsc(*arrays, K, N, rank, world)
        out = sh.forward_into(Xd, bd, Y, row_scale=rd, col_scale_full=cd)
        assert out.data_ptr() == Y[:, sh.n0:sh.n1].data_ptr() and tuple(out.shape) == (M, sh.n1 - sh.n0)
        loc = sh.forward(Xd, bd, row_scale=rd, col_scale_full=cd)
        torch.cuda.synchronize()
        assert bool((Y.view(torch.int32)[:, sh.n1:] == SENT).all()), rank
        assert torch.equal(loc.view(torch.int32), Y[:, sh.n0:sh.n1].contiguous().view(torch.int32)), rank
        sh.local.close()
    assert np.array_equal(_bits(Y), want[("both", "plain")])
    assert torch.equal(Y.view(torch.int32), whole.view(torch.int32))
