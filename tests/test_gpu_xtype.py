"""fp16, bf16 and int8 X on the device-pointer calls (tcsc_hip_gemm_dev_x,
TCSCDevice.gemm_torch_x) through every kernel family on the GPU.

The contract: Y equals, bit for bit, what the fp32 call gives on the
element-wise widened X.  So every case compares the narrow call's bits with
the CPU oracle on the widened fp32 X and with the same handle's
gemm_torch(X_widened); no tolerance anywhere.

X is made on the CPU: for the 16-bit types oracle.init_x_frac (order-sensitive:
every partial sum rounds) rounded to the type with torch's CPU cast, for int8
integer draws in [-127, 127].  init_x_frac reaches 2^23, past fp16's largest
finite value (65504), so for fp16 it is first scaled by 2^-8 (exact in fp32;
the small end then lands in fp16's subnormals and zeros); the widened X is
asserted finite for every type.

The scheme follows test_gpu_ldy: each case asserts the kernel family that ran
(call_kernel, jit_width, jit_waves, call_tile_rows), runs one plain call, one
PReLU call and one strided call (ldY = N + 1) inside a sentinel-filled buffer
of which only the view may change."""
import functools

import numpy as np
import pytest

from test_gpu_ldy import SENT, _assert_only_view_written, _bits, _case, _dev, _fill, _jit_handle

pytestmark = pytest.mark.gpu

DTYPES = ("float16", "bfloat16", "int8")


@pytest.fixture(autouse=True)
def _oracle_built(oracle_mod):
    """The cached cases below import the oracle themselves: it is built first."""


def _tdtype(name):
    import torch
    return getattr(torch, name)


def _narrow_x(M, K, dtype, seed):
    """(X in the type as a CPU torch tensor, X widened to fp32 as numpy)."""
    import torch
    import oracle as O
    if dtype == "int8":
        Xt = torch.from_numpy(np.random.default_rng(seed).integers(-127, 128, size=(M, K)).astype(np.int8))
    else:
        X = O.init_x_frac(M, K, seed)
        if dtype == "float16":
            X = X * np.float32(2.0 ** -8)  # exact; |X| <= 2^15 fits fp16
        Xt = torch.from_numpy(X).to(_tdtype(dtype))  # torch's CPU cast (round to nearest even)
    Xw = Xt.to(torch.float32).numpy()
    assert Xw.shape == (M, K) and np.isfinite(Xw).all(), (dtype, "widened X is not finite")
    return Xt, Xw


@functools.lru_cache(maxsize=None)
def _xcase(M, K, N, dtype, B=0):
    """W (test_gpu_ldy._case's for the shape), X in the type, b, alpha and the
    oracle's results on the widened X: computed once, never modified."""
    import oracle as O
    W = O.gen_ternary(K, N, 4, 1000 * M + K + N)
    Xt, Xw = _narrow_x(M, K, dtype, M + 11)
    b = np.linspace(-3, 3, N).astype(np.float32)
    alpha = np.linspace(-0.5, 0.5, N).astype(np.float32)
    if B:
        arrays = O.blocked_tcsc_encode(W, B)
        ref, ref_p = O.base_blocked_tcsc(Xw, arrays, b, K, N, B), None  # (the oracle has no blocked PReLU)
    else:
        t = O.tcsc_encode(W)
        ref, ref_p = O.base_tcsc(Xw, t, b), O.base_tcsc_prelu(Xw, t, b, alpha)
        arrays = t.arrays
    for a in (Xw, b, alpha, ref) + ((ref_p,) if ref_p is not None else ()):
        a.setflags(write=False)
    return arrays, Xt, Xw, b, alpha, ref, ref_p


def _x_on_device(Xt, offset):
    """X on the GPU: its own allocation (aligned), or a slice that starts
    `offset` elements into a larger buffer of the type."""
    import torch
    if not offset:
        Xd = Xt.cuda()
        assert Xd.data_ptr() % 16 == 0
        return Xd
    M, K = Xt.shape
    buf = torch.zeros(M * K + 8, dtype=Xt.dtype, device="cuda")
    Xd = buf[offset:offset + M * K].view(M, K)
    Xd.copy_(Xt)
    assert Xd.is_contiguous() and Xd.data_ptr() == buf.data_ptr() + offset * Xt.element_size()
    return Xd


def check_x(h, case, what, offsets=(0,)):
    """The shared scheme (module docstring) for one handle and one case."""
    import torch
    arrays, Xt, Xw, b, alpha, ref, ref_p = case
    M, N = Xt.shape[0], b.shape[0]
    bd, ad = _dev(b), _dev(alpha)
    Xwd = _dev(Xw)
    dense = h.gemm_torch(Xwd, bd)
    dense_p = h.gemm_torch(Xwd, bd, alpha=ad)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dense), ref.view(np.uint32)), (what, "fp32 call on the widened X != oracle")
    for off in offsets:
        Xd = _x_on_device(Xt, off)
        keep = Xd.clone()
        tag = (what, str(Xt.dtype), "offset", off)
        Y = h.gemm_torch_x(Xd, bd)
        Yp = h.gemm_torch_x(Xd, bd, alpha=ad)
        torch.cuda.synchronize()
        assert Y.dtype == torch.float32 and tuple(Y.shape) == (M, N)
        assert np.array_equal(_bits(Y), ref.view(np.uint32)), (tag, "plain != oracle")
        assert torch.equal(Y.view(torch.int32), dense.view(torch.int32)), (tag, "plain != gemm_torch(widened)")
        if ref_p is not None:
            assert np.array_equal(_bits(Yp), ref_p.view(np.uint32)), (tag, "prelu != oracle")
        assert torch.equal(Yp.view(torch.int32), dense_p.view(torch.int32)), (tag, "prelu != gemm_torch(widened)")
        buf = torch.empty((M + 2, N + 1), device="cuda")
        view = buf[1:M + 1, 0:N]
        _fill(buf)
        out = h.gemm_torch_x(Xd, bd, view)
        torch.cuda.synchronize()
        assert out is view and (M == 1 or view.stride(0) == N + 1)
        assert np.array_equal(_bits(view), ref.view(np.uint32)), (tag, "strided view != oracle")
        _assert_only_view_written(buf, 1, M + 1, 0, N, tag)
        assert torch.equal(Xd.view(torch.int8), keep.view(torch.int8)), (tag, "X was written")


def _offsets(K):
    """K = 388 (vector loads) also runs X one element into a larger buffer,
    which forces the scalar form."""
    return (0, 1) if K % 4 == 0 else (0,)


# ---- every kernel family ----------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K,N,mode,kernel", [(1, 193, 301, 0, "tsg_tcsc_ell_pc_kernel"),
                                               (4, 388, 700, 0, "tsg_tcsc_ell_pc_kernel"),
                                               (4, 388, 700, 3, "tsg_tcsc_ell_kernel"),
                                               (16, 193, 301, 0, "tsg_tcsc_ell_kernel"),
                                               (16, 388, 700, 0, "tsg_tcsc_ell_kernel")])
def test_xtype_small_m_walks(tsg, dtype, M, K, N, mode, kernel):
    """The producer/consumer walk (M = 1, and M = 4 as planned) and the ELL walk
    (M = 16 as planned; M = 4 with the producer/consumer walk switched off):
    both read X in place through ell_stage."""
    case = _xcase(M, K, N, dtype)
    h = tsg.TCSCDevice(*case[0], K, N)
    h.set_small_m(mode)
    assert h.call_kernel(M) == kernel and h.call_tile_rows(M) == 0
    check_x(h, case, (kernel, M, K, N), _offsets(K))
    h.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width,M,K,N", [(128, 63, 193, 700), (128, 130, 388, 301), (16, 65, 388, 700),
                                         (8, 130, 193, 301), (8, 63, 388, 700)])
def test_xtype_rows64_widths(tsg, dtype, width, M, K, N):
    """The 64-row image at widths 128, 16 and 8 (8 waves): always through the
    staged copy (tsg_transpose_rows_kernel; at K = 388 three chunks, the last
    one starting at K - 188), never direct X."""
    case = _xcase(M, K, N, dtype)
    h = _jit_handle(tsg, case[0], K, N, 64, width)
    assert h.call_kernel(M) == "tsg_jit64_kernel" and h.jit_width(M) == width and h.jit_waves(M) == 8
    check_x(h, case, ("rows64", width, M, K, N), _offsets(K))
    h.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("knob", [None, "TSG_JIT_HALF"])
@pytest.mark.parametrize("M,K,N", [(65, 193, 700), (130, 388, 301)])
def test_xtype_rows64_four_wave_shape(tsg, monkeypatch, dtype, knob, M, K, N):
    """The 64-row image's automatic 4-wave shape, and its half ring
    (TSG_JIT_HALF=1), whose staged copy is the blocked layout
    (tsg_transpose_quads_kernel)."""
    for k in ("TSG_JIT_HALF", "TSG_JIT_PAIR"):
        monkeypatch.delenv(k, raising=False)
    if knob:
        monkeypatch.setenv(knob, "1")
    case = _xcase(M, K, N, dtype)
    h = _jit_handle(tsg, case[0], K, N, 64, 0)
    assert h.call_kernel(M) == "tsg_jit64_kernel" and h.jit_waves(M) == 4, (h.jit_width(M), h.jit_waves(M))
    check_x(h, case, ("rows64 4-wave", knob, M, K, N), _offsets(K))
    h.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width,M,K,N", [(64, 130, 388, 700), (64, 65, 193, 301), (0, 130, 193, 700),
                                         (0, 130, 388, 700)])
def test_xtype_rows128(tsg, dtype, width, M, K, N):
    """The 128-row image at width 64 (8 waves) and, with width 0, its automatic
    4-wave shape (tsg_transpose_pairs_kernel)."""
    case = _xcase(M, K, N, dtype)
    h = _jit_handle(tsg, case[0], K, N, 128, width)
    assert h.call_kernel(M) == "tsg_jit_kernel" and h.call_tile_rows(M) == 128
    if width:
        assert h.jit_width(M) == width and h.jit_waves(M) == 8
    else:
        assert h.jit_waves(M) == 4, (h.jit_width(M), h.jit_waves(M))
    check_x(h, case, ("rows128", width, M, K, N), _offsets(K))
    h.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K,N", [(130, 193, 301), (63, 388, 700)])
def test_xtype_rx_kernel(tsg, monkeypatch, dtype, M, K, N):
    """The rx kernel (tsg_transpose_kernel / tsg_transpose4_kernel)."""
    monkeypatch.setenv("TSG_KERNEL", "rx")
    case = _xcase(M, K, N, dtype)
    h = tsg.TCSCDevice(*case[0], K, N)
    h.set_small_m(1)
    assert h.kernel_name() == "tsg_tcsc_rx_kernel" and h.call_kernel(M) == "tsg_tcsc_rx_kernel"
    check_x(h, case, ("rx", M, K, N), _offsets(K))
    h.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_xtype_blocked_handle(tsg, dtype):
    M, K, N, B = 130, 388, 700, 64
    case = _xcase(M, K, N, dtype, B)
    h = tsg.TCSCDevice.from_blocked(*case[0], K, N, B)
    h.set_small_m(1)
    assert h.call_kernel(M) == "tsg_jit_kernel"
    check_x(h, case, ("blocked", M, K, N, B), _offsets(K))
    h.close()


# ---- tiny K -----------------------------------------------------------------------

@pytest.mark.parametrize("K", [3, 4])
@pytest.mark.parametrize("M", [5, 70])
def test_xtype_tiny_k(tsg, M, K):
    """K below one quad (3) and exactly one quad (4), as planned: a walk at
    M = 5, the 64-row image at M = 70."""
    N = 301
    case = _xcase(M, K, N, "bfloat16")
    h = tsg.TCSCDevice(*case[0], K, N)
    assert h.call_kernel(M) == ("tsg_tcsc_ell_kernel" if M == 5 else "tsg_jit64_kernel")
    check_x(h, case, ("tiny K", M, K, N), _offsets(K))
    h.close()


# ---- every bit pattern ----------------------------------------------------------------

def _identity_tcsc(n):
    return (np.arange(n + 1, dtype=np.int32), np.zeros(n + 1, np.int32), np.arange(n, dtype=np.int32),
            np.zeros(0, np.int32))


def _all_patterns(dtype, shape):
    """Every bit pattern of the type (65,536, or int8's 256 as [4, 64] blocks)
    as a CPU tensor of `shape`, and the patterns widened to fp32 with numpy."""
    import torch
    if dtype == "int8":
        block = np.arange(256, dtype=np.uint8).view(np.int8).reshape(4, 64)
        Xn = np.tile(block, (shape[0] // 4, shape[1] // 64))
        return torch.from_numpy(Xn), Xn.astype(np.float32)
    bits = np.arange(65536, dtype=np.uint16).reshape(shape)
    if dtype == "float16":
        wide = bits.view(np.float16).astype(np.float32)
    else:
        wide = (bits.astype(np.uint32) << 16).view(np.float32)
    return torch.from_numpy(bits.view(np.int16)).view(_tdtype(dtype)), wide


def _check_patterns(h, dtype, M, n):
    """W = identity, b = 0: Y[m, k] is the chain 0 + widen(X[m, k]), then + 0."""
    import torch
    Xt, wide = _all_patterns(dtype, (M, n))
    assert tuple(Xt.shape) == (M, n) and Xt.dtype == _tdtype(dtype)
    with np.errstate(invalid="ignore"):
        want = (np.float32(0) + wide) + np.float32(0)
    Y = h.gemm_torch_x(Xt.cuda(), torch.zeros(n, device="cuda"))
    torch.cuda.synchronize()
    got = Y.cpu().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (dtype, "NaN-ness differs")
    if dtype != "int8":
        assert nan.sum() == (2046 if dtype == "float16" else 254)  # the type's NaN patterns
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), (dtype, "bits differ")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["rows64", "rows128", "rx"])
def test_xtype_every_bit_pattern_images(tsg, monkeypatch, dtype, family):
    """All patterns of the type as a [128, 512] X against the 512 identity:
    subnormals, -0, +-inf and every NaN through the staged copies."""
    n, M = 512, 128
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
    _check_patterns(h, dtype, M, n)
    h.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_xtype_every_bit_pattern_ell_walk(tsg, dtype):
    """The same as a [32, 2048] X against the 2048 identity on the ELL walk."""
    n, M = 2048, 32
    h = tsg.TCSCDevice(*_identity_tcsc(n), n, n)
    h.set_small_m(2)
    assert h.call_kernel(M) == "tsg_tcsc_ell_kernel"
    _check_patterns(h, dtype, M, n)
    h.close()


# ---- isolation ------------------------------------------------------------------------

@pytest.mark.parametrize("family,M,K,N", [("walk", 16, 193, 301), ("rows64", 65, 388, 301), ("rows128", 130, 388, 700)])
def test_xtype_isolation_bf16(tsg, family, M, K, N):
    """bf16 X as a slice with NaN elements directly before and after it (at an
    aligned and at an odd element offset), after a call on the same handle
    whose X is all NaN and has more rows: Y is still the oracle's."""
    import torch
    case = _xcase(M, K, N, "bfloat16")
    arrays, Xt, Xw, b, alpha, ref, ref_p = case
    if family == "walk":
        h = tsg.TCSCDevice(*arrays, K, N)
        assert h.call_kernel(M) == "tsg_tcsc_ell_kernel"
    else:
        rows = 64 if family == "rows64" else 128
        h = _jit_handle(tsg, arrays, K, N, rows, 0)
        assert h.call_tile_rows(M) == rows and h.call_tile_rows(M + 64) == rows
    assert not np.isnan(ref).any() and not np.isnan(ref_p).any()
    bd, ad = _dev(b), _dev(alpha)
    nan_bits = 0x7FC5  # a quiet bf16 NaN
    poison = torch.full((M + 64, K), nan_bits, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    assert bool(torch.isnan(poison).all())
    guard = 128 * K + 1024
    for off in (0, 1):
        buf = torch.full((2 * guard + M * K + 8,), nan_bits, dtype=torch.int16, device="cuda").view(torch.bfloat16)
        lo = guard + off
        Xd = buf[lo:lo + M * K].view(M, K)
        Xd.copy_(Xt)
        assert Xd.data_ptr() % 8 == 2 * off
        Yn = h.gemm_torch_x(poison, bd)  # leaves NaN in every real slot of the work buffer
        Y = h.gemm_torch_x(Xd, bd)
        Yp = h.gemm_torch_x(Xd, bd, alpha=ad)
        torch.cuda.synchronize()
        assert bool(torch.isnan(Yn).any())
        tag = (family, M, K, N, "offset", off)
        assert np.array_equal(_bits(Y), ref.view(np.uint32)), (tag, int(torch.isnan(Y).sum()), "NaN outputs")
        assert np.array_equal(_bits(Yp), ref_p.view(np.uint32)), (tag, int(torch.isnan(Yp).sum()), "NaN outputs")
        bits = buf.view(torch.int16)
        assert bool((bits[:lo] == nan_bits).all()) and bool((bits[lo + M * K:] == nan_bits).all()), (tag, "guard written")
    h.close()


# ---- work-buffer hand-over ------------------------------------------------------------------

def test_xtype_work_buffer_hand_over(tsg):
    """fp32 (direct X: no work buffer), bf16 (staged), fp32 again on one handle
    over two streams, no host sync in between: all three results are right."""
    import torch
    M, K, N = 64, 388, 700
    arrays, X, b, alpha, ref, ref_p = _case(M, K, N)
    arrays_x, Xt, Xw, bx, alphax, ref_x, ref_xp = _xcase(M, K, N, "bfloat16")
    assert all(np.array_equal(a, c) for a, c in zip(arrays, arrays_x)) and np.array_equal(b, bx)
    h = tsg.TCSCDevice(*arrays, K, N)
    assert h.call_kernel(M) == "tsg_jit64_kernel"
    Xd, Xnd, bd = _dev(X), Xt.cuda(), _dev(b)
    assert Xd.data_ptr() % 16 == 0 and Xnd.data_ptr() % 16 == 0
    h.gemm_torch(Xd, bd)  # the image is compiled before the checked calls
    torch.cuda.synchronize()
    assert h.call_launches(Xd, M) == 1  # the fp32 call reads X itself
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        Y1 = h.gemm_torch(Xd, bd)
    with torch.cuda.stream(s2):
        Y2 = h.gemm_torch_x(Xnd, bd)
    with torch.cuda.stream(s1):
        Y3 = h.gemm_torch(Xd, bd)
    with torch.cuda.stream(s2):
        Y4 = h.gemm_torch_x(Xnd, bd)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Y1), ref.view(np.uint32))
    assert np.array_equal(_bits(Y2), ref_x.view(np.uint32))
    assert np.array_equal(_bits(Y3), ref.view(np.uint32))
    assert np.array_equal(_bits(Y4), ref_x.view(np.uint32))
    assert h.info()["work_bytes"] > 0  # the bf16 calls were staged
    h.close()


# ---- graph capture ------------------------------------------------------------------------

def test_xtype_graph_capture_after_reserve(tsg):
    """reserve(130) sizes the work buffer for the staged copy of a shape whose
    fp32 call needs none; the captured bf16 call allocates nothing."""
    import torch
    M, K, N = 64, 388, 700
    arrays, Xt, Xw, b, alpha, ref, ref_p = _xcase(M, K, N, "bfloat16")
    h = tsg.TCSCDevice(*arrays, K, N)
    assert h.call_kernel(M) == "tsg_jit64_kernel"
    h.reserve(130)
    work = h.info()["work_bytes"]
    assert work > 0
    Xd, bd = Xt.cuda(), _dev(b)
    buf = torch.empty((M + 2, N + 1), device="cuda")
    view = buf[1:M + 1, 0:N]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture
        h.gemm_torch_x(Xd, bd, view)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        h.gemm_torch_x(Xd, bd, view)
    assert h.info()["work_bytes"] == work
    for replay in range(2):
        _fill(buf)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(view), ref.view(np.uint32)), replay
        _assert_only_view_written(buf, 1, M + 1, 0, N, ("graph replay", replay))
    h.close()


def test_xtype_capture_without_reserve_fails_loudly(tsg):
    """A fresh handle has no work buffer: a captured bf16 call at a shape whose
    fp32 call needs none is refused with the reserve hint, not a crash."""
    import torch
    M, K, N = 64, 388, 700
    arrays, Xt, Xw, b, alpha, ref, ref_p = _xcase(M, K, N, "bfloat16")
    h = tsg.TCSCDevice(*arrays, K, N)
    Xd, bd = Xt.cuda(), _dev(b)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(tsg.TSGError, match="call tcsc_hip_reserve"):
        with torch.cuda.graph(g):
            h.gemm_torch_x(Xd, bd)
    torch.cuda.synchronize()
    Y = h.gemm_torch_x(Xd, bd)  # the handle still works
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Y), ref.view(np.uint32))
    h.close()


# ---- errors -------------------------------------------------------------------------------

def test_xtype_unknown_type_is_refused(tsg):
    import torch
    M, K, N = 16, 193, 301
    arrays, Xt, Xw, b, alpha, ref, ref_p = _xcase(M, K, N, "bfloat16")
    h = tsg.TCSCDevice(*arrays, K, N)
    Xd, bd, ad = Xt.cuda(), _dev(b), _dev(alpha)
    buf = torch.empty((M + 2, N), device="cuda")
    _fill(buf)
    for xtype in (4, -1):
        for dalpha in (None, ad.data_ptr()):
            with pytest.raises(tsg.TSGError, match="is not a tsg_xtype") as e:
                h.gemm_dev_x(Xd.data_ptr(), xtype, bd.data_ptr(), buf[1:].data_ptr(), M, 0, dalpha)
            assert e.value.code == 1  # TSG_ERR_ARG
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int32) == SENT).all())
    h.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_xtype_empty_calls(tsg, dtype):
    """M = 0 is TSG_OK and writes nothing; K = 0 gives Y = b (a walk at M = 5,
    an image at M = 70)."""
    import torch
    K, N = 193, 301
    arrays, Xt, Xw, b, alpha, ref, ref_p = _xcase(16, K, N, dtype)
    h = tsg.TCSCDevice(*arrays, K, N)
    bd = _dev(b)
    Y0 = h.gemm_torch_x(torch.empty((0, K), dtype=_tdtype(dtype), device="cuda"), bd)
    assert tuple(Y0.shape) == (0, N)
    h.close()
    bn = np.array([1.5, -2.0, 0.0], np.float32)
    h = tsg.TCSCDevice(np.zeros(4, np.int32), np.zeros(4, np.int32), [], [], 0, 3)
    for M in (5, 70):
        Y = h.gemm_torch_x(torch.empty((M, 0), dtype=_tdtype(dtype), device="cuda"), _dev(bn))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(Y), np.tile(bn, (M, 1)).view(np.uint32)), M
    h.close()


def test_gemm_torch_x_argument_checks(tsg):
    import torch
    M, K, N = 16, 193, 301
    arrays, Xt, Xw, b, alpha, ref, ref_p = _xcase(M, K, N, "bfloat16")
    h = tsg.TCSCDevice(*arrays, K, N)
    Xd, bd = Xt.cuda(), _dev(b)
    wide = torch.zeros((M, 2 * K), dtype=torch.bfloat16, device="cuda")
    bad = {
        "float64": dict(X=Xd.double(), b=bd),
        "int32": dict(X=Xd.to(torch.int32), b=bd),
        "non-contiguous": dict(X=wide[:, 0:2 * K:2], b=bd),
        "row-strided": dict(X=wide[:, :K], b=bd),
        "device": dict(X=Xt, b=bd),
        "narrow": dict(X=Xd[:, :K - 1].contiguous(), b=bd),
        "b dtype": dict(X=Xd, b=bd.to(torch.bfloat16)),
        "Y dtype": dict(X=Xd, b=bd, Y=torch.empty((M, N), dtype=torch.bfloat16, device="cuda")),
        "Y overlapping": dict(X=Xd, b=bd, Y=torch.empty(M * N, device="cuda").as_strided((M, N), (N - 1, 1))),
    }
    for name, kw in bad.items():
        with pytest.raises(tsg.TSGError):
            h.gemm_torch_x(**kw)
    # gemm_torch and gemm_torch_into keep refusing a non-fp32 X
    with pytest.raises(tsg.TSGError):
        h.gemm_torch(Xd, bd)
    with pytest.raises(tsg.TSGError):
        h.gemm_torch_into(Xd, bd, torch.empty((M, N), device="cuda"))
    # a float32 X is the fp32 call
    Y = h.gemm_torch_x(_dev(Xw), bd)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Y), ref.view(np.uint32))
    h.close()
