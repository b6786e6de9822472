"""Output row stride (ldY) of the device-pointer calls (tcsc_hip_gemm_dev_ld,
TCSCDevice.gemm_torch_into, ShardedTCSC.forward_into) through every kernel
family on the GPU.

One scheme for every case: the output is the view buf[1:M+1, n0:n0+N] of a
[M+2, LD] buffer pre-filled (through an int32 view) with a NaN bit pattern no
result can hold; after the call the view equals the CPU oracle bit for bit,
equals the same handle's dense gemm_torch result bit for bit, and every other
float of the buffer -- the guard rows and the columns left and right of the
view -- still holds the sentinel.  X is init_x_frac (order-sensitive); each
case also runs one PReLU call."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# a quiet NaN with a payload: arithmetic only ever produces the canonical NaNs
SENT = 0x7FC5A5A5


def stride_cases(N):
    """name -> (LD, n0), each named for the store path it forces."""
    la = 4 * ((N + 3) // 4) + 8
    return {
        "dense": (N, 0),                # the ldY = N case through the new entry point
        "odd": (N + 1, 0),              # odd stride: 3 rows of 4 misaligned, scalar stores
        "aligned": (la, 4),             # every row 16-B aligned: float4 stores
        "misbase": (la, 1),             # aligned stride, misaligned base: scalar stores on every row
        "middle": (3 * N + 5, N + 2),   # the view sits in the middle of a wide buffer
    }


@functools.lru_cache(maxsize=None)
def _case(M, K, N, B=0):
    """W, X, b, alpha and the oracle's results for a shape: computed once,
    shared by every test that uses the shape, never modified."""
    import oracle as O
    W = O.gen_ternary(K, N, 4, 1000 * M + K + N)
    X = O.init_x_frac(M, K, M + 11)
    b = np.linspace(-3, 3, N).astype(np.float32)
    alpha = np.linspace(-0.5, 0.5, N).astype(np.float32)
    if B:
        blk = O.blocked_tcsc_encode(W, B)
        ref, ref_p = O.base_blocked_tcsc(X, blk, b, K, N, B), None  # (the oracle has no blocked PReLU)
        arrays = blk
    else:
        t = O.tcsc_encode(W)
        ref, ref_p = O.base_tcsc(X, t, b), O.base_tcsc_prelu(X, t, b, alpha)
        arrays = t.arrays
    for a in (X, b, alpha, ref) + ((ref_p,) if ref_p is not None else ()):
        a.setflags(write=False)
    return arrays, X, b, alpha, ref, ref_p


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _fill(buf):
    buf.view(__import__("torch").int32).fill_(SENT)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _assert_only_view_written(buf, r0, r1, c0, c1, what):
    """Every float of buf outside buf[r0:r1, c0:c1] still holds the sentinel."""
    import torch
    bits = buf.view(torch.int32).clone()
    bits[r0:r1, c0:c1] = SENT
    wrong = (bits != SENT).nonzero()
    assert wrong.numel() == 0, (what, "wrote outside the view at (row, col)", wrong[:8].tolist())


def check_strided(h, M, N, X, b, alpha, ref, ref_p, what, cases=None):
    """The shared scheme (module docstring) over the stride cases."""
    import torch
    Xd, bd, ad = _dev(X), _dev(b), _dev(alpha)
    dense = h.gemm_torch(Xd, bd)
    dense_p = h.gemm_torch(Xd, bd, alpha=ad)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dense), ref.view(np.uint32)), (what, "dense call != oracle")
    for name, (LD, n0) in stride_cases(N).items():
        if cases is not None and name not in cases:
            continue
        buf = torch.empty((M + 2, LD), device="cuda")
        view = buf[1:M + 1, n0:n0 + N]
        for al, want, want_dense in ((None, ref, dense), (ad, ref_p, dense_p)):
            _fill(buf)
            out = h.gemm_torch_into(Xd, bd, view, alpha=al)
            torch.cuda.synchronize()
            tag = (what, name, LD, n0, "prelu" if al is not None else "plain")
            assert out is view
            if want is not None:
                assert np.array_equal(_bits(view), want.view(np.uint32)), (tag, "view != oracle")
            assert torch.equal(view.view(torch.int32), want_dense.view(torch.int32)), (tag, "view != dense gemm_torch")
            _assert_only_view_written(buf, 1, M + 1, n0, n0 + N, tag)


# ---- every kernel family ----------------------------------------------------

@pytest.mark.parametrize("M,K,N,mode,kernel", [(1, 193, 301, 0, "tsg_tcsc_ell_pc_kernel"),
                                               (1, 385, 700, 0, "tsg_tcsc_ell_pc_kernel"),
                                               (4, 385, 700, 0, "tsg_tcsc_ell_pc_kernel"),
                                               (4, 385, 700, 3, "tsg_tcsc_ell_kernel"),
                                               (16, 193, 301, 0, "tsg_tcsc_ell_kernel"),
                                               (16, 385, 700, 0, "tsg_tcsc_ell_kernel")])
def test_ldy_small_m_walks(tsg, M, K, N, mode, kernel):
    """The producer/consumer walk (M = 1, and M = 4 as planned) and the ELL walk
    (M = 16 as planned; M = 4 with the producer/consumer walk switched off)."""
    arrays, X, b, alpha, ref, ref_p = _case(M, K, N)
    h = tsg.TCSCDevice(*arrays, K, N)
    h.set_small_m(mode)
    assert h.call_kernel(M) == kernel
    check_strided(h, M, N, X, b, alpha, ref, ref_p, (kernel, M, K, N))
    h.close()


def _jit_handle(tsg, arrays, K, N, rows, width):
    h = tsg.TCSCDevice(*arrays, K, N)
    h.set_small_m(1)
    h.set_tile_rows(rows)
    if width:
        h.set_jit_width(width)
    return h


@pytest.mark.parametrize("width,M,K,N", [(128, 63, 193, 700), (64, 65, 385, 301), (32, 130, 193, 301),
                                         (16, 63, 385, 700), (8, 65, 193, 700), (32, 63, 385, 700),
                                         (128, 130, 385, 301)])
def test_ldy_rows64_widths(tsg, width, M, K, N):
    """The 64-row image, every stream width (8 waves)."""
    arrays, X, b, alpha, ref, ref_p = _case(M, K, N)
    h = _jit_handle(tsg, arrays, K, N, 64, width)
    assert h.call_kernel(M) == "tsg_jit64_kernel" and h.jit_width(M) == width and h.jit_waves(M) == 8
    check_strided(h, M, N, X, b, alpha, ref, ref_p, ("rows64", width, M, K, N))
    h.close()


@pytest.mark.parametrize("knob", [None, "TSG_JIT_HALF", "TSG_JIT_PAIR"])
@pytest.mark.parametrize("M,K,N", [(65, 193, 700), (130, 385, 301)])
def test_ldy_rows64_four_wave_shapes(tsg, monkeypatch, knob, M, K, N):
    """The 64-row image's 4-wave shape (the automatic pick at these sizes), its
    half ring (TSG_JIT_HALF=1) and its wave pairs (TSG_JIT_PAIR=1)."""
    for k in ("TSG_JIT_HALF", "TSG_JIT_PAIR"):
        monkeypatch.delenv(k, raising=False)
    if knob:
        monkeypatch.setenv(knob, "1")
    arrays, X, b, alpha, ref, ref_p = _case(M, K, N)
    h = _jit_handle(tsg, arrays, K, N, 64, 0)
    assert h.call_kernel(M) == "tsg_jit64_kernel" and h.jit_waves(M) == 4, (h.jit_width(M), h.jit_waves(M))
    check_strided(h, M, N, X, b, alpha, ref, ref_p, ("rows64 4-wave", knob, M, K, N))
    h.close()


@pytest.mark.parametrize("width,M,K,N", [(64, 127, 193, 700), (32, 130, 385, 301), (16, 127, 385, 700),
                                         (8, 130, 193, 301), (0, 130, 193, 700)])
def test_ldy_rows128(tsg, width, M, K, N):
    """The 128-row image: every stream width (8 waves) and, with width 0, the
    automatic 4-wave shape."""
    arrays, X, b, alpha, ref, ref_p = _case(M, K, N)
    h = _jit_handle(tsg, arrays, K, N, 128, width)
    assert h.call_kernel(M) == "tsg_jit_kernel" and h.call_tile_rows(M) == 128
    if width:
        assert h.jit_width(M) == width and h.jit_waves(M) == 8
    else:
        assert h.jit_waves(M) == 4, (h.jit_width(M), h.jit_waves(M))
    check_strided(h, M, N, X, b, alpha, ref, ref_p, ("rows128", width, M, K, N))
    h.close()


@pytest.mark.parametrize("M,K,N", [(130, 193, 301), (5, 385, 700)])
def test_ldy_rx_kernel(tsg, monkeypatch, M, K, N):
    monkeypatch.setenv("TSG_KERNEL", "rx")
    arrays, X, b, alpha, ref, ref_p = _case(M, K, N)
    h = tsg.TCSCDevice(*arrays, K, N)
    h.set_small_m(1)
    assert h.kernel_name() == "tsg_tcsc_rx_kernel" and h.call_kernel(M) == "tsg_tcsc_rx_kernel"
    check_strided(h, M, N, X, b, alpha, ref, ref_p, ("rx", M, K, N))
    h.close()


def test_ldy_blocked_handle(tsg):
    M, K, N, B = 130, 385, 700, 64
    arrays, X, b, alpha, ref, ref_p = _case(M, K, N, B)
    h = tsg.TCSCDevice.from_blocked(*arrays, K, N, B)
    h.set_small_m(1)
    assert h.call_kernel(M) == "tsg_jit_kernel"
    check_strided(h, M, N, X, b, alpha, ref, ref_p, ("blocked", M, K, N, B))
    h.close()


# ---- two handles, one buffer --------------------------------------------------

def test_ldy_two_handles_one_buffer(tsg):
    """W split at the ragged column 301: both halves write their blocks into one
    [M, 700] tensor on two streams; the result is the unsplit handle's Y."""
    import torch
    M, K, N, cut = 70, 257, 700, 301
    arrays, X, b, alpha, ref, ref_p = _case(M, K, N)
    full = tsg.TCSCDevice(*arrays, K, N)
    Xd, bd = _dev(X), _dev(b)
    want = full.gemm_torch(Xd, bd)
    parts = [(0, cut), (cut, N)]
    hs = [tsg.TCSCDevice(*tsg.tcsc_slice(*arrays, N, a, c), K, c - a) for a, c in parts]
    bs = [bd[a:c].contiguous() for a, c in parts]
    Y = torch.empty((M, N), device="cuda")
    _fill(Y)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for h, bb, (a, c), s in zip(hs, bs, parts, streams):
        with torch.cuda.stream(s):
            h.gemm_torch_into(Xd, bb, Y[:, a:c])
    torch.cuda.synchronize()
    assert torch.equal(Y.view(torch.int32), want.view(torch.int32))
    assert np.array_equal(_bits(Y), ref.view(np.uint32))
    for h in hs + [full]:
        h.close()


def test_ldy_sharded_forward_into(tsg):
    """The same W through ShardedTCSC.forward_into for world 3, the ranks
    looped on one GPU: no scratch block, no reorder."""
    import torch
    import tsg_dist
    M, K, N, world = 70, 257, 700, 3
    arrays, X, b, alpha, ref, ref_p = _case(M, K, N)
    Xd, bd = _dev(X), _dev(b)
    Y = torch.empty((M, N), device="cuda")
    _fill(Y)
    for rank in range(world):
        sh = tsg_dist.ShardedTCSC.from_tcsc(*arrays, K, N, rank, world)
        out = sh.forward_into(Xd, bd, Y)
        assert out.data_ptr() == Y[:, sh.n0:sh.n1].data_ptr() and tuple(out.shape) == (M, sh.n1 - sh.n0)
        torch.cuda.synchronize()
        # the columns of later ranks are untouched so far
        assert bool((Y.view(torch.int32)[:, sh.n1:] == SENT).all()), rank
        sh.local.close()
    assert np.array_equal(_bits(Y), ref.view(np.uint32))
    with pytest.raises(tsg.TSGError):
        tsg_dist.ShardedTCSC.from_tcsc(*arrays, K, N, 0, world).forward_into(Xd, bd, Y[:, :N - 1])


# ---- graph capture ----------------------------------------------------------------

def test_ldy_graph_capture_after_reserve(tsg):
    import torch
    M, K, N = 70, 257, 700
    arrays, X, b, alpha, ref, ref_p = _case(M, K, N)
    h = tsg.TCSCDevice(*arrays, K, N)
    assert h.call_kernel(M) == "tsg_jit64_kernel"
    h.reserve(M)
    LD, n0 = stride_cases(N)["odd"][0] + 6, 3
    Xd, bd = _dev(X), _dev(b)
    buf = torch.empty((M + 2, LD), device="cuda")
    view = buf[1:M + 1, n0:n0 + N]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture
        h.gemm_torch_into(Xd, bd, view)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        h.gemm_torch_into(Xd, bd, view)
    for replay in range(2):
        _fill(buf)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(view), ref.view(np.uint32)), replay
        _assert_only_view_written(buf, 1, M + 1, n0, n0 + N, ("graph replay", replay))
    h.close()


# ---- 64-bit row offsets -------------------------------------------------------------

@pytest.mark.parametrize("rows", [0, 64, 128])
def test_ldy_row_offsets_past_2_32(tsg, rows):
    """ldY = 2^29 + 3 with M = 9: the last row starts 2^32 + 24 floats into the
    buffer (about 19.3 GiB, allocated and never filled): the automatic kernel
    and both weight-compiled images forced.  The sentinel guards the 8 floats
    on either side of each row's block."""
    import torch
    M, K, N, ldY, n0, G = 9, 64, 40, 2 ** 29 + 3, 8, 8
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, the case needs 24 GiB")
    arrays, X, b, alpha, ref, ref_p = _case(M, K, N)
    h = tsg.TCSCDevice(*arrays, K, N)
    if rows:
        h.set_small_m(1)
        h.set_tile_rows(rows)
        assert h.call_tile_rows(M) == rows
    else:
        assert h.call_tile_rows(M) == 0  # a small-M walk
    assert (M - 1) * ldY >= 2 ** 32
    buf = torch.empty((M, ldY), device="cuda")
    view = buf[:, n0:n0 + N]
    guard = buf[:, n0 - G:n0 + N + G]
    Xd, bd, ad = _dev(X), _dev(b), _dev(alpha)
    for al, want in ((None, ref), (ad, ref_p)):
        guard.view(torch.int32).fill_(SENT)
        h.gemm_torch_into(Xd, bd, view, alpha=al)
        torch.cuda.synchronize()
        got = _bits(guard)
        assert np.array_equal(got[:, G:G + N], want.view(np.uint32)), (rows, h.call_kernel(M))
        assert (got[:, :G] == SENT).all() and (got[:, G + N:] == SENT).all(), (rows, "guards overwritten")
    h.close()
    del buf, view, guard
    torch.cuda.empty_cache()


# ---- errors -------------------------------------------------------------------------

def test_ldy_smaller_than_n_is_refused(tsg):
    import torch
    M, K, N = 16, 193, 301
    arrays, X, b, alpha, ref, ref_p = _case(M, K, N)
    h = tsg.TCSCDevice(*arrays, K, N)
    Xd, bd, ad = _dev(X), _dev(b), _dev(alpha)
    buf = torch.empty((M + 2, N), device="cuda")
    _fill(buf)
    for dalpha in (None, ad.data_ptr()):
        with pytest.raises(tsg.TSGError, match="ldY=300 is less than N=301"):
            h.gemm_dev(Xd.data_ptr(), bd.data_ptr(), buf[1:].data_ptr(), M, 0, dalpha, ldY=N - 1)
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int32) == SENT).all())
    h.close()


def test_gemm_torch_into_argument_checks(tsg):
    import torch
    M, K, N = 16, 193, 301
    arrays, X, b, alpha, ref, ref_p = _case(M, K, N)
    h = tsg.TCSCDevice(*arrays, K, N)
    Xd, bd = _dev(X), _dev(b)
    big = torch.empty((M, 2 * N + 3), device="cuda")
    _fill(big)
    bad = {
        "transposed": torch.empty((N, M), device="cuda").t(),
        "column-strided": big[:, 0:2 * N:2],
        "row-overlapping": torch.empty(M * N, device="cuda").as_strided((M, N), (N - 1, 1)),
        "dtype": torch.empty((M, N), device="cuda", dtype=torch.float64),
        "device": torch.empty((M, N)),
        "shape": big[:, :N + 1],
        "rows": big[:M - 1, :N],
    }
    for name, Y in bad.items():
        with pytest.raises(tsg.TSGError):
            h.gemm_torch_into(Xd, bd, Y)
        pytest.raises(tsg.TSGError, h.gemm_torch_into, Xd, bd, Y, _dev(alpha))
    with pytest.raises(tsg.TSGError):  # gemm_torch itself still wants a contiguous Y
        h.gemm_torch(Xd, bd, big[:, :N])
    torch.cuda.synchronize()
    assert bool((big.view(torch.int32) == SENT).all())
    # one row has no next row: any row stride is accepted
    one = torch.empty(4 * N, device="cuda").as_strided((1, N), (7, 1), 5)
    h.gemm_torch_into(Xd[:1], bd, one)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(one), ref[:1].view(np.uint32))
    h.close()


# ---- a dispatcher template from before the ldY argument -------------------------------

def test_template_without_ldy_marker_is_refused(tsg, monkeypatch, tmp_path, capfd):
    """A dispatcher template that lacks the tsg_jit_args_ldy marker (built
    before the argument list grew; here: the marker's name patched out of a
    copy) is refused by the loader like a missing one -- the registration
    falls back to rx with a warning, a pinned jit fails -- and never launched."""
    libdir = os.path.dirname(tsg.LIB_PATH)
    for f in os.listdir(libdir):
        if f.endswith(".co"):
            data = open(os.path.join(libdir, f), "rb").read()
            assert b"tsg_jit_args_ldy" in data, f
            (tmp_path / f).write_bytes(data.replace(b"tsg_jit_args_ldy", b"tsg_jit_args_old"))
    monkeypatch.setenv("TSG_JIT_DIR", str(tmp_path))
    M, K, N = 70, 257, 700
    arrays, X, b, alpha, ref, ref_p = _case(M, K, N)
    h = tsg.TCSCDevice(*arrays, K, N)
    assert h.kernel_name() == "tsg_tcsc_rx_kernel"
    assert "falling back to the rx kernel" in capfd.readouterr().err
    h.set_small_m(1)
    check_strided(h, M, N, X, b, alpha, ref, ref_p, ("rx fallback", M, K, N), cases=("odd",))
    h.close()
    monkeypatch.setenv("TSG_KERNEL", "jit")
    with pytest.raises(tsg.TSGError, match="predates the dispatcher's ldY argument"):
        tsg.TCSCDevice(*arrays, K, N)
