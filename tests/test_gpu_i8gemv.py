"""The M <= 32 integer matrix-core kernel (tsg_i8gemv_kernel) on the GPU.

Every comparison is on bits, no tolerance.  The reference is test_gpu_i8mfma's:
the numpy int64 product (asserted |chain| <= 2^24) as float32, then the
contract's fp32 operations one per line.  Each case first asserts
call_i8_kernel(M) == 2 under set_i8_mfma(2), then compares the call with the
reference and with the same call on the 128 x 128 tile kernel (set_i8_small(1))
and on the walks (set_i8_mfma(1))."""
import numpy as np
import pytest

from test_gpu_i8mfma import SENT, F, _bits, _case, _handle, _ref, _w
from test_gpu_ldy import _dev
from test_gpu_ytype import _cast_bits

pytestmark = pytest.mark.gpu


def _three(h, M, call):
    """call() on the new kernel, on the tile kernel and on the walks."""
    import torch
    out = []
    for mfma, small, kernel in ((2, 0, 2), (2, 1, 1), (1, 0, 0)):
        h.set_i8_mfma(mfma)
        h.set_i8_small(small)
        assert h.call_i8_kernel(M) == kernel and h.call_i8_mfma(M) == (kernel != 0)
        out.append(call())
        torch.cuda.synchronize()
    h.set_i8_mfma(2)
    h.set_i8_small(0)
    return out


# S: the waves the launcher picks (tsg_i8gemv_pick), tn its tile columns; one edge per case:
# M 1 / 17 / 31 / 32; N 1 / 31 / 33 / 65 / 130; K 0 / 1 / 63 (fewer steps than waves), 64 S and 64 S + 64 (the steps
# divide the waves or do not), 200 and 1000 (K % 16 != 0: byte-wise X); X one byte off; and the 64-column tile.
@pytest.mark.parametrize("M,K,N,off,tn,S", [
    (1, 0, 1, 0, 32, 1), (17, 1, 31, 0, 32, 1), (31, 63, 33, 0, 32, 1), (32, 1024, 65, 0, 32, 16),
    (32, 1088, 130, 0, 32, 16), (5, 200, 130, 0, 32, 4), (8, 1000, 33, 0, 32, 16), (9, 256, 65, 1, 32, 4),
    (32, 192, 16390, 0, 64, 2), (3, 640, 16384, 0, 64, 8)],
    ids=lambda v: str(v))
def test_shapes(tsg, oracle_mod, M, K, N, off, tn, S):
    import torch
    assert tsg.i8gemv_pick(K, N) == (tn, S)
    W, X, b, _ = _case(M, K, N)
    h = _handle(tsg, oracle_mod, W)
    assert h.call_i8_kernel(33) == 1 and h.call_i8_kernel(32) == 2
    store = torch.zeros(M * K + 32, dtype=torch.int8, device="cuda")
    Xd = store[off:off + M * K].view(M, K)  # torch allocations are 16-byte aligned: off = 1 is not
    Xd.copy_(_dev(X))
    assert Xd.data_ptr() % 16 == off
    bd = _dev(b)
    new, tile, walk = _three(h, M, lambda: h.gemm_torch_x(Xd, bd))
    assert np.array_equal(_bits(new), _ref(X, W, b).view(np.uint32))
    assert np.array_equal(_bits(new), _bits(tile)) and np.array_equal(_bits(new), _bits(walk))
    h.close()


def test_split_sums(tsg, oracle_mod):
    """|chain| = 2^24 as the sum of the S = 16 waves' partials; then a W that is
    nonzero only in the k-steps of wave 5, so every other wave adds a zero tile."""
    M, K, N = 2, 131072, 32
    assert tsg.i8gemv_pick(K, N) == (32, 16)
    W = _w(K, N, 5)
    W[:, 0], W[:, 1] = 1, -1
    X = np.empty((M, K), np.int8)
    X[0, :], X[1, :] = -128, 127
    b = np.linspace(-3, 3, N).astype(F)
    Xd, bd = _dev(X), _dev(b)
    one_wave = (np.arange(K) // 64 % 16 == 5).astype(np.int32)[:, None]
    for Wi, top in ((W, 2.0 ** 24), (W * one_wave, 2.0 ** 20)):
        want = _ref(X, Wi, b)
        assert want[0, 0] == F(-top) + b[0] and want[0, 1] == F(top) + b[1]
        h = _handle(tsg, oracle_mod, Wi)
        new, tile, walk = _three(h, M, lambda: h.gemm_torch_x(Xd, bd))
        assert np.array_equal(_bits(new), want.view(np.uint32))
        assert np.array_equal(_bits(new), _bits(tile)) and np.array_equal(_bits(new), _bits(walk))
        h.close()


@pytest.mark.parametrize("variant", ["scaled", "prelu", "ex"])
@pytest.mark.parametrize("ydtype", ["float32", "float16", "bfloat16"])
def test_output_side(tsg, oracle_mod, ydtype, variant):
    """Into rows 1..M, columns 1..N+1 of an [M + 2, N + 3] sentinel buffer (odd
    ldY, odd offset: every edge of the view shares a dword with a sentinel)."""
    import torch
    M, K, N = 31, 200, 33
    W, X, b, rng = _case(M, K, N)
    dt = getattr(torch, ydtype)
    it = torch.int32 if ydtype == "float32" else torch.int16
    rs, cs = rng.uniform(0.004, 0.01, M).astype(F), rng.uniform(0.02, 0.08, N).astype(F)
    alpha = np.linspace(-0.5, 0.5, N).astype(F)
    gate = torch.from_numpy(rng.uniform(-2, 2, (M, N)).astype(F)).to(torch.bfloat16)
    res = torch.from_numpy(rng.uniform(-4, 4, (M, N)).astype(F)).to(dt)
    want = {"scaled": lambda: _ref(X, W, b, rs, cs),
            "prelu": lambda: tsg.epilogue_ref(_ref(X, W, b), "prelu", alpha=alpha),
            "ex": lambda: tsg.epilogue_ref(_ref(X, W, b, rs, cs), "relu2", mul=gate.float().numpy(),
                                           add=res.float().numpy())}[variant]()
    want = want.view(np.uint32) if ydtype == "float32" else _cast_bits(want, ydtype)
    h = _handle(tsg, oracle_mod, W)
    Xd, bd, rd, cd, ad, gd, resd = _dev(X), _dev(b), _dev(rs), _dev(cs), _dev(alpha), gate.cuda(), res.cuda()
    buf = torch.empty((M + 2, N + 3), dtype=dt, device="cuda")
    view = buf[1:M + 1, 1:N + 1]

    def call():
        buf.view(it).fill_(SENT)
        if variant == "scaled":
            h.gemm_torch_scaled(Xd, bd, view, row_scale=rd, col_scale=cd)
        elif variant == "prelu":
            h.gemm_torch_xy(Xd, bd, view, alpha=ad)
        else:
            view.copy_(resd)  # the residual is Y itself
            h.gemm_torch_ex(Xd, bd, view, act="relu2", mul=gd, add=view, row_scale=rd, col_scale=cd)
        got = _bits(view)
        outside = buf.view(it).clone()
        outside[1:M + 1, 1:N + 1] = SENT
        assert bool((outside == SENT).all()), "wrote outside the view"
        return got

    new, tile, walk = _three(h, M, call)
    assert np.array_equal(new, want) and np.array_equal(new, tile) and np.array_equal(new, walk)
    h.close()


@pytest.mark.parametrize("xdtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("norm", [False, True], ids=["actquant", "normquant"])
def test_quantising_calls(tsg, oracle_mod, norm, xdtype):
    import torch
    M, K, N = 5, 200, 130
    W, _, b, rng = _case(M, K, N)
    Xt = torch.from_numpy((rng.standard_normal((M, K)) * 3).astype(F)).to(getattr(torch, xdtype))
    gamma, eps = rng.uniform(0.5, 1.5, K).astype(F), 1e-5
    cs = rng.uniform(0.02, 0.08, N).astype(F)
    xn = tsg.rms_norm_ref(Xt.float().numpy(), gamma, eps)[0] if norm else Xt.float().numpy()
    q, deq = tsg.act_quant_ref(xn)
    want = _ref(q, W, b, deq, cs)
    h = _handle(tsg, oracle_mod, W)
    Xd, bd, cd, gd = Xt.cuda(), _dev(b), _dev(cs), _dev(gamma)

    def call():
        out = torch.zeros(M, device="cuda")
        if norm:
            Y = h.gemm_torch_normquant(Xd, bd, gd, eps, col_scale=cd, row_scale_out=out)
        else:
            Y = h.gemm_torch_actquant(Xd, bd, col_scale=cd, row_scale_out=out)
        return _bits(Y), _bits(out)

    for y, d in _three(h, M, call):
        assert np.array_equal(y, want.view(np.uint32)) and np.array_equal(d, deq.view(np.uint32))
    h.close()


def test_capture(tsg, oracle_mod):
    """Without reserve a captured call is refused and enqueues nothing; after
    reserve(8) an M = 8 call is captured and replays to the eager bits, twice."""
    import torch
    M, K, N = 8, 200, 130
    W, X, b, rng = _case(M, K, N)
    h = _handle(tsg, oracle_mod, W)
    assert h.call_i8_kernel(M) == 2
    Xd, bd = _dev(X), _dev(b)
    Y = torch.zeros((M, N), device="cuda")
    g = torch.cuda.CUDAGraph()
    with pytest.raises(tsg.TSGError, match="tcsc_hip_reserve") as e:
        with torch.cuda.graph(g):
            h.gemm_torch_x(Xd, bd, Y)
    torch.cuda.synchronize()
    assert e.value.code == 1 and not Y.any()
    h.reserve(M)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        h.gemm_torch_x(Xd, bd, Y)
    for X2 in (X, np.ascontiguousarray(X[::-1] // 2)):
        Xd.copy_(_dev(X2))
        Y.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(Y), _ref(X2, W, b).view(np.uint32))
        assert np.array_equal(_bits(Y), _bits(h.gemm_torch_x(Xd, bd)))
    del g  # destroyed here (it synchronises the device), not by a garbage collection inside a later capture
    h.close()


def test_rule(tsg):
    """The automatic rule at M <= 32 (from profiles/i8gemv_ab.jsonl,
    K = 4096, N = 16384 and 4096): every M <= 32 at a density of 1/4 and up, 8 <= M
    <= 32 at 1/16 and up, never below 1/16, below N = 4096 or below K = 4096; M = 33
    .. 63 stays on the add streams.  Then reserve(48) on such a handle, whose rule
    holds at 32 and not at 48: it builds the image, so an M = 8 call is captured."""
    import torch
    Ms = (1, 7, 8, 32, 33, 63)
    for K, N, s, want in ((4096, 4096, 4, [2, 2, 2, 2, 0, 0]), (4096, 4096, 16, [0, 0, 2, 2, 0, 0]),
                          (4096, 4096, 32, [0] * 6), (4096, 4064, 4, [0] * 6), (4032, 4096, 4, [0] * 6)):
        h = tsg.TCSCDevice(*tsg.gen_tcsc(K, N, s, 3), K, N)
        assert [h.call_i8_kernel(M) for M in Ms] == want, (K, N, s)
        h.set_i8_small(1)
        assert not any(h.call_i8_kernel(M) for M in Ms)
        with pytest.raises(tsg.TSGError) as e:
            h.set_i8_small(2)
        assert e.value.code == 1
        h.set_i8_small(0)
        if (K, N, s) == (4096, 4096, 4):
            M = 8
            X = torch.randint(-128, 128, (M, K), dtype=torch.int8, device="cuda")
            b, Y = torch.linspace(-3, 3, N, device="cuda"), torch.zeros((M, N), device="cuda")
            assert h.call_i8_mfma(48) == 0
            h.reserve(48)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                h.gemm_torch_x(X, b, Y)
            g.replay()
            torch.cuda.synchronize()
            h.set_i8_mfma(1)
            assert np.array_equal(_bits(Y), _bits(h.gemm_torch_x(X, b)))
            del g  # (as in test_capture)
        h.close()
