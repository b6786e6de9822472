"""The fused gate/up call (tcsc_hip_gemm_dev_glu: tsg_i8glu_kernel and, at
M <= 32, tsg_i8glu_gemv_kernel) on the GPU.

Every comparison is on bits, no tolerance.  The reference is numpy: the int64
product of each W (asserted |chain| <= 2^24) as float32, the contract's fp32
operations one per line (test_gpu_i8mfma's _ref), then tsg.epilogue_ref with u
as its `mul` -- or, when the call has a `mul` of its own, u multiplied in one
line before it.  The asymmetric activation tells a swapped pair of images."""
import numpy as np
import pytest

from test_gpu_i8mfma import SENT, F, _bits, _case, _handle, _ref, _w
from test_gpu_ldy import _dev
from test_gpu_ytype import _cast_bits

pytestmark = pytest.mark.gpu


def _want(tsg, q, Wg, Wu, b, bu, act, rs=None, cs=None, csu=None, alpha=None, mul=None, add=None):
    u = _ref(q, Wu, bu, rs, csu)
    y = _ref(q, Wg, b, rs, cs)
    if mul is None:
        return tsg.epilogue_ref(y, act, alpha=alpha, mul=u, add=add)
    a = (tsg.epilogue_ref(y, act, alpha=alpha) * u).astype(F)
    return tsg.epilogue_ref(a, "none", mul=mul, add=add)


def _pair(tsg, oracle_mod, M, K, N):
    """_case's W, X and b as the gate, a second W and bias as the up projection."""
    Wg, X, b, rng = _case(M, K, N)
    Wu, bu = _w(K, N, K + N + 1), np.linspace(2, -1, N).astype(F)
    return Wg, Wu, X, b, bu, rng, _handle(tsg, oracle_mod, Wg), _handle(tsg, oracle_mod, Wu)


# S: the waves of the split-K variant (tsg_i8glu_pick), 0: M > 32, the tile variant.  One edge per case --
# tile: below the granule; byte-wise X (K % 16 != 0); one past everything; three M tiles and N past a 128 padding
# boundary; K = 0 (Y = act(b) * b_up); X one byte off.  Split-K: the smallest; one step; steps = S; steps that do
# not divide by S; byte-wise X; 10 granules padded to 16 (the XCD numbering) and X one byte off; 18 steps at M = 31.
@pytest.mark.parametrize("M,K,N,off,S", [
    (33, 63, 31, 0, 0), (64, 200, 64, 0, 0), (65, 65, 65, 0, 0), (129, 1024, 130, 0, 0), (40, 0, 40, 0, 0),
    (130, 256, 33, 1, 0),
    (1, 1, 1, 0, 1), (17, 63, 33, 0, 1), (32, 512, 65, 0, 8), (32, 576, 130, 0, 8), (5, 200, 95, 0, 4),
    (9, 256, 577, 1, 4), (31, 1100, 32, 0, 8)], ids=lambda v: str(v))
def test_shapes(tsg, oracle_mod, M, K, N, off, S):
    import torch
    Wg, Wu, X, b, bu, _, hg, hu = _pair(tsg, oracle_mod, M, K, N)
    store = torch.zeros(M * K + 32, dtype=torch.int8, device="cuda")
    Xd = store[off:off + M * K].view(M, K)  # torch allocations are 16-byte aligned: off = 1 is not
    Xd.copy_(_dev(X))
    assert Xd.data_ptr() % 16 == off
    bd, bud = _dev(b), _dev(bu)
    want = _want(tsg, X, Wg, Wu, b, bu, "relu2").view(np.uint32)
    assert np.array_equal(_bits(hg.gemm_torch_glu(hu, Xd, bd, bud)), want)
    if M <= 32:  # the same call on the tile variant
        assert tsg.i8glu_pick(K, N) == (32, S)
        hg.set_i8_small(1)
        assert np.array_equal(_bits(hg.gemm_torch_glu(hu, Xd, bd, bud)), want)
    for h in (hg, hu):  # the two-call sequence on the add streams
        h.set_i8_mfma(1)
    U = hu.gemm_torch_ex(Xd, bud)
    assert np.array_equal(_bits(hg.gemm_torch_ex(Xd, bd, act="relu2", mul=U)), want)
    hg.close(), hu.close()


@pytest.mark.parametrize("M", [2, 34])
def test_extremes(tsg, oracle_mod, M):
    """|chain| = 2^24 of both matrices in one element (row 0, column 0: gate - 2^24, up + 2^24; row 1 nearly so
    with the signs exchanged); then an all-zero up W: u = b_up exactly."""
    K, N = 131072, 33
    Wg, Wu = _w(K, N, 5), _w(K, N, 6)
    Wg[:, 0], Wu[:, 0] = 1, -1
    X = np.empty((M, K), np.int8)
    X[0::2, :], X[1::2, :] = -128, 127
    b, bu = np.linspace(-3, 3, N).astype(F), np.linspace(2, -1, N).astype(F)
    Xd, bd, bud = _dev(X), _dev(b), _dev(bu)
    hg = _handle(tsg, oracle_mod, Wg)
    for Wi in (Wu, np.zeros_like(Wu)):
        want = _want(tsg, X, Wg, Wi, b, bu, "none")
        top = F(2.0 ** 24)
        assert want[0, 0] == (-top + b[0]) * ((top if Wi.any() else F(0)) + bu[0])
        hu = _handle(tsg, oracle_mod, Wi)
        assert np.array_equal(_bits(hg.gemm_torch_glu(hu, Xd, bd, bud, act="none")), want.view(np.uint32))
        hu.close()
    hg.close()


@pytest.mark.parametrize("M", [31, 70])
@pytest.mark.parametrize("act", ["none", "prelu", "relu"])
@pytest.mark.parametrize("ydtype", ["float32", "float16", "bfloat16"])
def test_output_side(tsg, oracle_mod, ydtype, act, M):
    """Both scales, the up column scale, a bf16 mul and add = Y in place, into rows 1..M, columns 1..N+1 of an
    [M + 2, N + 3] sentinel buffer (odd ldY, odd offset: every edge of the view shares a dword with a sentinel)."""
    import torch
    K, N = 200, 33
    Wg, Wu, X, b, bu, rng, hg, hu = _pair(tsg, oracle_mod, M, K, N)
    dt = getattr(torch, ydtype)
    it = torch.int32 if ydtype == "float32" else torch.int16
    rs = rng.uniform(0.004, 0.01, M).astype(F)
    cs, csu = rng.uniform(0.02, 0.08, N).astype(F), rng.uniform(0.02, 0.08, N).astype(F)
    alpha = np.linspace(-0.5, 0.5, N).astype(F) if act == "prelu" else None
    mul = torch.from_numpy(rng.uniform(-2, 2, (M, N)).astype(F)).to(torch.bfloat16)
    res = torch.from_numpy(rng.uniform(-4, 4, (M, N)).astype(F)).to(dt)
    want = _want(tsg, X, Wg, Wu, b, bu, act, rs, cs, csu, alpha, mul.float().numpy(), res.float().numpy())
    want = want.view(np.uint32) if ydtype == "float32" else _cast_bits(want, ydtype)
    buf = torch.empty((M + 2, N + 3), dtype=dt, device="cuda")
    buf.view(it).fill_(SENT)
    view = buf[1:M + 1, 1:N + 1]
    view.copy_(res.cuda())  # the residual is Y itself
    hg.gemm_torch_glu(hu, _dev(X), _dev(b), _dev(bu), view, act=act, alpha=None if alpha is None else _dev(alpha),
                      mul=mul.cuda(), add=view, row_scale=_dev(rs), col_scale=_dev(cs), col_scale_up=_dev(csu))
    assert np.array_equal(_bits(view), want)
    outside = buf.view(it).clone()
    outside[1:M + 1, 1:N + 1] = SENT
    assert bool((outside == SENT).all()), "wrote outside the view"
    hg.close(), hu.close()


@pytest.mark.parametrize("M", [7, 70])
@pytest.mark.parametrize("xdtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("quant", ["act", "norm"])
def test_quant(tsg, oracle_mod, quant, xdtype, M):
    """The row pass runs once: Y and row_scale_out are the two-call sequence's bytes (the parent's code, with
    reference tests of its own) and the numpy reference's on act_quant_ref / rms_norm_ref's q and deq."""
    import torch
    K, N = 200, 65
    Wg, Wu, _, b, bu, rng, hg, hu = _pair(tsg, oracle_mod, M, K, N)
    Xt = torch.from_numpy((rng.standard_normal((M, K)) * 3).astype(F)).to(getattr(torch, xdtype))
    gamma, eps = (rng.uniform(0.5, 1.5, K).astype(F), 1e-5) if quant == "norm" else (None, None)
    cs, csu = rng.uniform(0.02, 0.08, N).astype(F), rng.uniform(0.02, 0.08, N).astype(F)
    xn = tsg.rms_norm_ref(Xt.float().numpy(), gamma, eps)[0] if quant == "norm" else Xt.float().numpy()
    q, deq = tsg.act_quant_ref(xn)
    want = _want(tsg, q, Wg, Wu, b, bu, "relu2", deq, cs, csu)
    Xd, bd, bud, cd, cud = Xt.cuda(), _dev(b), _dev(bu), _dev(cs), _dev(csu)
    kw = dict(quant=quant, gamma=None if gamma is None else _dev(gamma), eps=eps)
    out, out1, out2 = (torch.zeros(M, device="cuda") for _ in range(3))
    Y = hg.gemm_torch_glu(hu, Xd, bd, bud, col_scale=cd, col_scale_up=cud, row_scale_out=out, **kw)
    U = hu.gemm_torch_ex(Xd, bud, col_scale=cud, row_scale_out=out1, **kw)
    Y2 = hg.gemm_torch_ex(Xd, bd, act="relu2", mul=U, col_scale=cd, row_scale_out=out2, **kw)
    assert np.array_equal(_bits(Y), _bits(Y2)) and np.array_equal(_bits(Y), want.view(np.uint32))
    for o in (out, out1, out2):
        assert np.array_equal(_bits(o), deq.view(np.uint32))
    hg.close(), hu.close()


def test_capture(tsg, oracle_mod):
    """Without reserve_glu a captured call is refused, naming it, and enqueues nothing; after reserve_glu(8) an
    M = 8 call is captured and replays to the eager bits, twice."""
    import torch
    M, K, N = 8, 200, 130
    Wg, Wu, X, b, bu, _, hg, hu = _pair(tsg, oracle_mod, M, K, N)
    Xd, bd, bud = _dev(X), _dev(b), _dev(bu)
    Y = torch.zeros((M, N), device="cuda")
    g = torch.cuda.CUDAGraph()
    with pytest.raises(tsg.TSGError, match="tcsc_hip_reserve_glu") as e:
        with torch.cuda.graph(g):
            hg.gemm_torch_glu(hu, Xd, bd, bud, Y)
    torch.cuda.synchronize()
    assert e.value.code == 1 and not Y.any()
    hg.reserve_glu(hu, M)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hg.gemm_torch_glu(hu, Xd, bd, bud, Y)
    for X2 in (X, np.ascontiguousarray(X[::-1] // 2)):
        Xd.copy_(_dev(X2))
        Y.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(Y), _want(tsg, X2, Wg, Wu, b, bu, "relu2").view(np.uint32))
        assert np.array_equal(_bits(Y), _bits(hg.gemm_torch_glu(hu, Xd, bd, bud)))
    del g  # destroyed here (it synchronises the device), not by a garbage collection inside a later capture
    hg.close(), hu.close()
