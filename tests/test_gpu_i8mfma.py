"""The integer matrix-core kernel (tcsc_hip_set_i8_mfma) on the GPU.

Every comparison is on bits, no tolerance.  The reference is numpy: the int64
dot product (asserted |chain| <= 2^24) as float32, then the contract's fp32
operations one per line.  Each case first asserts call_i8_mfma(M) == 1 under
mode 2, and where it says so also compares with the same call under mode 1 (the
add streams).  The shapes cross every edge of the 128 x 128 x 64 tiling: M, N
and K below, at and one past a wave tile (64) and a workgroup tile (128), a K
that is no multiple of 16 (the byte-wise X path) and K = 0."""
import numpy as np
import pytest

from test_gpu_ldy import _dev
from test_gpu_ytype import _cast_bits

pytestmark = pytest.mark.gpu
F = np.float32
SENT = 0x7FC5  # a bit pattern no result holds, in 16 and in 32 bits


def _w(K, N, seed):
    """A dense ternary W, about two thirds nonzero."""
    return np.random.default_rng(seed).integers(-1, 2, size=(K, N)).astype(np.int32)


def _ref(X8, W, b, rs=None, cs=None):
    """((chain * rs) * cs) + b in fp32, the chain from the int64 product."""
    c = X8.astype(np.int64) @ W.astype(np.int64)
    assert np.abs(c).max(initial=0) <= 2 ** 24
    t = c.astype(F)
    if rs is not None:
        t = (t * rs[:, None]).astype(F)
    if cs is not None:
        t = (t * cs[None, :]).astype(F)
    return (t + b[None, :]).astype(F)


def _case(M, K, N):
    rng = np.random.default_rng(M + 7 * K + 13 * N)
    X = rng.integers(-128, 128, size=(M, K)).astype(np.int8)
    if K:
        X[0, 0], X[-1, -1] = -128, 127
    return _w(K, N, K + N), X, np.linspace(-3, 3, N).astype(F), rng


def _handle(tsg, oracle_mod, W):
    h = tsg.TCSCDevice(*oracle_mod.tcsc_encode(W).arrays, *W.shape)
    h.set_i8_mfma(2)
    return h


def _both(h, M, call):
    """call() on the new kernel (mode 2) and on the add streams (mode 1)."""
    import torch
    out = []
    for mode in (2, 1):
        h.set_i8_mfma(mode)
        assert h.call_i8_mfma(M) == (1 if mode == 2 else 0)
        out.append(call())
        torch.cuda.synchronize()
    return out


def _bits(t):
    import torch
    it = torch.int32 if t.dtype == torch.float32 else torch.int16
    return t.contiguous().view(it).cpu().numpy().view(np.uint32 if it == torch.int32 else np.uint16)


@pytest.mark.parametrize("M,K,N", [(1, 1, 1), (33, 63, 31), (129, 65, 257), (64, 200, 128), (130, 1024, 130), (5, 0, 40)])
def test_shapes(tsg, oracle_mod, M, K, N):
    W, X, b, _ = _case(M, K, N)
    h = _handle(tsg, oracle_mod, W)
    Xd, bd = _dev(X), _dev(b)
    new, old = _both(h, M, lambda: h.gemm_torch_x(Xd, bd))
    assert np.array_equal(_bits(new), _ref(X, W, b).view(np.uint32))
    assert np.array_equal(_bits(new), _bits(old))
    h.close()


@pytest.mark.parametrize("variant", ["scaled", "prelu", "ex"])
@pytest.mark.parametrize("ydtype", ["float32", "float16", "bfloat16"])
def test_output_side(tsg, oracle_mod, ydtype, variant):
    """Into rows 1..M, columns 1..N+1 of an [M + 2, N + 3] sentinel buffer (odd
    ldY, odd offset: every edge of the view shares a dword with a sentinel)."""
    import torch
    M, K, N = 129, 200, 257
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

    new, old = _both(h, M, call)
    assert np.array_equal(new, want) and np.array_equal(new, old)
    h.close()


@pytest.mark.parametrize("xdtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("norm", [False, True], ids=["actquant", "normquant"])
def test_quantising_calls(tsg, oracle_mod, norm, xdtype):
    import torch
    M, K, N = 33, 200, 130
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

    (ynew, dnew), (yold, dold) = _both(h, M, call)
    assert np.array_equal(ynew, want.view(np.uint32)) and np.array_equal(dnew, deq.view(np.uint32))
    assert np.array_equal(ynew, yold) and np.array_equal(dnew, dold)
    h.close()


@pytest.mark.parametrize("K,runs", [(131072, 1), (131073, 0)])
def test_the_bound(tsg, oracle_mod, K, runs):
    """K = 131072: |chain| reaches exactly 2^24 and is still exact.  One row
    more and the handle is not eligible: mode 2 changes nothing."""
    M, N = 2, 32
    W = _w(K, N, 5)
    W[:, 0], W[:, 1] = 1, -1
    X = np.random.default_rng(6).integers(-128, 128, size=(M, K)).astype(np.int8)
    if runs:
        X[0, :], X[1, :] = -128, 127
    b = np.linspace(-3, 3, N).astype(F)
    want = _ref(X, W, b)
    assert not runs or (want[0, 0] == F(-2.0 ** 24) + b[0] and want[0, 1] == F(2.0 ** 24) + b[1])
    h = _handle(tsg, oracle_mod, W)
    assert h.call_i8_mfma(M) == runs
    assert np.array_equal(_bits(h.gemm_torch_x(_dev(X), _dev(b))), want.view(np.uint32))
    h.close()


def test_modes(tsg, oracle_mod):
    """The automatic rule (from profiles/i8mfma_ab.jsonl: M >= 64
    at a density of 1/4 and up, M >= 512 at 1/16 and up, else never), the
    setter's range, and a BlockedTCSC handle, which mode 2 leaves alone."""
    K, N = 64, 40
    for nnz, want in ((K * N // 4, [0, 1, 1, 1]), (K * N // 4 - 1, [0, 0, 1, 1]), (K * N // 16, [0, 0, 1, 1]),
                      (K * N // 16 - 1, [0, 0, 0, 0])):
        W = np.zeros(K * N, np.int32)
        W[:nnz] = 1
        h = tsg.TCSCDevice(*oracle_mod.tcsc_encode(W.reshape(K, N)).arrays, K, N)
        assert [h.call_i8_mfma(M) for M in (63, 64, 512, 4096)] == want, nnz
        with pytest.raises(tsg.TSGError) as e:
            h.set_i8_mfma(3)
        assert e.value.code == 1
        h.close()
    arrays = oracle_mod.tcsc_encode(_w(K, N, 1)).arrays
    hb = tsg.TCSCDevice.from_blocked(*tsg.tcsc_to_blocked(*arrays, K, N, 32), K, N, 32)
    hb.set_i8_mfma(2)
    assert hb.call_i8_mfma(64) == 0
    hb.close()


def test_capture(tsg, oracle_mod):
    """Without reserve a captured mode-2 call is refused and enqueues nothing;
    after reserve it is captured and replays to the eager bits, twice."""
    import torch
    M, K, N = 70, 200, 130
    W, X, b, rng = _case(M, K, N)
    h = _handle(tsg, oracle_mod, W)
    assert h.call_i8_mfma(M) == 1
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
    h.close()
