"""The 16-bit matrix-core kernel (tcsc_hip_set_x16_mfma) on the GPU, fp16 and bf16.

Integer-valued X (|x| <= 64, so every partial sum is an integer <= 2^24 and any
summation order is exact): on bits, against the numpy int64 reference and the
same call with the mode off.  Fractional X: against float64 within the
contract's derived bound.  The shapes cross every edge of the 128 x 256 x 64
tiling, the 64-row kernel variant (M <= 64), a K that is no multiple of 8 and
an X base off by one element (the element-wise loads), and K = 0."""
import numpy as np
import pytest

from test_gpu_i8mfma import SENT, _bits, _ref, _w
from test_gpu_ldy import _dev
from test_gpu_ytype import _cast_bits

pytestmark = pytest.mark.gpu
F = np.float32
XTYPES = ["float16", "bfloat16"]


def _xt(tsg, xdtype):
    return tsg.TSG_X_F16 if xdtype == "float16" else tsg.TSG_X_BF16


def _int_case(M, K, N):
    rng = np.random.default_rng(M + 7 * K + 13 * N)
    X = rng.integers(-64, 65, size=(M, K)).astype(F)
    return _w(K, N, K + N), X, np.linspace(-3, 3, N).astype(F), rng


def _xdev(X, xdtype, off=0):
    """X on the device in its 16-bit type, `off` elements into its buffer."""
    import torch
    buf = torch.zeros(X.size + off, dtype=getattr(torch, xdtype), device="cuda")
    buf[off:] = torch.from_numpy(X).reshape(-1).to(buf.dtype)
    return buf[off:].view(X.shape)


def _handle(tsg, oracle_mod, W):
    return tsg.TCSCDevice(*oracle_mod.tcsc_encode(W).arrays, *W.shape)


def _both(tsg, h, M, xdtype, call):
    """call() on the new kernel (mode 1) and as the library runs it without (mode 0)."""
    import torch
    out = []
    for mode in (1, 0):
        h.set_x16_mfma(mode)
        assert h.call_x16_mfma(M, _xt(tsg, xdtype)) == mode
        out.append(call())
        torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("xdtype", XTYPES)
@pytest.mark.parametrize("M,K,N,off", [(1, 1, 1, 0), (33, 63, 31, 0), (129, 65, 257, 0), (64, 200, 128, 0),
                                       (130, 1024, 130, 0), (5, 0, 40, 0), (65, 203, 300, 0), (70, 200, 513, 1)])
def test_integer_x(tsg, oracle_mod, M, K, N, off, xdtype):
    W, X, b, _ = _int_case(M, K, N)
    h = _handle(tsg, oracle_mod, W)
    Xd, bd = _xdev(X, xdtype, off), _dev(b)
    new, old = _both(tsg, h, M, xdtype, lambda: h.gemm_torch_x(Xd, bd))
    assert np.array_equal(_bits(new), _ref(X, W, b).view(np.uint32))
    assert np.array_equal(_bits(new), _bits(old))
    h.close()


@pytest.mark.parametrize("xdtype", XTYPES)
@pytest.mark.parametrize("variant", ["scaled", "prelu", "ex"])
@pytest.mark.parametrize("ydtype", ["float32", "float16", "bfloat16"])
def test_output_side(tsg, oracle_mod, ydtype, variant, xdtype):
    """Into rows 1..M, columns 1..N+1 of an [M + 2, N + 3] sentinel buffer (odd
    ldY, odd offset: every edge of the view shares a dword with a sentinel)."""
    import torch
    M, K, N = 129, 200, 257
    W, X, b, rng = _int_case(M, K, N)
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
    Xd, bd, rd, cd, ad, gd, resd = _xdev(X, xdtype), _dev(b), _dev(rs), _dev(cs), _dev(alpha), gate.cuda(), res.cuda()
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

    new, old = _both(tsg, h, M, xdtype, call)
    assert np.array_equal(new, want) and np.array_equal(new, old)
    h.close()


def _frac_case(xdtype):
    import torch
    M, K, N = 129, 200, 257
    rng = np.random.default_rng(77)
    W = _w(K, N, 3)
    X = rng.uniform(0.25, 1.0, (M, K)) * rng.choice([-1.0, 1.0], (M, K))
    X = torch.from_numpy(X.astype(F)).to(getattr(torch, xdtype)).float().numpy()  # exactly 16-bit values
    return M, K, N, W, X, np.linspace(-3, 3, N).astype(F)


@pytest.mark.parametrize("xdtype", XTYPES)
def test_fractional_x_within_the_bound(tsg, oracle_mod, xdtype):
    """|chain - exact| <= d u S / (1 - d u), d = c + ceil(K / 16), u = 2^-23, plus
    2^-23 |y| for the final + b.  About 2e-3 here, where a dropped or misplaced
    term is >= 0.25; the reference's own fp32 evaluation must lie inside it."""
    M, K, N, W, X, b = _frac_case(xdtype)
    want = X.astype(np.float64) @ W + b
    u = 2.0 ** -23
    d = (W != 0).sum(0)[None, :] + -(-K // 16)
    tol = d * u * (np.abs(X).astype(np.float64) @ np.abs(W)) / (1 - d * u) + u * np.abs(want)
    assert tol.max() < 5e-3
    assert (np.abs(((X @ W.astype(F)).astype(F) + b).astype(np.float64) - want) <= tol).all()
    h = _handle(tsg, oracle_mod, W)
    h.set_x16_mfma(1)
    assert h.call_x16_mfma(M, _xt(tsg, xdtype)) == 1
    Xd, bd = _xdev(X, xdtype), _dev(b)
    Y = h.gemm_torch_x(Xd, bd).cpu().numpy().astype(np.float64)
    err = np.abs(Y - want)
    print("max err / tol:", (err / tol).max(), "max err:", err.max())
    assert (err <= tol).all()

    # an inf in one row and a NaN in another: every other row keeps its bytes
    X2 = X.copy()
    X2[3, 17], X2[70, 150] = np.inf, np.nan
    Y2 = h.gemm_torch_x(_xdev(X2, xdtype), bd)
    keep = [m for m in range(M) if m not in (3, 70)]
    assert np.array_equal(_bits(Y2)[keep], _bits(h.gemm_torch_x(Xd, bd))[keep])
    h.close()


def test_routing(tsg, oracle_mod):
    """Mode 1 leaves an fp32 X, an int8 X and a quantising call where they were."""
    import torch
    M, K, N = 70, 200, 130
    W, X, b, rng = _int_case(M, K, N)
    h = _handle(tsg, oracle_mod, W)
    bd = _dev(b)
    calls = {"f32": lambda: h.gemm_torch_x(_dev(X), bd), "i8": lambda: h.gemm_torch_x(_dev(X.astype(np.int8)), bd),
             "actquant": lambda: h.gemm_torch_actquant(_xdev(X / 7, "bfloat16"), bd)}
    got = {}
    for mode in (0, 1):
        h.set_x16_mfma(mode)
        assert h.call_x16_mfma(M, tsg.TSG_X_F32) == 0 and h.call_x16_mfma(M, tsg.TSG_X_I8) == 0
        assert h.call_x16_mfma(M, tsg.TSG_X_BF16) == mode and h.call_x16_mfma(0, tsg.TSG_X_BF16) == 0
        got[mode] = {k: _bits(f()) for k, f in calls.items()}
        torch.cuda.synchronize()
    for k in calls:
        assert np.array_equal(got[0][k], got[1][k]), k
    with pytest.raises(tsg.TSGError) as e:
        h.set_x16_mfma(2)
    assert e.value.code == 1
    h.close()


def test_capture(tsg, oracle_mod):
    """Without reserve a captured call is refused and enqueues nothing; after
    reserve it is captured and replays to the eager bits, twice."""
    import torch
    M, K, N = 70, 200, 130
    W, X, b, rng = _int_case(M, K, N)
    h = _handle(tsg, oracle_mod, W)
    h.set_x16_mfma(1)
    Xd, bd = _xdev(X, "bfloat16"), _dev(b)
    Y = torch.zeros((M, N), device="cuda")
    g = torch.cuda.CUDAGraph()
    with pytest.raises(tsg.TSGError, match="tcsc_hip_reserve"):  # (unbound: no frame cycle keeps a graph for the collector)
        with torch.cuda.graph(g):
            h.gemm_torch_x(Xd, bd, Y)
    torch.cuda.synchronize()
    assert not Y.any()
    h.reserve(M)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        h.gemm_torch_x(Xd, bd, Y)
    for X2 in (X, np.ascontiguousarray(-X[::-1])):
        Xd.copy_(_xdev(X2, "bfloat16"))
        Y.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(Y), _bits(h.gemm_torch_x(Xd, bd)))
    assert np.array_equal(_bits(Y), _ref(np.ascontiguousarray(-X[::-1]), W, b).view(np.uint32))
    h.close()
