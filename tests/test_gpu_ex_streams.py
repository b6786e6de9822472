"""The descriptor call (tcsc_hip_gemm_dev_ex, TCSCDevice.gemm_torch_ex) on one
handle from two streams, issued back to back with no host sync in between: the
quantisation scratch (inv, deq, rn and, for a small-M walk, the int8 copy of X)
is shared by every call of the handle, and include/ternary_spgemm.h promises
that it is ordered across streams exactly like the work buffer.  The style is
test_gpu_streams.test_two_streams_one_handle's and
test_gpu_xtype.test_xtype_work_buffer_hand_over's, which use the plain fp32 and
the typed-X call only.

What these establish: under the issue pattern that the header describes, every
result is bit for bit the CPU reference's (rms_norm_ref, act_quant_ref, the
oracle's chain, expect32, epilogue_ref, the cast), every round equals the first
and row_scale_out equals deq each time.  What they do not establish: that the
wait between the streams exists.  A pass can also mean that the kernels of the
two streams did not overlap on this run; a missing wait shows here only when
they do."""
import numpy as np
import pytest

from test_gpu_ldy import _dev
from test_gpu_scaled import _got_bits, _ybits_of, expect32
from test_gpu_xtype import _tdtype

pytestmark = pytest.mark.gpu

F = np.float32


def _round_to(a32, dtype):
    """fp32 numpy -> (CPU tensor of the type, the tensor widened back to fp32)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a32, F)).to(_tdtype(dtype))
    return t, t.to(torch.float32).numpy()


def _expect(tsg, O, t, Xw, rows, quant, g, eps, cs, b, act, Gw, Rw, ydtype):
    """(the bits of the Y type on these rows, deq on these rows): the contract, step by step."""
    Xc, deq = np.ascontiguousarray(Xw[rows]), None
    if quant == "norm":
        Xc = tsg.rms_norm_ref(Xc, g, eps)[0]
    if quant:
        q, deq = tsg.act_quant_ref(Xc)
        Xc = q.astype(F)
    chain = O.base_tcsc(Xc, t, np.zeros(b.shape[0], F))
    y = expect32(chain, deq, cs, b)
    want = tsg.epilogue_ref(y, act, None, None if Gw is None else np.ascontiguousarray(Gw[rows]),
                            None if Rw is None else np.ascontiguousarray(Rw[rows]))
    assert np.isfinite(want).all()
    return _ybits_of(want, ydtype), deq


def _activations(M, K, seed):
    rng = np.random.default_rng(seed)
    return _round_to((rng.standard_normal((M, K)) * 1.5 * rng.uniform(0.5, 2.0, (M, 1))).astype(F), "bfloat16")


def _operands(M, N, seed):
    """A bf16 gate +-U[0.5, 2) and a bf16 residual U[-64, 64)."""
    rng = np.random.default_rng(seed)
    G = rng.uniform(0.5, 2.0, (M, N)) * rng.choice([-1.0, 1.0], (M, N))
    return _round_to(G.astype(F), "bfloat16"), _round_to(rng.uniform(-64.0, 64.0, (M, N)).astype(F), "bfloat16")


def _deq_bits(t):
    import torch
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _two_streams(tsg, O, h, t, M, K, N, rows, rounds, quants):
    """Stream 1: quants[0] with relu2 and a gate; stream 2: quants[1] with an
    in-place residual; different X, bf16 throughout.  `rounds` rounds, no host
    sync between the calls."""
    import torch
    bf16 = torch.bfloat16
    b = np.linspace(-1, 1, N).astype(F)
    cs = np.random.default_rng(3).uniform(0.5, 2.0, N).astype(F)
    g, eps = np.random.default_rng(4).uniform(0.5, 1.5, K).astype(F), 1e-5
    (X1t, X1w), (X2t, X2w) = _activations(M, K, 1), _activations(M, K, 2)
    (Gt, Gw), (Rt, Rw) = _operands(M, N, 5)
    want1, deq1 = _expect(tsg, O, t, X1w, rows, quants[0], g, eps, cs, b, "relu2", Gw, None, "bfloat16")
    want2, deq2 = _expect(tsg, O, t, X2w, rows, quants[1], g, eps, cs, b, "none", None, Rw, "bfloat16")
    assert not np.array_equal(want1, want2)
    X1, X2, Gd, Rd, bd, cd, gd = X1t.cuda(), X2t.cuda(), Gt.cuda(), Rt.cuda(), _dev(b), _dev(cs), _dev(g)
    norm = lambda q: dict(gamma=gd, eps=eps) if q == "norm" else {}
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(rounds):  # (allocated before the calls: nothing below waits for the host)
        outs.append((torch.empty((M, N), dtype=bf16, device="cuda"), Rd.clone(), torch.zeros(M, device="cuda"),
                     torch.zeros(M, device="cuda")))
    torch.cuda.synchronize()
    for Y1, Y2, d1, d2 in outs:
        with torch.cuda.stream(s1):
            h.gemm_torch_ex(X1, bd, Y1, act="relu2", mul=Gd, col_scale=cd, quant=quants[0], row_scale_out=d1,
                            **norm(quants[0]))
        with torch.cuda.stream(s2):
            h.gemm_torch_ex(X2, bd, Y2, add=Y2, col_scale=cd, quant=quants[1], row_scale_out=d2, **norm(quants[1]))
    torch.cuda.synchronize()
    for i, (Y1, Y2, d1, d2) in enumerate(outs):
        assert np.array_equal(_got_bits(Y1, "bfloat16")[rows], want1), ("stream 1", quants[0], "round", i)
        assert np.array_equal(_got_bits(Y2, "bfloat16")[rows], want2), ("stream 2", quants[1], "round", i)
        assert np.array_equal(_deq_bits(d1)[rows], deq1.view(np.uint32)), ("stream 1 row_scale_out", i)
        assert np.array_equal(_deq_bits(d2)[rows], deq2.view(np.uint32)), ("stream 2 row_scale_out", i)
        for got, first in zip((Y1, Y2, d1, d2), outs[0]):
            assert torch.equal(got.view(torch.int8), first.view(torch.int8)), ("round", i, "differs from the first")


def test_ex_two_streams_on_the_images(tsg, oracle_mod):
    """The images at M = 1024: a norm-quant call with relu2 and a gate on one
    stream, an act-quant call with an in-place residual on the other; inv, deq
    and rn of the scratch belong to one call at a time."""
    O = oracle_mod
    K, N, M = 2048, 4096, 1024
    t = O.tcsc_encode(O.gen_ternary(K, N, 4, 21))
    h = tsg.TCSCDevice(*t.arrays, K, N)
    h.reserve(M)
    assert h.call_kernel(M) != "tsg_tcsc_ell_kernel"
    _two_streams(tsg, O, h, t, M, K, N, np.r_[0:64, M - 64:M], 4, ("norm", "act"))
    h.close()


def test_ex_two_streams_on_the_walks_int8_copy(tsg, oracle_mod):
    """The same W through the forced small-M walk at M = 16: both streams
    quantise into the one int8 copy of X that the walk reads."""
    O = oracle_mod
    K, N, M = 2048, 4096, 16
    t = O.tcsc_encode(O.gen_ternary(K, N, 4, 21))
    h = tsg.TCSCDevice(*t.arrays, K, N)
    h.set_small_m(2)
    h.reserve(M)
    assert h.call_kernel(M) == "tsg_tcsc_ell_kernel"
    _two_streams(tsg, O, h, t, M, K, N, np.arange(M), 8, ("act", "act"))
    h.close()


def test_ex_scratch_hand_over(tsg, oracle_mod):
    """Alternating across two streams on one handle: a plain fp32 descriptor
    call that reads X itself (one launch, no work buffer), a norm-quant call
    (work buffer and scratch) and a plain bf16 call (staged, no scratch), each
    with relu and a residual."""
    import torch
    O = oracle_mod
    M, K, N = 64, 388, 700
    t = O.tcsc_encode(O.gen_ternary(K, N, 4, 1000 * M + K + N))
    h = tsg.TCSCDevice(*t.arrays, K, N)
    assert h.call_kernel(M) == "tsg_jit64_kernel"
    rows = np.arange(M)
    b = np.linspace(-3, 3, N).astype(F)
    g, eps = np.random.default_rng(4).uniform(0.5, 1.5, K).astype(F), 1e-5
    cs_q = np.random.default_rng(3).uniform(0.5, 2.0, N).astype(F)
    cs_p = (cs_q * F(2.0 ** -20)).astype(F)  # init_x_frac's chains reach 2^25
    X32 = O.init_x_frac(M, K, M + 11)
    Xbt, Xbw = _round_to(X32, "bfloat16")
    Xnt, Xnw = _activations(M, K, 7)
    (_, _), (Rt, Rw) = _operands(M, N, 8)
    kinds = {  # name -> (X on the device, X widened, quant, col_scale, Y type)
        "fp32": (_dev(X32), X32, None, cs_p, "float32"),
        "norm": (Xnt.cuda(), Xnw, "norm", cs_q, "bfloat16"),
        "bf16": (Xbt.cuda(), Xbw, None, cs_p, "bfloat16"),
    }
    want = {n: _expect(tsg, O, t, Xw, rows, q, g, eps, cs, b, "relu", None, Rw, yd)
            for n, (Xd, Xw, q, cs, yd) in kinds.items()}
    assert not np.array_equal(want["norm"][0], want["bf16"][0])
    bd, gd, Rd = _dev(b), _dev(g), Rt.cuda()
    cds = {n: _dev(v[3]) for n, v in kinds.items()}

    def call(n, d):
        Xd, Xw, q, cs, yd = kinds[n]
        kw = dict(gamma=gd, eps=eps, row_scale_out=d) if q else {}
        return h.gemm_torch_ex(Xd, bd, act="relu", add=Rd, out_dtype=_tdtype(yd), col_scale=cds[n], quant=q, **kw)

    for n in kinds:  # the image is compiled before the checked calls
        call(n, torch.zeros(M, device="cuda"))
    torch.cuda.synchronize()
    assert h.call_launches(kinds["fp32"][0], M) == 1  # the fp32 call reads X itself
    s = (torch.cuda.Stream(), torch.cuda.Stream())
    order = ["fp32", "norm", "bf16"] * 4  # twelve calls, each kind on both streams and after both others
    ds = [torch.zeros(M, device="cuda") for _ in order]
    torch.cuda.synchronize()
    outs = []
    for i, n in enumerate(order):
        with torch.cuda.stream(s[i % 2]):
            outs.append(call(n, ds[i]))
    torch.cuda.synchronize()
    for i, (n, Y, d) in enumerate(zip(order, outs, ds)):
        bits, deq = want[n]
        assert np.array_equal(_got_bits(Y, kinds[n][4]), bits), (i, n, "on stream", i % 2)
        if deq is not None:
            assert np.array_equal(_deq_bits(d), deq.view(np.uint32)), (i, n, "row_scale_out")
    assert h.info()["work_bytes"] > 0  # the bf16 and the norm-quant calls were staged
    h.close()
