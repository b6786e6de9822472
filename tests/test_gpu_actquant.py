"""Fused per-row int8 activation quantisation on the device-pointer calls
(tcsc_hip_gemm_dev_actquant, TCSCDevice.gemm_torch_actquant) through every
kernel family on the GPU.

The contract (include/ternary_spgemm.h; tspgemm.act_quant_ref states it in
numpy): all fp32 on the widened X, one rounding per operation,

    a = max(max_k |x[m,k]|, 1e-5);  inv = 127 / a;  deq[m] = a / 127
    q[m,k] = min(max(rint(x[m,k] * inv), -127), 127)          ties to even
    Y = the scaled call's on the int8 X = q with row_scale = deq

so the expected Y is test_gpu_scaled.expect32(base_tcsc(q), deq, cs, b, alpha),
then test_gpu_ytype._cast_bits.  Everything is compared as integers.

Inputs (the case builder, _acase, asserts all of this on the CPU; the CPU file
test_actquant_ref.py runs it for every shape used here).  A random X cannot
tell the contract from its neighbours (x / deq, (x / a) * 127, (x * 127) / a,
inv = 127 * (1 / a), float64 arithmetic, round half away): they give the same q
in every element.  So X is made of near-ties.  Row m has its maximum a[m] = 3 *
U[0.5, 2) at k = (37 m) % K (row 0 at k = 0, row 1 at k = K - 1), negative in
odd rows; every other element is fp32((j + 0.5) * a / 127) moved by -2..+2
ulps, j uniform in -126..125.  After them come rows with a = 127 / 8 exactly and
x = (j + 0.5) / 8 -- exact ties, inv = 8 -- then an all-zero row and a row whose
maximum, 3e-6, is below the eps.  (M >= 32: four exact-tie rows; M = 16: two;
M = 4: one; M = 1: the near-tie row alone.  The zero row and the row below
the eps from M = 16 on.)  On an fp32 X each of the six variants differs from
the contract's q in at least 3 % of the elements, and half-away in at least
30 % of the exact-tie rows' elements.  A 16-bit X is that X cast to the type
(the exact-tie rows survive the cast unchanged; the near-ties mostly do not):
half-away is told apart on the tie rows and every other variant by at least
one element -- the arithmetic after the widening is the fp32 code.  The row
maximum is exactly a[m] (after the cast: the cast a[m]), and the expected Y is
finite in the Y type.

Each family case asserts the kernel that ran, then runs the plain and the PReLU
call with and without the column scale into a dense output and into the
odd-stride sentinel view (rows 1..M, columns 1..N+1 of an [M + 2, N + 3] buffer
of NaN patterns), where only the view may change; row_scale_out is the slice
[3, 3 + M) of a sentinel-filled buffer, where only the slice may change and
must hold deq bit for bit; X, b, alpha and the column scale are unchanged."""
import functools

import numpy as np
import pytest

from test_gpu_ldy import SENT, _bits, _dev, _jit_handle
from test_gpu_scaled import _draw_scales, _got_bits, _outputs, _ybits_of, expect32
from test_gpu_xtype import _tdtype, _x_on_device
from test_gpu_ytype import SENT16, YMAX, _fill16

pytestmark = pytest.mark.gpu

YDTYPES = ("float32", "float16", "bfloat16")
XDTYPES = ("float32", "float16", "bfloat16")

# (M, K, N) of every family case below, and of the type product, with its B
FAMILY_SHAPES = [(1, 193, 301, 0), (4, 193, 301, 0), (16, 193, 301, 0), (63, 193, 700, 0), (65, 388, 700, 0),
                 (130, 193, 301, 0), (65, 193, 700, 0), (130, 388, 700, 0), (130, 385, 700, 64), (65, 1030, 301, 0)]
TYPE_SHAPES = [(16, 193, 301), (65, 388, 700)]


@pytest.fixture(autouse=True)
def _oracle_built(oracle_mod):
    """The cached cases below import the oracle themselves: it is built first."""


# ---- the case builder ---------------------------------------------------------------

F = np.float32


def _clamp(t):
    return np.minimum(np.maximum(t, F(-127.0)), F(127.0))


def variants(Xw):
    """name -> q of each wrong neighbour of the contract (module docstring)."""
    amax = np.abs(Xw).max(axis=1)
    a = np.maximum(amax, F(1e-5)).astype(F)[:, None]
    inv, deq = (F(127.0) / a).astype(F), (a / F(127.0)).astype(F)
    t = (Xw * inv).astype(F)
    x64, a64 = Xw.astype(np.float64), a.astype(np.float64)
    out = {
        "x / deq": np.rint((Xw / deq).astype(F)),
        "(x / a) * 127": np.rint(((Xw / a).astype(F) * F(127.0)).astype(F)),
        "(x * 127) / a": np.rint(((Xw * F(127.0)).astype(F) / a).astype(F)),
        "inv = 127 * (1 / a)": np.rint((Xw * (F(127.0) * (F(1.0) / a).astype(F)).astype(F)).astype(F)),
        "float64": np.rint(x64 * 127.0 / a64).astype(F),
        "half away": (np.sign(t) * np.floor(np.abs(t) + F(0.5))).astype(F),
    }
    return {k: _clamp(v.astype(F)).astype(np.int8) for k, v in out.items()}


def _rows_plan(M):
    """(near-tie rows, exact-tie rows, zero row?, row below the eps?) of an M-row X."""
    ties = 4 if M >= 32 else 2 if M >= 16 else 1 if M >= 4 else 0
    extra = 2 if M >= 16 else 0
    return M - ties - extra, ties, extra == 2


def _build_x(M, K, seed):
    """The fp32 X of the module docstring: (X, a[m] signed as placed, the
    exact-tie rows' indices)."""
    rng = np.random.default_rng(seed)
    near, ties, extra = _rows_plan(M)
    X = np.zeros((M, K), F)
    a = np.zeros(M, F)
    tie_rows = list(range(near, near + ties))
    for m in range(M):
        if extra and m == M - 2:
            continue  # the all-zero row
        j = rng.integers(-126, 126, size=K).astype(F)
        if m in tie_rows:
            am = F(127.0) / F(8.0)
            row = ((j + F(0.5)) / F(8.0)).astype(F)  # exact
        else:
            am = F(3e-6) if (extra and m == M - 1) else (F(3.0) * F(rng.uniform(0.5, 2.0))).astype(F)
            row = ((j.astype(np.float64) + 0.5) * np.float64(am) / 127.0).astype(F)
            row = (row.view(np.int32) + rng.integers(-2, 3, size=K).astype(np.int32)).view(F)
        k = 0 if m == 0 else K - 1 if m == 1 else (37 * m) % K
        row[k] = -am if m % 2 else am
        X[m], a[m] = row, row[k]
    return X, a, tie_rows


@functools.lru_cache(maxsize=None)
def _xq(M, K, xdtype):
    """X in its type (CPU tensor), its widened copy, the contract's (q, deq),
    the exact-tie rows; the input conditions are asserted here."""
    import torch
    import tspgemm as T
    # the first seed whose X tells every variant apart as the docstring asks
    # (a variant can agree with the contract on a whole row, by its a[m]: that
    # decides a one-row X; a 16-bit X keeps only a few near-ties)
    for seed in range(1000 * M + K, 1000 * M + K + 64):
        X, a, tie_rows = _build_x(M, K, seed)
        Xt = torch.from_numpy(X) if xdtype == "float32" else torch.from_numpy(X).to(_tdtype(xdtype))
        Xw = Xt.to(torch.float32).numpy()
        q, deq = T.act_quant_ref(Xw)
        diff = {k: (v != q) for k, v in variants(Xw).items()}
        if all(d.mean() >= 0.03 if xdtype == "float32" else d.any() for d in diff.values()):
            break
    assert np.isfinite(Xw).all()
    a_t = a if xdtype == "float32" else torch.from_numpy(a).to(_tdtype(xdtype)).to(torch.float32).numpy()
    assert np.array_equal(np.abs(Xw).max(axis=1), np.abs(a_t)), "a row's maximum is not a[m]"
    rows = np.arange(M)
    placed = np.where(rows == 0, 0, np.where(rows == 1, K - 1, (37 * rows) % K))
    assert np.array_equal(Xw[rows, placed], a_t)
    for name, d in diff.items():
        if xdtype == "float32":
            assert d.mean() >= 0.03, (name, "differs from the contract in only", float(d.mean()), (M, K))
        else:
            assert d.any(), (name, "is not told apart on this X", (M, K, xdtype))
    if tie_rows:
        share = float(diff["half away"][tie_rows].mean())
        assert share >= 0.30, ("half away on the exact-tie rows", share, (M, K, xdtype))
    near, ties, extra = _rows_plan(M)
    if extra:
        assert not q[M - 2].any() and deq[M - 2] == F(1e-5) / F(127.0)
        assert deq[M - 1] == F(1e-5) / F(127.0) and 0 < np.abs(q[M - 1]).max() < 127
    assert np.abs(q).max() == 127 and deq.dtype == F and q.dtype == np.int8
    for arr in (Xw, q, deq):
        arr.setflags(write=False)
    return Xt, Xw, q, deq, tuple(tie_rows)


@functools.lru_cache(maxsize=None)
def _weights(M, K, N, B=0):
    """W as test_gpu_scaled draws it: (arrays, chain(Xw) with a zero b)."""
    import oracle as O
    W = O.gen_ternary(K, N, 4, 1000 * M + K + N)
    zeros = np.zeros(N, F)
    if B:
        arrays = O.blocked_tcsc_encode(W, B)
        return arrays, lambda Xw: O.base_blocked_tcsc(Xw, arrays, zeros, K, N, B)
    t = O.tcsc_encode(W)
    return t.arrays, lambda Xw: O.base_tcsc(Xw, t, zeros)


def expected_bits(run, Xw, b, alpha, cs, ydtype):
    """want[(with col_scale?, 'plain' | 'prelu')] = the bits of the Y type, and deq."""
    import tspgemm as T
    q, deq = T.act_quant_ref(Xw)
    chain = run(q.astype(F))
    assert np.isfinite(chain).all() and not np.signbit(chain[chain == 0]).any()
    want = {}
    for c in (cs, None):
        for key, al in (("plain", None), ("prelu", alpha)):
            y = expect32(chain, deq, c, b, al)
            assert np.isfinite(y).all(), (c is not None, key, "expected array is not finite")
            if ydtype != "float32":
                assert float(np.abs(y).max()) <= YMAX[ydtype], (key, "expected array overflows the Y type")
            wb = _ybits_of(y, ydtype)
            wb.setflags(write=False)
            want[(c is not None, key)] = wb
    return want, deq


@functools.lru_cache(maxsize=None)
def _acase(M, K, N, xdtype="float32", ydtype="float32", B=0):
    """One shape's inputs and expectations, computed once, never modified:
    (arrays, Xt, Xw, b, alpha, cs, deq, want)."""
    Xt, Xw, q, deq, tie_rows = _xq(M, K, xdtype)
    arrays, run = _weights(M, K, N, B)
    b = np.linspace(-3, 3, N).astype(F)
    alpha = np.linspace(-0.5, 0.5, N).astype(F)
    cs = _draw_scales(M, N, 0, 7 * M + N)[1]
    want, deq2 = expected_bits(run, Xw, b, alpha, cs, ydtype)
    assert np.array_equal(deq2.view(np.uint32), deq.view(np.uint32))
    # the column scale and the PReLU both show in the expectation
    assert not np.array_equal(want[(True, "plain")], want[(False, "plain")])
    assert not np.array_equal(want[(True, "plain")], want[(True, "prelu")])
    for arr in (b, alpha, cs):
        arr.setflags(write=False)
    return arrays, Xt, Xw, b, alpha, cs, deq, want


# ---- the shared scheme -----------------------------------------------------------------

def _scale_out(M):
    """(buffer, slice [3, 3 + M)) for row_scale_out, the buffer sentinel-filled."""
    import torch
    rbuf = torch.empty(M + 11, device="cuda")
    rbuf.view(torch.int32).fill_(SENT)
    return rbuf, rbuf[3:3 + M]


def _assert_scale_out(rbuf, M, deq, what):
    import torch
    got = rbuf.view(torch.int32).cpu().numpy().view(np.uint32)
    assert np.array_equal(got[3:3 + M], deq.view(np.uint32)), (what, "row_scale_out != deq")
    assert (got[:3] == SENT).all() and (got[3 + M:] == SENT).all(), (what, "row_scale_out was written outside [0, M)")


def check_actquant(h, case, ydtype, what, prelu=True, Xd=None):
    import torch
    arrays, Xt, Xw, b, alpha, cs, deq, want = case
    M, N = Xt.shape[0], b.shape[0]
    Xd = Xt.cuda() if Xd is None else Xd
    bd, ad, cd = _dev(b), _dev(alpha), _dev(cs)
    keep = [t.clone() for t in (Xd, bd, ad, cd)]
    outs = _outputs(M, N, ydtype)
    for c in (cd, None):
        for key, al in (("plain", None), ("prelu", ad)):
            if key == "prelu" and not prelu:
                continue
            wb = want[(c is not None, key)]
            for name, (buf, view, box, fill, only) in outs.items():
                tag = (what, ydtype, "cs" if c is not None else "no cs", key, name)
                fill(buf)
                rbuf, rd = _scale_out(M)
                out = h.gemm_torch_actquant(Xd, bd, view, alpha=al, col_scale=c, row_scale_out=rd)
                torch.cuda.synchronize()
                assert out is view
                got = _got_bits(view, ydtype)
                assert np.array_equal(got, wb), (tag, int((got != wb).sum()), "of", wb.size, "elements differ",
                                                 np.argwhere(got != wb)[:6].tolist())
                only(buf, *box, tag)
                _assert_scale_out(rbuf, M, deq, tag)
    for t, k, n in zip((Xd, bd, ad, cd), keep, ("X", "b", "alpha", "col_scale")):
        assert torch.equal(t.view(torch.int8), k.view(torch.int8)), (what, n, "was written")


# ---- every kernel family -----------------------------------------------------------------

@pytest.mark.parametrize("M,K,N,mode,kernel", [(1, 193, 301, 0, "tsg_tcsc_ell_pc_kernel"),
                                               (4, 193, 301, 3, "tsg_tcsc_ell_kernel"),
                                               (16, 193, 301, 0, "tsg_tcsc_ell_kernel")])
def test_actquant_small_m_walks(tsg, M, K, N, mode, kernel):
    """The producer/consumer walk and the ELL walk: they run on the int8 q the
    row pass wrote."""
    case = _acase(M, K, N)
    h = tsg.TCSCDevice(*case[0], K, N)
    h.set_small_m(mode)
    assert h.call_kernel(M) == kernel and h.call_tile_rows(M) == 0
    check_actquant(h, case, "float32", (kernel, M, K, N))
    h.close()


@pytest.mark.parametrize("width,M,K,N", [(128, 63, 193, 700), (16, 65, 388, 700), (8, 130, 193, 301)])
def test_actquant_rows64_widths(tsg, width, M, K, N):
    """The 64-row image at widths 128, 16 and 8 (8 waves); K = 388 stages by quads."""
    case = _acase(M, K, N)
    h = _jit_handle(tsg, case[0], K, N, 64, width)
    assert h.call_kernel(M) == "tsg_jit64_kernel" and h.jit_width(M) == width and h.jit_waves(M) == 8
    check_actquant(h, case, "float32", ("rows64", width, M, K, N))
    h.close()


@pytest.mark.parametrize("M,K,N", [(65, 193, 700), (65, 1030, 301)])
def test_actquant_rows64_four_wave_shape_and_long_k(tsg, M, K, N):
    """The 64-row image's automatic 4-wave shape; K = 1030: several iterations
    of the row pass per lane, scalar loads, a tail."""
    case = _acase(M, K, N)
    h = _jit_handle(tsg, case[0], K, N, 64, 0)
    assert h.call_kernel(M) == "tsg_jit64_kernel"
    if K == 193:
        assert h.jit_waves(M) == 4, (h.jit_width(M), h.jit_waves(M))
    check_actquant(h, case, "float32", ("rows64 auto", M, K, N))
    h.close()


@pytest.mark.parametrize("width", [64, 0])
def test_actquant_rows128(tsg, width):
    M, K, N = 130, 388, 700
    case = _acase(M, K, N)
    h = _jit_handle(tsg, case[0], K, N, 128, width)
    assert h.call_kernel(M) == "tsg_jit_kernel" and h.call_tile_rows(M) == 128
    if width:
        assert h.jit_width(M) == width and h.jit_waves(M) == 8
    else:
        assert h.jit_waves(M) == 4, (h.jit_width(M), h.jit_waves(M))
    check_actquant(h, case, "float32", ("rows128", width, M, K, N))
    h.close()


def test_actquant_rx_kernel(tsg, monkeypatch):
    M, K, N = 130, 193, 301
    monkeypatch.setenv("TSG_KERNEL", "rx")
    case = _acase(M, K, N)
    h = tsg.TCSCDevice(*case[0], K, N)
    h.set_small_m(1)
    assert h.kernel_name() == "tsg_tcsc_rx_kernel" and h.call_kernel(M) == "tsg_tcsc_rx_kernel"
    check_actquant(h, case, "float32", ("rx", M, K, N))
    h.close()


def test_actquant_blocked_handle(tsg):
    """A blocked handle (the plain call only: the oracle has no blocked PReLU)."""
    M, K, N, B = 130, 385, 700, 64
    case = _acase(M, K, N, B=B)
    h = tsg.TCSCDevice.from_blocked(*case[0], K, N, B)
    h.set_small_m(1)
    assert h.call_kernel(M) == "tsg_jit_kernel"
    check_actquant(h, case, "float32", ("blocked", M, K, N, B), prelu=False)
    h.close()


# ---- types -------------------------------------------------------------------------------

def _type_handle(tsg, arrays, family, M, K, N):
    if family == "walk":
        h = tsg.TCSCDevice(*arrays, K, N)
        assert h.call_kernel(M) == "tsg_tcsc_ell_kernel"
    else:
        h = _jit_handle(tsg, arrays, K, N, 64, 16)
        assert h.call_kernel(M) == "tsg_jit64_kernel" and h.jit_width(M) == 16
    return h


@pytest.mark.parametrize("ydtype", YDTYPES)
@pytest.mark.parametrize("xdtype", XDTYPES)
@pytest.mark.parametrize("family", ["walk", "rows64"])
def test_actquant_full_type_product(tsg, xdtype, ydtype, family):
    M, K, N = TYPE_SHAPES[0] if family == "walk" else TYPE_SHAPES[1]
    case = _acase(M, K, N, xdtype, ydtype)
    h = _type_handle(tsg, case[0], family, M, K, N)
    check_actquant(h, case, ydtype, ("product", family, M, K, N, xdtype))
    h.close()


@pytest.mark.parametrize("xdtype", XDTYPES)
@pytest.mark.parametrize("family", ["walk", "rows64"])
def test_actquant_misaligned_x(tsg, xdtype, family):
    """X one element into a larger buffer: not aligned to 4 elements, so the
    row pass and the staging pass take their scalar loads (K = 388 would
    otherwise go by quads)."""
    M, K, N = TYPE_SHAPES[1] if family == "rows64" else (16, 388, 301)
    case = _acase(M, K, N, xdtype, "float32")
    h = _type_handle(tsg, case[0], family, M, K, N)
    Xd = _x_on_device(case[1], 1)
    assert Xd.data_ptr() % (4 * Xd.element_size()) != 0
    check_actquant(h, case, "float32", ("misaligned", family, M, K, N, xdtype), Xd=Xd)
    h.close()


# ---- equivalence ---------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["walk", "rows64"])
def test_actquant_equals_the_scaled_call_on_q(tsg, family):
    """The call is gemm_torch_scaled(q as int8, row_scale = deq) on the same
    handle, bit for bit, q and deq the contract's."""
    import torch
    M, K, N = TYPE_SHAPES[0] if family == "walk" else TYPE_SHAPES[1]
    arrays, Xt, Xw, b, alpha, cs, deq, want = _acase(M, K, N)
    q = _xq(M, K, "float32")[2]
    h = _type_handle(tsg, arrays, family, M, K, N)
    Xd, bd, ad, cd = Xt.cuda(), _dev(b), _dev(alpha), _dev(cs)
    qd, dd = torch.from_numpy(np.array(q)).cuda(), _dev(deq)
    for al in (None, ad):
        for c in (None, cd):
            Ys = h.gemm_torch_scaled(qd, bd, alpha=al, row_scale=dd, col_scale=c)
            Ya = h.gemm_torch_actquant(Xd, bd, alpha=al, col_scale=c)
            torch.cuda.synchronize()
            assert torch.equal(Ys.view(torch.int32), Ya.view(torch.int32)), (family, al is not None, c is not None)
    h.close()


# ---- isolation ------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["walk", "rows64", "rows128"])
def test_actquant_nan_and_inf_rows_stay_in_their_row(tsg, family):
    """One row all NaN, then one row with an inf: every other row of Y and every
    other deq entry is what it is without them, and the call does not fault."""
    import torch
    M, K, N = {"walk": TYPE_SHAPES[0], "rows64": TYPE_SHAPES[1], "rows128": (130, 388, 700)}[family]
    arrays, Xt, Xw, b, alpha, cs, deq, want = _acase(M, K, N)
    h = _type_handle(tsg, arrays, family, M, K, N) if family != "rows128" else _jit_handle(tsg, arrays, K, N, 128, 64)
    bd, cd = _dev(b), _dev(cs)
    wb = want[(True, "plain")]
    for bad_row, value, whole in ((2, float("nan"), True), (M - 3, float("inf"), False), (0, float("-inf"), False)):
        X = Xt.clone()
        if whole:
            X[bad_row, :] = value
        else:
            X[bad_row, 5] = value
        others = np.arange(M) != bad_row
        rbuf, rd = _scale_out(M)
        Y = h.gemm_torch_actquant(X.cuda(), bd, col_scale=cd, row_scale_out=rd)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(Y)[others], wb[others]), (family, bad_row, value)
        got = rd.cpu().numpy()
        assert np.array_equal(got.view(np.uint32)[others], deq.view(np.uint32)[others]), (family, bad_row, value)
    h.close()


@pytest.mark.parametrize("family", ["walk", "rows64", "rows128"])
def test_actquant_scratch_of_an_earlier_call_is_not_reused(tsg, family):
    """A call with 1000 X right before the checked call (same handle, same
    stream, then another stream) changes nothing: inv, deq and q are this
    call's."""
    import torch
    M, K, N = {"walk": TYPE_SHAPES[0], "rows64": TYPE_SHAPES[1], "rows128": (130, 388, 700)}[family]
    arrays, Xt, Xw, b, alpha, cs, deq, want = _acase(M, K, N)
    h = _type_handle(tsg, arrays, family, M, K, N) if family != "rows128" else _jit_handle(tsg, arrays, K, N, 128, 64)
    Xd, bd, cd = Xt.cuda(), _dev(b), _dev(cs)
    Xbig = Xd * 1000.0
    wb = want[(True, "plain")]
    h.gemm_torch_actquant(Xbig, bd, col_scale=cd)
    rbuf, rd = _scale_out(M)
    Y = h.gemm_torch_actquant(Xd, bd, col_scale=cd, row_scale_out=rd)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Y), wb)
    _assert_scale_out(rbuf, M, deq, family)
    s = torch.cuda.Stream()
    h.gemm_torch_actquant(Xbig, bd, col_scale=cd)  # on the current stream, still running when ...
    with torch.cuda.stream(s):                     # ... the other stream's call is enqueued
        Xs, bs, cs_s = Xt.cuda(), _dev(b), _dev(cs)
        Y2 = h.gemm_torch_actquant(Xs, bs, col_scale=cs_s)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Y2), wb)
    h.close()


def test_actquant_zero_k_and_zero_rows(tsg):
    """K = 0: amax is 0, deq = 1e-5 / 127, Y = b; M = 0: nothing is written."""
    import torch
    N = 40
    z = np.zeros(N + 1, np.int32)
    h = tsg.TCSCDevice(z, z, np.zeros(0, np.int32), np.zeros(0, np.int32), 0, N)
    b = np.linspace(-3, 3, N).astype(F)
    for M in (3, 70):
        rbuf, rd = _scale_out(M)
        Y = h.gemm_torch_actquant(torch.empty((M, 0), device="cuda"), _dev(b), row_scale_out=rd)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(Y), np.broadcast_to(b, (M, N)).view(np.uint32))
        _assert_scale_out(rbuf, M, np.full(M, F(1e-5) / F(127.0), F), ("K = 0", M))
    h.close()
    M, K, N = TYPE_SHAPES[0]
    case = _acase(M, K, N)
    h = tsg.TCSCDevice(*case[0], K, N)
    rbuf, rd = _scale_out(4)
    Y = h.gemm_torch_actquant(torch.empty((0, K), device="cuda"), _dev(case[3]), row_scale_out=rd[:0])
    torch.cuda.synchronize()
    assert tuple(Y.shape) == (0, N) and bool((rbuf.view(torch.int32) == SENT).all())
    h.close()


# ---- errors ---------------------------------------------------------------------------------

def test_actquant_bad_arguments_are_refused(tsg):
    """An int8 X, a bad xtype, a bad ytype and ldY < N: TSG_ERR_ARG, nothing written."""
    import torch
    M, K, N = TYPE_SHAPES[0]
    arrays, Xt, Xw, b, alpha, cs, deq, want = _acase(M, K, N, "bfloat16", "bfloat16")
    h = tsg.TCSCDevice(*arrays, K, N)
    Xd, bd, ad, cd = Xt.cuda(), _dev(b), _dev(alpha), _dev(cs)
    X8 = torch.zeros((M, K), dtype=torch.int8, device="cuda")
    buf = torch.empty((M + 2, 2 * N), dtype=torch.bfloat16, device="cuda")
    _fill16(buf)
    rbuf, rd = _scale_out(M)
    args = dict(drow_scale_out=rd.data_ptr(), dcol_scale=cd.data_ptr())
    y = buf[1:].data_ptr()
    for dalpha in (None, ad.data_ptr()):
        with pytest.raises(tsg.TSGError, match="int8") as e:
            h.gemm_dev_actquant(X8.data_ptr(), tsg.TSG_X_I8, bd.data_ptr(), y, tsg.TSG_Y_BF16, M, 0, dalpha, **args)
        assert e.value.code == 1  # TSG_ERR_ARG
        for xtype in (4, -1):
            with pytest.raises(tsg.TSGError, match="is not a tsg_xtype") as e:
                h.gemm_dev_actquant(Xd.data_ptr(), xtype, bd.data_ptr(), y, tsg.TSG_Y_BF16, M, 0, dalpha, **args)
            assert e.value.code == 1
        for ytype in (3, -1):
            with pytest.raises(tsg.TSGError, match="is not a tsg_ytype") as e:
                h.gemm_dev_actquant(Xd.data_ptr(), tsg.TSG_X_BF16, bd.data_ptr(), y, ytype, M, 0, dalpha, **args)
            assert e.value.code == 1
        with pytest.raises(tsg.TSGError, match="is less than N") as e:
            h.gemm_dev_actquant(Xd.data_ptr(), tsg.TSG_X_BF16, bd.data_ptr(), y, tsg.TSG_Y_BF16, M, 0, dalpha,
                                ldY=N - 1, **args)
        assert e.value.code == 1
    with pytest.raises(tsg.TSGError, match="int8") as e:
        h.gemm_torch_actquant(X8, bd, out_dtype=torch.bfloat16)
    assert e.value.code == 1
    for bad in (rd.double(), rd[:M - 1], torch.ones(M), [0.0] * M, torch.ones(2 * M, device="cuda")[::2]):
        with pytest.raises(tsg.TSGError, match="row_scale_out"):
            h.gemm_torch_actquant(Xd, bd, out_dtype=torch.bfloat16, row_scale_out=bad)
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int16) == SENT16).all())
    assert bool((rbuf.view(torch.int32) == SENT).all())
    h.close()


# ---- graph capture -----------------------------------------------------------------------------

def test_actquant_graph_capture_after_reserve(tsg):
    """After reserve(M) a captured bf16-in, bf16-out call allocates nothing; a
    replay is right, and so is one after X was rewritten in place (the row
    pass runs again at every replay)."""
    import torch
    M, K, N = 65, 388, 700
    arrays, Xt, Xw, b, alpha, cs, deq, want = _acase(M, K, N, "bfloat16", "bfloat16")
    run = _weights(M, K, N)[1]
    Xw2 = (Xw[::-1] * F(0.5)).copy()  # (exact in bf16: another X with other row maxima per row)
    Xt2 = torch.from_numpy(Xw2).to(torch.bfloat16)
    assert np.array_equal(Xt2.to(torch.float32).numpy(), Xw2)
    want2, deq2 = expected_bits(run, Xw2, b, alpha, cs, "bfloat16")
    assert not np.array_equal(want2[(True, "plain")], want[(True, "plain")])
    h = tsg.TCSCDevice(*arrays, K, N)
    assert h.call_kernel(M) == "tsg_jit64_kernel"
    h.reserve(M)
    work = h.info()["work_bytes"]
    assert work > 0
    Xd, bd, cd = Xt.cuda(), _dev(b), _dev(cs)
    buf = torch.empty((M + 2, N + 3), dtype=torch.bfloat16, device="cuda")
    view = buf[1:M + 1, 1:N + 1]
    rbuf, rd = _scale_out(M)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # (no warm-up call: reserve alone must have prepared everything)
        h.gemm_torch_actquant(Xd, bd, view, col_scale=cd, row_scale_out=rd)
    assert h.info()["work_bytes"] == work
    from test_gpu_ytype import _assert_only_view_written16, _ybits
    for replay, (wb, dq) in enumerate(((want[(True, "plain")], deq), (want2[(True, "plain")], deq2))):
        if replay:
            Xd.copy_(Xt2.cuda())
        _fill16(buf)
        rbuf.view(torch.int32).fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_ybits(view), wb), replay
        _assert_only_view_written16(buf, 1, M + 1, 1, N + 1, ("graph replay", replay))
        _assert_scale_out(rbuf, M, dq, ("graph replay", replay))
    h.close()


@pytest.mark.parametrize("family", ["walk", "rows64"])
def test_actquant_capture_without_reserve_fails_loudly(tsg, family):
    """The work buffer is large enough (a plain bf16 call at the larger M grew
    it) but the quantisation scratch was sized by a smaller call: a captured
    call at the larger M is refused with the reserve hint, the scratch does not
    grow (a second capture is refused too), and the handle still works."""
    import torch
    small, (M, K, N) = (2, TYPE_SHAPES[0]) if family == "walk" else (60, (130, 193, 301))
    arrays, Xt, Xw, b, alpha, cs, deq, want = _acase(M, K, N, "bfloat16", "float32")
    if family == "walk":
        h = tsg.TCSCDevice(*arrays, K, N)
        assert h.call_kernel(M) == "tsg_tcsc_ell_kernel"
    else:
        h = _jit_handle(tsg, arrays, K, N, 64, 8)
    Xd, bd, cd = Xt.cuda(), _dev(b), _dev(cs)
    h.gemm_torch_xy(Xd, bd)                      # the work buffer of M rows, the image of M rows
    h.gemm_torch_actquant(Xd[:small], bd)        # the scratch of `small` rows (<= 128: one allocation step)
    torch.cuda.synchronize()
    work = h.info()["work_bytes"]
    big = Xd if family == "walk" else torch.cat([Xd, Xd])  # (rows64: past the scratch's 128-row step)
    if family != "walk":
        h.gemm_torch_xy(big, bd)
        torch.cuda.synchronize()
        work = h.info()["work_bytes"]
    for attempt in range(2):
        g = torch.cuda.CUDAGraph()
        with pytest.raises(tsg.TSGError, match="call tcsc_hip_reserve") as e:
            with torch.cuda.graph(g):
                h.gemm_torch_actquant(big, bd, col_scale=cd)
        assert e.value.code == 1 and "activation-quantisation scratch" in str(e.value), attempt
        torch.cuda.synchronize()
    assert h.info()["work_bytes"] == work
    Y = h.gemm_torch_actquant(Xd, bd, col_scale=cd)  # the handle still works (and now grows the scratch)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Y), want[(True, "plain")])
    h.close()
