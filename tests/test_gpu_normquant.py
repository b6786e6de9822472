"""Fused RMSNorm + int8 activation quantisation on the device-pointer calls
(tcsc_hip_gemm_dev_normquant, TCSCDevice.gemm_torch_normquant) through every
kernel family on the GPU.

The contract (include/ternary_spgemm.h; tspgemm.rms_norm_ref states it in
numpy): all fp32 on the widened X, one rounding per operation, no fma,

    sq = x * x;  s[p] = sum of sq[p + 256 i], ascending, p = 0..255
    ss = the 256 partials by a balanced binary tree, neighbours first
    rn[m] = 1 / sqrt(ss / K + eps);  xn[m,k] = (x[m,k] * rn[m]) * gamma[k]
    Y, deq = the actquant call's on the fp32 X = xn

so the expected Y is test_gpu_actquant.expected_bits on xn.  Everything is
compared as integers.

Inputs (the case builder, _ncase, asserts all of this on the CPU; the CPU file
test_normquant_ref.py runs it for every shape used here).  A Gaussian X proves
little: a wrong sum shape changes deq in a minority of rows and a wrong
multiplication order changes no q at all.  So the rows are near-ties in
normalised space.  gamma[k] is U[0.5, 1.5); an ordinary row m draws j[k] uniform
in -126..125, w[k] = (j[k] + 0.5) / gamma[k] and, at k = (37 m) % K, +-127 /
gamma[k]; then u = w / sqrt(mean(w^2)) and x = fp32(u * c), c = 3 * U[0.5, 2):
RMSNorm is scale invariant, xn * inv lands within a few ulps of j + 0.5, and the
fp32 rounding of x supplies the scatter.

Element-level variants -- a staging pass that evaluates (x * g) * rn, x * (rn *
g), (x * (rn * inv)) * g, (x * rn) * (g * inv), float64 arithmetic, or rounds
half away -- are judged on q: each differs from the contract's q in at least
5 % of the elements of every fp32 case (measured: 11-26 %).

Row-level variants -- a serial sum, 64 partials, the tree from the high bit
down, a float64 sum, fma in the accumulation, ss * (1 / K), rn rounded from
float64 -- are judged on deq's bits.  Each is told apart by 12-15 % of candidate
rows (serial 57-97 %, rn 25 %, fma 3-5 %), so the rows are picked from a pool of
4096 candidates per case: every case with M >= 4 holds at least one row that
tells each tellable variant apart, and the single row of the M = 1 case tells
all of them apart at once.  fma cannot be told for K <= 256 (every partial
holds one element) nor on a 16-bit X (its squares are exact in fp32):
row_variant_names says which variants a case can tell.

A 16-bit X is the fp32 X cast to the type.  It meets the row-level conditions;
the element-level ones are carried by the fp32 cases, because the code after
the widening is the same template.

From M = 16 on, row M - 2 is all zero (rn = 1 / sqrt(eps), q = 0, Y = b) and row
M - 1 is tiny -- |x| <= 1e-9, so ms is far below eps, rn <= 1 / sqrt(eps) and the
maximum after the norm is below 1e-5: deq == 1e-5f / 127.

Each family case asserts the kernel that ran, then runs the plain and the PReLU
call with and without the column scale into a dense output and into the
odd-stride sentinel view, row_scale_out the slice [3, 3 + M) of a sentinel
buffer; X, gamma, b, alpha and the column scale are unchanged afterwards."""
import functools

import numpy as np
import pytest

import test_gpu_actquant as A
from test_gpu_actquant import FAMILY_SHAPES, TYPE_SHAPES, XDTYPES, YDTYPES
from test_gpu_ldy import SENT, _bits, _dev, _jit_handle
from test_gpu_scaled import _draw_scales, _got_bits, _outputs
from test_gpu_xtype import _tdtype, _x_on_device
from test_gpu_ytype import SENT16, _fill16

pytestmark = pytest.mark.gpu

F = np.float32
EPS = 1e-5
POOL = 4096
DEQ_FLOOR = F(1e-5) / F(127.0)


@pytest.fixture(autouse=True)
def _oracle_built(oracle_mod):
    """The cached cases below import the oracle themselves: it is built first."""


# ---- the wrong neighbours of the contract ---------------------------------------------

def _tree(s, high_first=False):
    while s.shape[1] > 1:
        h = s.shape[1] // 2
        s = (s[:, :h] + s[:, h:]).astype(F) if high_first else (s[:, 0::2] + s[:, 1::2]).astype(F)
    return s[:, 0]


def _partials(sq, n):
    M, K = sq.shape
    s = np.zeros((M, n), sq.dtype)
    for k0 in range(0, K, n):
        w = min(n, K - k0)
        s[:, :w] = (s[:, :w] + sq[:, k0:k0 + w]).astype(sq.dtype)
    return s


def _rn_of(ss, K, eps):
    ms = (ss / F(K)).astype(F)
    return (F(1.0) / np.sqrt((ms + F(eps)).astype(F)).astype(F)).astype(F)


def _deq_of(Xw, rn, g):
    xn = ((Xw * rn[:, None]).astype(F) * g[None, :]).astype(F)
    a = np.maximum(np.abs(xn).max(axis=1), F(1e-5)).astype(F)
    return (a / F(127.0)).astype(F)


def row_variant_names(K, xdtype):
    """The row-level variants an X of this K and type can tell from the contract."""
    names = ["serial sum", "64 partials", "high bit first", "float64 sum", "ss * (1 / K)", "rn from float64"]
    if K > 256 and xdtype == "float32":
        names.append("fma")  # K <= 256: one element per partial; 16-bit X: exact squares
    return names


def row_variants(Xw, g, eps):
    """name -> deq of each wrong way to make rn (module docstring)."""
    M, K = Xw.shape
    sq = (Xw * Xw).astype(F)
    x64 = Xw.astype(np.float64)
    s256 = _partials(sq, 256)
    ss = _tree(s256)
    # fma: round(x * x + s) once; x * x is exact in float64
    sf = np.zeros((M, 256), F)
    for k0 in range(0, K, 256):
        w = min(256, K - k0)
        sf[:, :w] = (sf[:, :w].astype(np.float64) + x64[:, k0:k0 + w] * x64[:, k0:k0 + w]).astype(F)
    ms = (ss / F(K)).astype(F)
    rns = {
        "serial sum": _rn_of(np.cumsum(sq, axis=1, dtype=F)[:, -1], K, eps),
        "64 partials": _rn_of(_tree(_partials(sq, 64)), K, eps),
        "high bit first": _rn_of(_tree(s256, high_first=True), K, eps),
        "float64 sum": _rn_of((x64 * x64).sum(axis=1).astype(F), K, eps),
        "fma": _rn_of(_tree(sf), K, eps),
        "ss * (1 / K)": (F(1.0) / np.sqrt(((ss * (F(1.0) / F(K))).astype(F) + F(eps)).astype(F)).astype(F)).astype(F),
        "rn from float64": (1.0 / np.sqrt(ms.astype(np.float64) + np.float64(F(eps)))).astype(F),
    }
    return {k: _deq_of(Xw, v, g) for k, v in rns.items()}


def elem_variants(Xw, g, eps):
    """name -> q of each wrong way to make q from the contract's rn and inv."""
    import tspgemm as T
    xn, rn = T.rms_norm_ref(Xw, g, eps)
    a = np.maximum(np.abs(xn).max(axis=1), F(1e-5)).astype(F)
    inv = (F(127.0) / a).astype(F)[:, None]
    r, gg = rn[:, None], g[None, :]
    t = (xn * inv).astype(F)
    out = {
        "(x * g) * rn": ((Xw * gg).astype(F) * r).astype(F) * inv,
        "x * (rn * g)": (Xw * (r * gg).astype(F)).astype(F) * inv,
        "(x * (rn * inv)) * g": (Xw * (r * inv).astype(F)).astype(F) * gg,
        "(x * rn) * (g * inv)": (Xw * r).astype(F) * (gg * inv).astype(F),
        "float64": Xw.astype(np.float64) * r.astype(np.float64) * gg.astype(np.float64) * inv.astype(np.float64),
    }
    out = {k: np.rint(v.astype(F)) for k, v in out.items()}
    out["half away"] = (np.sign(t) * np.floor(np.abs(t) + F(0.5))).astype(F)
    return {k: A._clamp(v.astype(F)).astype(np.int8) for k, v in out.items()}


# ---- the case builder ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gamma(K):
    g = np.random.default_rng(7000 + K).uniform(0.5, 1.5, size=K).astype(F)
    g.setflags(write=False)
    return g


def _rows_plan(M):
    """(ordinary rows, zero row and tiny row?) of an M-row X."""
    extra = M >= 16
    return M - (2 if extra else 0), extra


@functools.lru_cache(maxsize=4)
def _pool(M, K, seed):
    """POOL candidate rows (fp32) by the recipe of the module docstring;
    candidate i is made for row i % (ordinary rows of M)."""
    rng = np.random.default_rng(seed)
    g = _gamma(K).astype(np.float64)
    near, _ = _rows_plan(M)
    j = rng.integers(-126, 126, size=(POOL, K)).astype(np.float64)
    w = (j + 0.5) / g[None, :]
    i = np.arange(POOL)
    m = i % near
    k = (37 * m) % K
    w[i, k] = np.where(m % 2 == 1, -127.0, 127.0) / g[k]
    u = w / np.sqrt((w * w).mean(axis=1))[:, None]
    c = 3.0 * rng.uniform(0.5, 2.0, size=POOL)
    X = (u * c[:, None]).astype(F)
    X.setflags(write=False)
    return X


def _told(Xw, K, xdtype, g, eps):
    """[rows, tellable variants] -> whether the row's deq tells the variant apart."""
    import tspgemm as T
    xn, rn = T.rms_norm_ref(Xw, g, eps)
    deq = _deq_of_xn(xn)
    rv = row_variants(Xw, g, eps)
    return np.stack([rv[n].view(np.uint32) != deq.view(np.uint32) for n in row_variant_names(K, xdtype)], axis=1)


def _deq_of_xn(xn):
    a = np.maximum(np.abs(xn).max(axis=1), F(1e-5)).astype(F) if xn.shape[1] else np.full(xn.shape[0], F(1e-5), F)
    return (a / F(127.0)).astype(F)


def _cast(X, xdtype):
    """(X in its type as a CPU tensor, its widened fp32 copy)."""
    import torch
    Xt = torch.from_numpy(np.array(X))
    if xdtype != "float32":
        Xt = Xt.to(_tdtype(xdtype))
    return Xt, Xt.to(torch.float32).numpy()


@functools.lru_cache(maxsize=None)
def _xn(M, K, xdtype, eps=EPS):
    """X in its type (CPU tensor), its widened copy, gamma, the contract's xn;
    the input conditions are asserted here."""
    import tspgemm as T
    g = _gamma(K)
    near, extra = _rows_plan(M)
    names = row_variant_names(K, xdtype)
    chosen = None
    for seed in range(100 * M + K, 100 * M + K + 8):  # (the first pool does; more only if it ever does not)
        P = _pool(M, K, seed)
        told = _told(_cast(P, xdtype)[1], K, xdtype, g, eps)  # [POOL, variants]
        row_of = np.arange(POOL) % near
        chosen = {}
        if M == 1:
            hit = np.flatnonzero(told.all(axis=1))
            if hit.size:
                chosen[0] = int(hit[0])
        else:
            left = np.ones(len(names), bool)
            while left.any():
                free = ~np.isin(row_of, list(chosen))
                gain = (told & left[None, :]).sum(axis=1) * free
                best = int(gain.argmax())
                if gain[best] == 0:
                    break
                chosen[int(row_of[best])] = best
                left &= ~told[best]
            if left.any():
                chosen = None
        if chosen:
            break
    assert chosen, ("no pool of", POOL, "candidates tells every row-level variant apart", names, (M, K, xdtype))
    X = np.zeros((M, K), F)
    for m in range(near):
        X[m] = P[chosen.get(m, m)]
    if extra:  # row M - 2 stays zero; row M - 1 is tiny
        rng = np.random.default_rng(seed + 1)
        X[M - 1] = ((rng.integers(-126, 126, size=K) + 0.5) * (1e-9 / 127.0)).astype(F)
    Xt, Xw = _cast(X, xdtype)
    assert np.isfinite(Xw).all()
    xn, rn = T.rms_norm_ref(Xw, g, eps)
    q, deq = T.act_quant_ref(xn)
    # row-level: each tellable variant is told apart by a row (M = 1: by the one row, all at once)
    rv = row_variants(Xw, g, eps)
    shares = {n: float((rv[n].view(np.uint32) != deq.view(np.uint32))[:near].mean()) for n in names}
    for n in names:
        assert shares[n] > 0, (n, "is told apart by no row of this X", (M, K, xdtype), shares)
    # the maximum after the norm sits where the recipe put it
    if xdtype == "float32":
        rows = np.arange(near)
        assert np.array_equal(np.abs(xn[:near]).argmax(axis=1), (37 * rows) % K), "a row's maximum moved"
        ev = elem_variants(Xw, g, eps)
        eshares = {n: float((v != q).mean()) for n, v in ev.items()}
        for n, sh in eshares.items():
            assert sh >= 0.05, (n, "differs from the contract's q in only", sh, "of the elements", (M, K), eshares)
    if extra:
        assert not q[M - 2].any() and deq[M - 2] == DEQ_FLOOR and rn[M - 2] == F(1.0) / np.sqrt(F(eps))
        assert deq[M - 1] == DEQ_FLOOR and np.abs(xn[M - 1]).max() < F(1e-5)
        if xdtype != "float16":  # (1e-9 is below fp16's smallest subnormal: the row is zero there)
            assert 0 < np.abs(q[M - 1]).max() < 127
    assert np.abs(q).max() == 127
    for arr in (Xw, xn):
        arr.setflags(write=False)
    return Xt, Xw, g, xn


@functools.lru_cache(maxsize=None)
def _ncase(M, K, N, xdtype="float32", ydtype="float32", B=0, eps=EPS, gamma=True):
    """One shape's inputs and expectations, computed once, never modified:
    (arrays, Xt, Xw, g or None, eps, b, alpha, cs, deq, want, xn)."""
    import tspgemm as T
    Xt, Xw, g, xn = _xn(M, K, xdtype, eps)
    if not gamma:
        g, xn = None, T.rms_norm_ref(Xw, None, eps)[0]
    arrays, run = A._weights(M, K, N, B)
    b = np.linspace(-3, 3, N).astype(F)
    alpha = np.linspace(-0.5, 0.5, N).astype(F)
    cs = _draw_scales(M, N, 0, 7 * M + N)[1]
    want, deq = A.expected_bits(run, xn, b, alpha, cs, ydtype)
    assert not np.array_equal(want[(True, "plain")], want[(False, "plain")])
    assert not np.array_equal(want[(True, "plain")], want[(True, "prelu")])
    for arr in (b, alpha, cs):
        arr.setflags(write=False)
    return arrays, Xt, Xw, g, eps, b, alpha, cs, deq, want, xn


# ---- the shared scheme ------------------------------------------------------------------------

def _gamma_dev(g, K, sliced=False):
    """gamma on the device: its own tensor, or the slice [3, 3 + K) of a NaN-filled
    buffer (4-byte aligned only).  Returns (buffer, tensor to pass)."""
    import torch
    if g is None:
        return None, None
    if not sliced:
        t = _dev(g)
        return t, t
    buf = torch.full((K + 9,), float("nan"), device="cuda")
    buf[3:3 + K] = torch.from_numpy(np.array(g)).cuda()
    return buf, buf[3:3 + K]


def check_normquant(h, case, ydtype, what, prelu=True, Xd=None, sliced_gamma=False):
    import torch
    arrays, Xt, Xw, g, eps, b, alpha, cs, deq, want, xn = case
    M, N, K = Xt.shape[0], b.shape[0], Xt.shape[1]
    Xd = Xt.cuda() if Xd is None else Xd
    bd, ad, cd = _dev(b), _dev(alpha), _dev(cs)
    gbuf, gd = _gamma_dev(g, K, sliced_gamma)
    named = [(Xd, "X"), (bd, "b"), (ad, "alpha"), (cd, "col_scale")] + ([(gbuf, "gamma")] if g is not None else [])
    keep = [t.clone() for t, _ in named]
    outs = _outputs(M, N, ydtype)
    for c in (cd, None):
        for key, al in (("plain", None), ("prelu", ad)):
            if key == "prelu" and not prelu:
                continue
            wb = want[(c is not None, key)]
            for name, (buf, view, box, fill, only) in outs.items():
                tag = (what, ydtype, "cs" if c is not None else "no cs", key, name)
                fill(buf)
                rbuf, rd = A._scale_out(M)
                out = h.gemm_torch_normquant(Xd, bd, gd, eps, view, alpha=al, col_scale=c, row_scale_out=rd)
                torch.cuda.synchronize()
                assert out is view
                got = _got_bits(view, ydtype)
                assert np.array_equal(got, wb), (tag, int((got != wb).sum()), "of", wb.size, "elements differ",
                                                 np.argwhere(got != wb)[:6].tolist())
                only(buf, *box, tag)
                A._assert_scale_out(rbuf, M, deq, tag)
    for (t, n), k in zip(named, keep):
        assert torch.equal(t.view(torch.int8), k.view(torch.int8)), (what, n, "was written")


# ---- every kernel family -------------------------------------------------------------------------

@pytest.mark.parametrize("M,K,N,mode,kernel", [(1, 193, 301, 0, "tsg_tcsc_ell_pc_kernel"),
                                               (4, 193, 301, 3, "tsg_tcsc_ell_kernel"),
                                               (16, 193, 301, 0, "tsg_tcsc_ell_kernel")])
def test_normquant_small_m_walks(tsg, M, K, N, mode, kernel):
    """The producer/consumer walk and the ELL walk: they run on the int8 q the
    row pass made from xn."""
    case = _ncase(M, K, N)
    h = tsg.TCSCDevice(*case[0], K, N)
    h.set_small_m(mode)
    assert h.call_kernel(M) == kernel and h.call_tile_rows(M) == 0
    check_normquant(h, case, "float32", (kernel, M, K, N))
    h.close()


@pytest.mark.parametrize("width,M,K,N", [(128, 63, 193, 700), (16, 65, 388, 700), (8, 130, 193, 301)])
def test_normquant_rows64_widths(tsg, width, M, K, N):
    """The 64-row image at widths 128, 16 and 8 (8 waves); K = 388 stages by quads."""
    case = _ncase(M, K, N)
    h = _jit_handle(tsg, case[0], K, N, 64, width)
    assert h.call_kernel(M) == "tsg_jit64_kernel" and h.jit_width(M) == width and h.jit_waves(M) == 8
    check_normquant(h, case, "float32", ("rows64", width, M, K, N))
    h.close()


@pytest.mark.parametrize("M,K,N", [(65, 193, 700), (65, 1030, 301)])
def test_normquant_rows64_four_wave_shape_and_long_k(tsg, M, K, N):
    """The 64-row image's automatic 4-wave shape; K = 1030: several iterations
    of the row pass per lane, scalar loads, a tail, and fma in the sum tellable."""
    case = _ncase(M, K, N)
    h = _jit_handle(tsg, case[0], K, N, 64, 0)
    assert h.call_kernel(M) == "tsg_jit64_kernel"
    if K == 193:
        assert h.jit_waves(M) == 4, (h.jit_width(M), h.jit_waves(M))
    check_normquant(h, case, "float32", ("rows64 auto", M, K, N))
    h.close()


@pytest.mark.parametrize("width", [64, 0])
def test_normquant_rows128(tsg, width):
    M, K, N = 130, 388, 700
    case = _ncase(M, K, N)
    h = _jit_handle(tsg, case[0], K, N, 128, width)
    assert h.call_kernel(M) == "tsg_jit_kernel" and h.call_tile_rows(M) == 128
    if width:
        assert h.jit_width(M) == width and h.jit_waves(M) == 8
    else:
        assert h.jit_waves(M) == 4, (h.jit_width(M), h.jit_waves(M))
    check_normquant(h, case, "float32", ("rows128", width, M, K, N))
    h.close()


def test_normquant_rx_kernel(tsg, monkeypatch):
    M, K, N = 130, 193, 301
    monkeypatch.setenv("TSG_KERNEL", "rx")
    case = _ncase(M, K, N)
    h = tsg.TCSCDevice(*case[0], K, N)
    h.set_small_m(1)
    assert h.kernel_name() == "tsg_tcsc_rx_kernel" and h.call_kernel(M) == "tsg_tcsc_rx_kernel"
    check_normquant(h, case, "float32", ("rx", M, K, N))
    h.close()


def test_normquant_blocked_handle(tsg):
    """A blocked handle (the plain call only: the oracle has no blocked PReLU)."""
    M, K, N, B = 130, 385, 700, 64
    case = _ncase(M, K, N, B=B)
    h = tsg.TCSCDevice.from_blocked(*case[0], K, N, B)
    h.set_small_m(1)
    assert h.call_kernel(M) == "tsg_jit_kernel"
    check_normquant(h, case, "float32", ("blocked", M, K, N, B), prelu=False)
    h.close()


# ---- types ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ydtype", YDTYPES)
@pytest.mark.parametrize("xdtype", XDTYPES)
@pytest.mark.parametrize("family", ["walk", "rows64"])
def test_normquant_full_type_product(tsg, xdtype, ydtype, family):
    M, K, N = TYPE_SHAPES[0] if family == "walk" else TYPE_SHAPES[1]
    case = _ncase(M, K, N, xdtype, ydtype)
    h = A._type_handle(tsg, case[0], family, M, K, N)
    check_normquant(h, case, ydtype, ("product", family, M, K, N, xdtype))
    h.close()


@pytest.mark.parametrize("xdtype", XDTYPES)
@pytest.mark.parametrize("family", ["walk", "rows64"])
def test_normquant_misaligned_x(tsg, xdtype, family):
    """X one element into a larger buffer: not aligned to 4 elements, so the
    row pass sums by its scalar load shape and the staging pass takes scalar
    loads (K = 388 goes by quads otherwise).  The bits are the aligned call's."""
    import torch
    M, K, N = TYPE_SHAPES[1] if family == "rows64" else (16, 388, 301)
    case = _ncase(M, K, N, xdtype, "float32")
    h = A._type_handle(tsg, case[0], family, M, K, N)
    Xd = _x_on_device(case[1], 1)
    assert Xd.data_ptr() % (4 * Xd.element_size()) != 0
    check_normquant(h, case, "float32", ("misaligned", family, M, K, N, xdtype), Xd=Xd)
    bd, gd = _dev(case[5]), _dev(case[3])
    Xa = case[1].cuda()
    assert Xa.data_ptr() % (4 * Xa.element_size()) == 0
    ra, rm = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    Ya = h.gemm_torch_normquant(Xa, bd, gd, case[4], row_scale_out=ra)
    Ym = h.gemm_torch_normquant(Xd, bd, gd, case[4], row_scale_out=rm)
    torch.cuda.synchronize()
    assert torch.equal(Ya.view(torch.int32), Ym.view(torch.int32)) and torch.equal(ra.view(torch.int32),
                                                                                   rm.view(torch.int32))
    h.close()


# ---- gamma and eps --------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["walk", "rows64"])
def test_normquant_without_gamma(tsg, family):
    """gamma None: the second multiply is not performed."""
    M, K, N = TYPE_SHAPES[0] if family == "walk" else TYPE_SHAPES[1]
    case = _ncase(M, K, N, gamma=False)
    assert case[3] is None and not np.array_equal(case[9][(True, "plain")], _ncase(M, K, N)[9][(True, "plain")])
    h = A._type_handle(tsg, case[0], family, M, K, N)
    check_normquant(h, case, "float32", ("no gamma", family, M, K, N))
    h.close()


@pytest.mark.parametrize("family,M,K,N", [("walk", 16, 193, 301), ("rows64", 65, 388, 700), ("rows64", 65, 193, 700)])
def test_normquant_gamma_is_a_slice_of_a_nan_buffer(tsg, family, M, K, N):
    """gamma at [3, 3 + K) of a NaN-filled buffer (aligned to 4 bytes only):
    nothing outside the slice reaches Y, and the buffer is unchanged."""
    case = _ncase(M, K, N)
    if family == "walk":
        h = A._type_handle(tsg, case[0], family, M, K, N)
    else:
        h = _jit_handle(tsg, case[0], K, N, 64, 16)
    check_normquant(h, case, "float32", ("gamma slice", family, M, K, N), sliced_gamma=True)
    h.close()


@pytest.mark.parametrize("family", ["walk", "rows64"])
def test_normquant_other_eps(tsg, family):
    """eps = 1e-6 (every other case runs 1e-5): the zero row's rn and the tiny
    row's q change with it."""
    M, K, N = TYPE_SHAPES[0] if family == "walk" else TYPE_SHAPES[1]
    case = _ncase(M, K, N, eps=1e-6)
    assert not np.array_equal(case[9][(True, "plain")], _ncase(M, K, N)[9][(True, "plain")])
    h = A._type_handle(tsg, case[0], family, M, K, N)
    check_normquant(h, case, "float32", ("eps 1e-6", family, M, K, N))
    h.close()


# ---- equivalence ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["walk", "rows64"])
def test_normquant_equals_the_actquant_call_on_xn(tsg, family):
    """The call is gemm_torch_actquant(xn as an fp32 tensor) on the same handle,
    bit for bit, xn the contract's."""
    import torch
    M, K, N = TYPE_SHAPES[0] if family == "walk" else TYPE_SHAPES[1]
    arrays, Xt, Xw, g, eps, b, alpha, cs, deq, want, xn = _ncase(M, K, N)
    h = A._type_handle(tsg, arrays, family, M, K, N)
    Xd, bd, ad, cd, gd = Xt.cuda(), _dev(b), _dev(alpha), _dev(cs), _dev(g)
    xnd = torch.from_numpy(np.array(xn)).cuda()
    for al in (None, ad):
        for c in (None, cd):
            ra, rn_ = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
            Ya = h.gemm_torch_actquant(xnd, bd, alpha=al, col_scale=c, row_scale_out=ra)
            Yn = h.gemm_torch_normquant(Xd, bd, gd, eps, alpha=al, col_scale=c, row_scale_out=rn_)
            torch.cuda.synchronize()
            assert torch.equal(Ya.view(torch.int32), Yn.view(torch.int32)), (family, al is not None, c is not None)
            assert torch.equal(ra.view(torch.int32), rn_.view(torch.int32))
    h.close()


# ---- isolation ------------------------------------------------------------------------------------------------

def _iso_handle(tsg, arrays, family, M, K, N):
    if family == "rows128":
        return _jit_handle(tsg, arrays, K, N, 128, 64)
    return A._type_handle(tsg, arrays, family, M, K, N)


_ISO_SHAPES = {"walk": TYPE_SHAPES[0], "rows64": TYPE_SHAPES[1], "rows128": (130, 388, 700)}


@pytest.mark.parametrize("family", ["walk", "rows64", "rows128"])
def test_normquant_nan_and_inf_rows_stay_in_their_row(tsg, family):
    """One row all NaN, one row with an inf, one row whose sum of squares
    overflows: every other row of Y and every other deq entry is what it is
    without them, and the call does not fault."""
    import torch
    M, K, N = _ISO_SHAPES[family]
    arrays, Xt, Xw, g, eps, b, alpha, cs, deq, want, xn = _ncase(M, K, N)
    h = _iso_handle(tsg, arrays, family, M, K, N)
    bd, cd, gd = _dev(b), _dev(cs), _dev(g)
    wb = want[(True, "plain")]
    for bad_row, value, whole in ((2, float("nan"), True), (M - 3, float("inf"), False), (0, float("-inf"), False),
                                  (1, 3e38, True)):
        X = Xt.clone()
        if whole:
            X[bad_row, :] = value
        else:
            X[bad_row, 5] = value
        others = np.arange(M) != bad_row
        rbuf, rd = A._scale_out(M)
        Y = h.gemm_torch_normquant(X.cuda(), bd, gd, eps, col_scale=cd, row_scale_out=rd)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(Y)[others], wb[others]), (family, bad_row, value)
        got = rd.cpu().numpy()
        assert np.array_equal(got.view(np.uint32)[others], deq.view(np.uint32)[others]), (family, bad_row, value)
    h.close()


@pytest.mark.parametrize("family", ["walk", "rows64", "rows128"])
def test_normquant_scratch_of_an_earlier_call_is_not_reused(tsg, family):
    """A call with 1000 X right before the checked call (same handle, same
    stream, then another stream) changes nothing: rn, inv, deq and q are this
    call's.  (1000 X has another rn, and the eps keeps xn from being equal.)"""
    import torch
    M, K, N = _ISO_SHAPES[family]
    arrays, Xt, Xw, g, eps, b, alpha, cs, deq, want, xn = _ncase(M, K, N)
    h = _iso_handle(tsg, arrays, family, M, K, N)
    Xd, bd, cd, gd = Xt.cuda(), _dev(b), _dev(cs), _dev(g)
    Xbig = Xd * 1000.0
    wb = want[(True, "plain")]
    h.gemm_torch_normquant(Xbig, bd, gd, eps, col_scale=cd)
    rbuf, rd = A._scale_out(M)
    Y = h.gemm_torch_normquant(Xd, bd, gd, eps, col_scale=cd, row_scale_out=rd)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Y), wb)
    A._assert_scale_out(rbuf, M, deq, family)
    s = torch.cuda.Stream()
    h.gemm_torch_normquant(Xbig, bd, gd, eps, col_scale=cd)  # on the current stream, still running when ...
    with torch.cuda.stream(s):                                # ... the other stream's call is enqueued
        Xs, bs, cs_s, gs = Xt.cuda(), _dev(b), _dev(cs), _dev(g)
        Y2 = h.gemm_torch_normquant(Xs, bs, gs, eps, col_scale=cs_s)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Y2), wb)
    h.close()


def test_normquant_zero_k_and_zero_rows(tsg):
    """K = 0: no sum and no division; deq = 1e-5 / 127, Y = b.  M = 0: nothing
    is written."""
    import torch
    N = 40
    z = np.zeros(N + 1, np.int32)
    h = tsg.TCSCDevice(z, z, np.zeros(0, np.int32), np.zeros(0, np.int32), 0, N)
    b = np.linspace(-3, 3, N).astype(F)
    for M in (3, 70):
        for gd in (None, torch.empty(0, device="cuda")):
            rbuf, rd = A._scale_out(M)
            Y = h.gemm_torch_normquant(torch.empty((M, 0), device="cuda"), _dev(b), gd, EPS, row_scale_out=rd)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(Y), np.broadcast_to(b, (M, N)).view(np.uint32))
            A._assert_scale_out(rbuf, M, np.full(M, DEQ_FLOOR, F), ("K = 0", M))
    h.close()
    M, K, N = TYPE_SHAPES[0]
    case = _ncase(M, K, N)
    h = tsg.TCSCDevice(*case[0], K, N)
    rbuf, rd = A._scale_out(4)
    Y = h.gemm_torch_normquant(torch.empty((0, K), device="cuda"), _dev(case[5]), _dev(case[3]), EPS,
                               row_scale_out=rd[:0])
    torch.cuda.synchronize()
    assert tuple(Y.shape) == (0, N) and bool((rbuf.view(torch.int32) == SENT).all())
    h.close()


# ---- errors -------------------------------------------------------------------------------------------------------

def test_normquant_bad_arguments_are_refused(tsg):
    """An int8 X, a bad xtype, a bad ytype, ldY < N, a bad eps: TSG_ERR_ARG,
    nothing written; the torch wrapper refuses a bad gamma."""
    import torch
    M, K, N = TYPE_SHAPES[0]
    arrays, Xt, Xw, g, eps, b, alpha, cs, deq, want, xn = _ncase(M, K, N, "bfloat16", "bfloat16")
    h = tsg.TCSCDevice(*arrays, K, N)
    Xd, bd, ad, cd, gd = Xt.cuda(), _dev(b), _dev(alpha), _dev(cs), _dev(g)
    X8 = torch.zeros((M, K), dtype=torch.int8, device="cuda")
    buf = torch.empty((M + 2, 2 * N), dtype=torch.bfloat16, device="cuda")
    _fill16(buf)
    rbuf, rd = A._scale_out(M)
    args = dict(drow_scale_out=rd.data_ptr(), dcol_scale=cd.data_ptr())
    y, gp, BF = buf[1:].data_ptr(), gd.data_ptr(), tsg.TSG_Y_BF16
    for dalpha in (None, ad.data_ptr()):
        with pytest.raises(tsg.TSGError, match="int8") as e:
            h.gemm_dev_normquant(X8.data_ptr(), tsg.TSG_X_I8, gp, eps, bd.data_ptr(), y, BF, M, 0, dalpha, **args)
        assert e.value.code == 1  # TSG_ERR_ARG
        for xtype in (4, -1):
            with pytest.raises(tsg.TSGError, match="is not a tsg_xtype") as e:
                h.gemm_dev_normquant(Xd.data_ptr(), xtype, gp, eps, bd.data_ptr(), y, BF, M, 0, dalpha, **args)
            assert e.value.code == 1
        for ytype in (3, -1):
            with pytest.raises(tsg.TSGError, match="is not a tsg_ytype") as e:
                h.gemm_dev_normquant(Xd.data_ptr(), tsg.TSG_X_BF16, gp, eps, bd.data_ptr(), y, ytype, M, 0, dalpha,
                                     **args)
            assert e.value.code == 1
        with pytest.raises(tsg.TSGError, match="is less than N") as e:
            h.gemm_dev_normquant(Xd.data_ptr(), tsg.TSG_X_BF16, gp, eps, bd.data_ptr(), y, BF, M, 0, dalpha,
                                 ldY=N - 1, **args)
        assert e.value.code == 1
        for bad_eps in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(tsg.TSGError, match="eps") as e:
                h.gemm_dev_normquant(Xd.data_ptr(), tsg.TSG_X_BF16, gp, bad_eps, bd.data_ptr(), y, BF, M, 0, dalpha,
                                     **args)
            assert e.value.code == 1
    for bad_eps in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(tsg.TSGError, match="eps"):
            h.gemm_torch_normquant(Xd, bd, gd, bad_eps, buf[1:M + 1, :N], col_scale=cd, row_scale_out=rd)
    with pytest.raises(tsg.TSGError, match="int8") as e:
        h.gemm_torch_normquant(X8, bd, gd, eps, out_dtype=torch.bfloat16)
    assert e.value.code == 1
    for bad in (gd.double(), gd[:K - 1], torch.ones(K), [1.0] * K, torch.ones(2 * K, device="cuda")[::2],
                gd.reshape(1, K)):
        with pytest.raises(tsg.TSGError, match="gamma"):
            h.gemm_torch_normquant(Xd, bd, bad, eps, buf[1:M + 1, :N], row_scale_out=rd)
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int16) == SENT16).all())
    assert bool((rbuf.view(torch.int32) == SENT).all())
    h.close()


# ---- graph capture ---------------------------------------------------------------------------------------------------

def test_normquant_graph_capture_after_reserve(tsg):
    """After reserve(M) a captured bf16-in, bf16-out call allocates nothing; a
    replay is right, and so is one after X was rewritten in place (the row
    pass runs again at every replay)."""
    import torch
    from test_gpu_ytype import _assert_only_view_written16, _ybits
    M, K, N = 65, 388, 700
    arrays, Xt, Xw, g, eps, b, alpha, cs, deq, want, xn = _ncase(M, K, N, "bfloat16", "bfloat16")
    run = A._weights(M, K, N)[1]
    # another X, exact in bf16: the rows in reverse order with every other element halved
    Xw2 = Xw[::-1].copy()
    Xw2[:, ::2] *= F(0.5)
    Xt2 = torch.from_numpy(Xw2).to(torch.bfloat16)
    assert np.array_equal(Xt2.to(torch.float32).numpy(), Xw2)
    want2, deq2 = A.expected_bits(run, tsg.rms_norm_ref(Xw2, g, eps)[0], b, alpha, cs, "bfloat16")
    assert not np.array_equal(want2[(True, "plain")], want[(True, "plain")])
    h = tsg.TCSCDevice(*arrays, K, N)
    assert h.call_kernel(M) == "tsg_jit64_kernel"
    h.reserve(M)
    work = h.info()["work_bytes"]
    assert work > 0
    Xd, bd, cd, gd = Xt.cuda(), _dev(b), _dev(cs), _dev(g)
    buf = torch.empty((M + 2, N + 3), dtype=torch.bfloat16, device="cuda")
    view = buf[1:M + 1, 1:N + 1]
    rbuf, rd = A._scale_out(M)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):  # (no warm-up call: reserve alone must have prepared everything)
        h.gemm_torch_normquant(Xd, bd, gd, eps, view, col_scale=cd, row_scale_out=rd)
    assert h.info()["work_bytes"] == work
    for replay, (wb, dq) in enumerate(((want[(True, "plain")], deq), (want2[(True, "plain")], deq2))):
        if replay:
            Xd.copy_(Xt2.cuda())
        _fill16(buf)
        rbuf.view(torch.int32).fill_(SENT)
        gr.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_ybits(view), wb), replay
        _assert_only_view_written16(buf, 1, M + 1, 1, N + 1, ("graph replay", replay))
        A._assert_scale_out(rbuf, M, dq, ("graph replay", replay))
    h.close()


@pytest.mark.parametrize("family", ["walk", "rows64"])
def test_normquant_capture_without_reserve_fails_loudly(tsg, family):
    """The work buffer is large enough but the scratch was sized by a smaller
    call: a captured call at the larger M is refused with the reserve hint, the
    scratch does not grow (a second capture is refused too), and the handle
    still works."""
    import torch
    small, (M, K, N) = (2, TYPE_SHAPES[0]) if family == "walk" else (60, (130, 193, 301))
    arrays, Xt, Xw, g, eps, b, alpha, cs, deq, want, xn = _ncase(M, K, N, "bfloat16", "float32")
    if family == "walk":
        h = tsg.TCSCDevice(*arrays, K, N)
        assert h.call_kernel(M) == "tsg_tcsc_ell_kernel"
    else:
        h = _jit_handle(tsg, arrays, K, N, 64, 8)
    Xd, bd, cd, gd = Xt.cuda(), _dev(b), _dev(cs), _dev(g)
    h.gemm_torch_xy(Xd, bd)                              # the work buffer of M rows, the image of M rows
    h.gemm_torch_normquant(Xd[:small], bd, gd, eps)      # the scratch of `small` rows (<= 128: one allocation step)
    torch.cuda.synchronize()
    work = h.info()["work_bytes"]
    big = Xd if family == "walk" else torch.cat([Xd, Xd])  # (rows64: past the scratch's 128-row step)
    if family != "walk":
        h.gemm_torch_xy(big, bd)
        torch.cuda.synchronize()
        work = h.info()["work_bytes"]
    for attempt in range(2):
        gr = torch.cuda.CUDAGraph()
        with pytest.raises(tsg.TSGError, match="call tcsc_hip_reserve") as e:
            with torch.cuda.graph(gr):
                h.gemm_torch_normquant(big, bd, gd, eps, col_scale=cd)
        assert e.value.code == 1 and "activation-quantisation scratch" in str(e.value), attempt
        torch.cuda.synchronize()
    assert h.info()["work_bytes"] == work
    Y = h.gemm_torch_normquant(Xd, bd, gd, eps, col_scale=cd)  # the handle still works (and now grows the scratch)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Y), want[(True, "plain")])
    h.close()
