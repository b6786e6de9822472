"""The fused epilogue of the descriptor call (tcsc_hip_gemm_dev_ex,
TCSCDevice.gemm_torch_ex) through every kernel family on the GPU: ReLU / ReLU^2,
the gate multiply and the residual add on the finished fp32 value, before the
one rounding to the Y type.

The contract (include/ternary_spgemm.h): all fp32, one rounding per operation,
no fused multiply-add,

    y = t + b[n];  a = act(y);  a = a * widen(mul);  a = a + widen(add);  cast

with a NULL operand's operation not performed.  The expected Y is
test_gpu_scaled.expect32 (the oracle's chain, the scales, + b) through
tspgemm.epilogue_ref, then test_gpu_ytype._cast_bits for a 16-bit Y.  Everything
is compared as integers, no tolerance.

Inputs (asserted on the CPU in expect(), which test_epilogue_ref.py runs for
every case of this file without a GPU).  X is init_x_frac (int8: integer draws),
b = linspace(-3, 3, N), cs = U[0.5, 2) and rs = U[0.5, 2) * 2^-e with e chosen
per case from the chain's largest magnitude so that |y| <= 2^6 + 3: ReLU^2 then
stays below 2^13, its product with a gate below 2^14 and the sum with the
residual below 2^15, finite in fp16.  (An int8 X has chains below 2^12 where
init_x_frac's reach 2^25 -- test_gpu_scaled's reasoning; e follows the chain, so
y stays well above |b| <= 3 for both.)  The gate G = +-U[0.5, 2) and the
residual R[m, n] = U[-1, 1) * 2^ceil(log2 |a * G|[m, n]) (1 where the product is
0), each rounded to its own type: the chains of a real W are spread over many
binades (and ReLU^2 doubles the spread), so a residual scaled by the largest
product would swallow the product's rounding in most elements, and a fused
multiply-add would pass; scaled per element, the sum keeps the product's low
bits in play everywhere.
With both operands the fp32 expectation must differ, in at least 10 % of the
elements whose a is non-zero, from (a) the fused fp32(float64(a) * float64(G) +
float64(R)), (b) the add performed before the multiply and (c) a rounded to a
16-bit type before the multiply; RELU and RELU2 must differ from NONE in at
least 25 % of all elements; every expectation is finite, also after the cast.

Every call writes into a dense output and into the odd-stride sentinel view of
test_gpu_scaled._outputs; each operand lives in a buffer of NaN patterns of its
own, rows 1..M, columns 2..N+2 of an [M + 2, N + 5] buffer (the residual's:
[M + 2, N + 6]; row strides that are neither of Y's nor each other's).  Afterwards the operands' buffers, X, b, alpha and the scales
are byte-identical to before and only the view of Y was written."""
import collections
import functools
import types

import numpy as np
import pytest

from test_gpu_ldy import SENT, _assert_only_view_written, _dev, _fill, _jit_handle
from test_gpu_scaled import _chains, _got_bits, _outputs, _ybits_of, expect32
from test_gpu_xtype import _tdtype
from test_gpu_ytype import SENT16, YMAX, _assert_only_view_written16, _cast_bits, _fill16, _ybits, torch_from_bits

pytestmark = pytest.mark.gpu

YDTYPES = ("float32", "float16", "bfloat16")
ACTS = ("none", "prelu", "relu", "relu2")
KERNEL = {"pc": "tsg_tcsc_ell_pc_kernel", "walk": "tsg_tcsc_ell_kernel", "rows64": "tsg_jit64_kernel",
          "rows128": "tsg_jit_kernel", "rx": "tsg_tcsc_rx_kernel", "blocked": "tsg_jit_kernel"}

# name -> (family, M, K, N, width, knob, B): the shapes and handles of test_gpu_scaled.py
FAMILIES = collections.OrderedDict([
    ("pc-m1", ("pc", 1, 193, 301, 0, None, 0)),
    ("walk-m4", ("walk", 4, 193, 301, 0, None, 0)),
    ("walk-m16", ("walk", 16, 193, 301, 0, None, 0)),
    ("rows64-w128", ("rows64", 63, 193, 700, 128, None, 0)),
    ("rows64-w16", ("rows64", 65, 388, 700, 16, None, 0)),
    ("rows64-w8", ("rows64", 130, 193, 301, 8, None, 0)),
    ("rows64-4w", ("rows64", 65, 193, 700, 0, None, 0)),
    ("rows64-half", ("rows64", 65, 193, 700, 0, "TSG_JIT_HALF", 0)),
    ("rows64-pair", ("rows64", 65, 193, 700, 0, "TSG_JIT_PAIR", 0)),
    ("rows128-w64", ("rows128", 130, 388, 700, 64, None, 0)),
    ("rows128-4w", ("rows128", 130, 388, 700, 0, None, 0)),
    ("rx", ("rx", 130, 193, 301, 0, None, 0)),
    ("blocked", ("blocked", 130, 385, 700, 0, None, 64)),
])


@pytest.fixture(autouse=True)
def _oracle_built(oracle_mod):
    """The cached cases below import the oracle themselves: it is built first."""


# ---- the case builder (CPU only) ---------------------------------------------

@functools.lru_cache(maxsize=None)
def ecase(M, K, N, xdtype="float32", B=0, scaled=True):
    """One shape's inputs and its fp32 value before the epilogue (y32 = the
    scaled chain + b), computed once, never modified.  scaled=False: no scales,
    y32 = chain + b (fp32 Y only: its magnitudes are the chain's)."""
    arrays, Xt, Xw, chain = _chains(M, K, N, xdtype, "float32", B)
    b = np.linspace(-3, 3, N).astype(np.float32)
    alpha = np.linspace(-0.5, 0.5, N).astype(np.float32)
    rs = cs = None
    if scaled:
        top = float(np.abs(chain).max())
        assert top > 0
        e = int(np.ceil(np.log2(top))) + 2 - 6  # |chain * rs * cs| <= top * 2^-e * 4 <= 2^6
        rng = np.random.default_rng(7 * M + N + K)
        rs = (rng.uniform(0.5, 2.0, M).astype(np.float32) * np.float32(2.0 ** -e)).astype(np.float32)
        cs = rng.uniform(0.5, 2.0, N).astype(np.float32)
    y32 = expect32(chain, rs, cs, b)
    assert np.isfinite(y32).all()
    if scaled:
        assert float(np.abs(y32).max()) <= 2.0 ** 6 + 3
    for a in (b, alpha, y32) + ((rs, cs) if scaled else ()):
        a.setflags(write=False)
    return types.SimpleNamespace(arrays=arrays, Xt=Xt, b=b, alpha=alpha, rs=rs, cs=cs, y32=y32, M=M, K=K, N=N, B=B,
                                 xdtype=xdtype)


def _round_to(a32, dtype):
    """fp32 numpy -> (CPU tensor of the type, the tensor widened back to fp32)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a32)).to(_tdtype(dtype))
    return t, t.to(torch.float32).numpy()


def _share(x, y, where):
    return float(np.mean(x.view(np.uint32)[where] != y.view(np.uint32)[where]))


@functools.lru_cache(maxsize=None)
def expect(key, act, multype, addtype, ydtype, seed=0):
    """The operands and the expectation of one call on ecase(*key): G (multype
    or None) and R (addtype or None) as CPU tensors of their type, the fp32
    expectation and its bits in the Y type.  Asserts the module docstring's
    input conditions."""
    import tspgemm as T
    ec = ecase(*key)
    f = np.float32
    alpha = ec.alpha if act == "prelu" else None
    rng = np.random.default_rng(1000 * ec.M + ec.N + 17 * ACTS.index(act) + seed)
    a = T.epilogue_ref(ec.y32, act, alpha)
    Gt = Gw = Rt = Rw = None
    if multype:
        G = (rng.uniform(0.5, 2.0, a.shape) * rng.choice([-1.0, 1.0], a.shape)).astype(f)
        Gt, Gw = _round_to(G, multype)
    if addtype:
        p = np.abs(a.astype(np.float64) * (Gw if multype else 1.0))
        R = (rng.uniform(-1.0, 1.0, a.shape) * 2.0 ** np.ceil(np.log2(np.where(p > 0, p, 1.0)))).astype(f)
        Rt, Rw = _round_to(R, addtype)
    want32 = T.epilogue_ref(ec.y32, act, alpha, Gw, Rw)
    assert np.isfinite(want32).all(), (key, act, "the expectation is not finite")
    if ydtype != "float32":
        assert float(np.abs(want32).max()) <= YMAX[ydtype], (key, act, "the expectation overflows the Y type")
    if act in ("relu", "relu2"):
        frac = float(np.mean(a.view(np.uint32) != ec.y32.view(np.uint32)))
        assert frac >= 0.25, (key, act, "differs from NONE in only", frac)
    if multype and addtype:
        nz = a != 0
        d64 = np.float64
        t16 = multype if multype != "float32" else "bfloat16"
        alts = {
            "fused": (a.astype(d64) * Gw.astype(d64) + Rw.astype(d64)).astype(f),
            "add before multiply": ((a + Rw).astype(f) * Gw).astype(f),
            "a rounded to 16 bits first": ((_round_to(a, t16)[1] * Gw).astype(f) + Rw).astype(f),
        }
        for name, alt in alts.items():
            frac = _share(alt, want32, nz)
            assert frac >= 0.10, (name, "is told apart from the contract in only", frac, key, act, multype, addtype)
    bits = _ybits_of(want32, ydtype)
    for x in (want32, bits):
        x.setflags(write=False)
    return types.SimpleNamespace(Gt=Gt, Gw=Gw, Rt=Rt, Rw=Rw, want32=want32, bits=bits)


def family_key(name, xdtype="float32", scaled=True):
    fam, M, K, N, width, knob, B = FAMILIES[name]
    return (M, K, N, xdtype, B, scaled)


def family_combos(name, ydtype):
    """What test 1 runs on a family: with fp32 Y the product act x {mul, add,
    both} on fp32 operands; with a 16-bit Y relu2 with both operands and none
    with the add only, operands of the Y type.  (The blocked handle too: the
    PReLU is epilogue_ref's, on the oracle's plain blocked chain.)"""
    if ydtype == "float32":
        return [(a, m, d) for a in ACTS for m, d in (("float32", None), (None, "float32"), ("float32", "float32"))]
    return [("relu2", ydtype, ydtype), ("none", None, ydtype)]


TYPE_PRODUCT = [(m, a) for m in YDTYPES for a in YDTYPES]

# the seeded draw (test 10): a fixed list, one default_rng stream
Draw = collections.namedtuple("Draw", "family M K N act multype addtype mul_ld add_ld ydtype c0 pad seed")
DRAW_SEED, DRAWS = 20240611, 39
# The M a family's kernel keeps (test_gpu_call_fuzz.py's rules: the planner's own
# pick gives the producer/consumer walk its few rows; a forced walk stays at M
# <= 32; the pinned images, rx and a blocked handle take any M), around the tile
# sizes; K and N are drawn freely from the small ranges below (a blocked handle
# needs K >= B).
DRAW_M = {"pc": (1, 2), "walk": (3, 4, 5, 9, 15, 17, 31, 32), "rows64": (33, 63, 64, 65, 127, 129, 190),
          "rows128": (33, 127, 128, 129, 131, 190), "rx": (33, 70, 130, 190), "blocked": (33, 70, 129, 190)}
DRAW_K, DRAW_N = (20, 420), (5, 720)


@functools.lru_cache(maxsize=None)
def drawn_cases():
    rng = np.random.default_rng(DRAW_SEED)
    names = [n for n in FAMILIES]
    out = []
    for i in range(DRAWS):
        fam = names[i % len(names)]  # three shapes of every family
        kind, B = FAMILIES[fam][0], FAMILIES[fam][6]
        M = DRAW_M[kind][int(rng.integers(len(DRAW_M[kind])))]
        K = max(int(rng.integers(DRAW_K[0], DRAW_K[1] + 1)), B)
        N = int(rng.integers(DRAW_N[0], DRAW_N[1] + 1))
        act = ACTS[int(rng.integers(4))]
        types_ = (None,) + YDTYPES
        mt, at = types_[int(rng.integers(4))], types_[int(rng.integers(4))]
        if mt is None and at is None and act in ("none", "prelu"):
            at = "bfloat16"  # (a descriptor without an epilogue is test 3's)
        out.append(Draw(fam, M, K, N, act, mt, at, int(rng.integers(0, 9)), int(rng.integers(0, 9)),
                        YDTYPES[int(rng.integers(3))], int(rng.integers(0, 5)), int(rng.integers(0, 4)), i))
    return tuple(out)


def draw_key(c):
    return (c.M, c.K, c.N, "float32", FAMILIES[c.family][6], True)


def build_draw(c):
    return expect(draw_key(c), c.act, c.multype, c.addtype, c.ydtype, c.seed)


def all_builds():
    """Every (key, act, multype, addtype, ydtype[, seed]) the family, type
    product and drawn tests of this file run: test_epilogue_ref.py builds them
    all on the CPU."""
    out = []
    for name in FAMILIES:
        for yd in YDTYPES:
            out += [(family_key(name), a, m, d, yd) for a, m, d in family_combos(name, yd)]
    for name in ("walk-m16", "rows64-w16"):
        for yd in YDTYPES:
            out += [(family_key(name), "relu2", m, d, yd) for m, d in TYPE_PRODUCT]
    out += [(family_key("rows64-w16", "int8"), "relu2", "bfloat16", "float16", yd) for yd in YDTYPES]
    return out


# ---- running one call ------------------------------------------------------------

def open_handle(tsg, monkeypatch, name, arrays, shape=None):
    """The handle of a family, with the kernel that a call of its M runs
    asserted.  shape: a drawn (M, K, N) in place of the family's own -- a walk is
    then forced as test_gpu_call_fuzz.py forces it, and an automatic image
    shape (width 0) may have 4 or 8 waves."""
    fam, M, K, N, width, knob, B = FAMILIES[name]
    if shape:
        M, K, N = shape
    for k in ("TSG_JIT_HALF", "TSG_JIT_PAIR", "TSG_KERNEL"):
        monkeypatch.delenv(k, raising=False)
    if knob:
        monkeypatch.setenv(knob, "1")
    if fam == "rx":
        monkeypatch.setenv("TSG_KERNEL", "rx")
    if fam in ("pc", "walk"):
        h = tsg.TCSCDevice(*arrays, K, N)
        # (M = 4: the producer/consumer walk switched off, as test_gpu_ldy; a drawn walk is forced)
        h.set_small_m(0 if fam == "pc" else 3 if M <= 4 else 2 if shape else 0)
    elif fam == "rx":
        h = tsg.TCSCDevice(*arrays, K, N)
        h.set_small_m(1)
    elif fam == "blocked":
        h = tsg.TCSCDevice.from_blocked(*arrays, K, N, B)
        h.set_small_m(1)
    else:
        h = _jit_handle(tsg, arrays, K, N, 64 if fam == "rows64" else 128, width)
    assert h.call_kernel(M) == KERNEL[fam], (name, h.call_kernel(M))
    if fam in ("rows64", "rows128"):
        assert h.call_tile_rows(M) == (64 if fam == "rows64" else 128)
        if width:
            assert h.jit_width(M) == width and h.jit_waves(M) == 8
        elif not shape:
            assert h.jit_waves(M) == 4, (h.jit_width(M), h.jit_waves(M))
    return h


def place(t, c0=2, pad=3):
    """A CPU [M, N] tensor -> (buffer, view): the values in rows 1..M, columns
    c0..c0+N of an [M + 2, c0 + N + pad] device buffer of NaN patterns."""
    import torch
    if t is None:
        return None, None
    M, N = t.shape
    buf = torch.empty((M + 2, c0 + N + pad), dtype=t.dtype, device="cuda")
    if t.dtype == torch.float32:
        buf.view(torch.int32).fill_(SENT)
    else:
        buf.view(torch.int16).fill_(SENT16)
    view = buf[1:M + 1, c0:c0 + N]
    view.copy_(t)
    return buf, view


def same_bytes(t, k):
    import torch
    return t.dtype == k.dtype and t.shape == k.shape and \
        torch.equal(t.contiguous().view(torch.int8), k.contiguous().view(torch.int8))


class Inputs:
    """X, b, alpha and the scales of a case on the device, with copies to compare against.
    X: the case's X already on the device (a slice, say); extra: further (name,
    tensor or None) pairs to keep a copy of (test_gpu_ex_fuzz.py: gamma)."""

    def __init__(self, ec, X=None, extra=()):
        self.X, self.b, self.alpha = ec.Xt.cuda() if X is None else X, _dev(ec.b), _dev(ec.alpha)
        self.rs = None if ec.rs is None else _dev(ec.rs)
        self.cs = None if ec.cs is None else _dev(ec.cs)
        self.named = [(n, t) for n, t in (("X", self.X), ("b", self.b), ("alpha", self.alpha),
                                          ("row_scale", self.rs), ("col_scale", self.cs)) + tuple(extra) if t is not None]
        self.keep = [t.clone() for _, t in self.named]

    def assert_unchanged(self, what):
        for (n, t), k in zip(self.named, self.keep):
            assert same_bytes(t, k), (what, n, "was written")


def run_call(h, inp, view, act, mul, add):
    return h.gemm_torch_ex(inp.X, inp.b, view, act=act, alpha=inp.alpha if act == "prelu" else None, mul=mul, add=add,
                           row_scale=inp.rs, col_scale=inp.cs)


def assert_bits(got, want, tag):
    bad = got != want
    assert not bad.any(), (tag, int(bad.sum()), "of", want.size, "elements differ, first at (row, col)",
                           np.argwhere(bad)[:4].tolist())


def check_ex(h, key, ydtype, combos, what, outs_kw=None, seeds=None, lds=None):
    """The shared scheme (module docstring) for one handle and a list of (act, multype, addtype)."""
    import torch
    ec = ecase(*key)
    inp = Inputs(ec)
    outs = _outputs(ec.M, ec.N, ydtype, **(outs_kw or {}))
    for i, (act, mt, at) in enumerate(combos):
        ex = expect(key, act, mt, at, ydtype, seeds[i] if seeds else 0)
        mc0, ac0 = lds[i] if lds else (2, 2)
        mbuf, mview = place(ex.Gt, mc0, 3)
        abuf, aview = place(ex.Rt, ac0, 4)
        keep = [None if t is None else t.clone() for t in (mbuf, abuf)]
        for name, (buf, view, box, fill, only) in outs.items():
            tag = (what, ydtype, act, mt, at, name)
            fill(buf)
            out = run_call(h, inp, view, act, mview, aview)
            torch.cuda.synchronize()
            assert out is view
            assert_bits(_got_bits(view, ydtype), ex.bits, tag)
            only(buf, *box, tag)
        for t, k, n in zip((mbuf, abuf), keep, ("mul", "add")):
            assert t is None or same_bytes(t, k), (what, act, n, "buffer was written")
    inp.assert_unchanged(what)


# ---- 1. every kernel family -------------------------------------------------------

@pytest.mark.parametrize("ydtype", YDTYPES)
@pytest.mark.parametrize("name", list(FAMILIES))
def test_epilogue_every_family(tsg, monkeypatch, name, ydtype):
    key = family_key(name)
    h = open_handle(tsg, monkeypatch, name, ecase(*key).arrays)
    check_ex(h, key, ydtype, family_combos(name, ydtype), name)
    h.close()


# ---- 2. the type product ---------------------------------------------------------------

@pytest.mark.parametrize("ydtype", YDTYPES)
@pytest.mark.parametrize("name", ["walk-m16", "rows64-w16"])
def test_epilogue_type_product(tsg, monkeypatch, name, ydtype):
    """multype x addtype x ytype are independent: relu2 with both operands."""
    key = family_key(name)
    h = open_handle(tsg, monkeypatch, name, ecase(*key).arrays)
    check_ex(h, key, ydtype, [("relu2", m, a) for m, a in TYPE_PRODUCT], ("product", name))
    h.close()


@pytest.mark.parametrize("ydtype", YDTYPES)
def test_epilogue_int8_x_with_scales(tsg, monkeypatch, ydtype):
    key = family_key("rows64-w16", "int8")
    h = open_handle(tsg, monkeypatch, "rows64-w16", ecase(*key).arrays)
    check_ex(h, key, ydtype, [("relu2", "bfloat16", "float16")], "int8 X")
    h.close()


# ---- 3. legacy equivalence, GPU against GPU ------------------------------------------------

@pytest.mark.parametrize("ydtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("name", ["walk-m16", "rows64-w16", "rows128-w64"])
def test_descriptor_restates_the_existing_calls(tsg, monkeypatch, name, ydtype):
    """act none / prelu and no operand: the descriptor IS the existing call.
    The bit comparison carries this test; beside it, the handle's timing ring
    counts the same number of timed kernel launches for both calls and the work
    buffer does not grow.  (call_kernel and call_launches ask the plan, which
    no entry point changes: they are asserted once, for the record.)"""
    import torch
    key = family_key(name, "bfloat16")
    ec = ecase(*key)
    h = open_handle(tsg, monkeypatch, name, ec.arrays)
    inp = Inputs(ec)
    dt = _tdtype(ydtype)
    gamma = _dev(np.linspace(0.5, 1.5, ec.K).astype(np.float32))
    kernel, launches = h.call_kernel(ec.M), h.call_launches(inp.X, ec.M)
    h.set_timing(True)
    for act, al in (("none", None), ("prelu", inp.alpha)):
        pairs = [
            ("xy", lambda: h.gemm_torch_xy(inp.X, inp.b, alpha=al, out_dtype=dt),
             lambda: h.gemm_torch_ex(inp.X, inp.b, act=act, alpha=al, out_dtype=dt)),
            ("scaled", lambda: h.gemm_torch_scaled(inp.X, inp.b, alpha=al, out_dtype=dt, row_scale=inp.rs,
                                                   col_scale=inp.cs),
             lambda: h.gemm_torch_ex(inp.X, inp.b, act=act, alpha=al, out_dtype=dt, row_scale=inp.rs,
                                     col_scale=inp.cs)),
            ("actquant", lambda: h.gemm_torch_actquant(inp.X, inp.b, alpha=al, out_dtype=dt, col_scale=inp.cs),
             lambda: h.gemm_torch_ex(inp.X, inp.b, act=act, alpha=al, out_dtype=dt, col_scale=inp.cs, quant="act")),
            ("normquant", lambda: h.gemm_torch_normquant(inp.X, inp.b, gamma, 1e-5, alpha=al, out_dtype=dt,
                                                         col_scale=inp.cs),
             lambda: h.gemm_torch_ex(inp.X, inp.b, act=act, alpha=al, out_dtype=dt, col_scale=inp.cs, quant="norm",
                                     gamma=gamma, eps=1e-5)),
        ]
        for call, old, new in pairs:
            h.kernel_time(reset=True)
            Y0 = old()
            torch.cuda.synchronize()
            n0, work = h.kernel_time(reset=True)[1], h.info()["work_bytes"]
            Y1 = new()
            torch.cuda.synchronize()
            n1 = h.kernel_time(reset=True)[1]
            assert Y0.dtype == Y1.dtype == dt
            assert same_bytes(Y0, Y1), (name, ydtype, call, act, "the descriptor call's bits differ")
            assert n0 == n1 >= 1 and h.info()["work_bytes"] == work, (call, act, n0, n1)
    assert h.call_kernel(ec.M) == kernel and h.call_launches(inp.X, ec.M) == launches
    h.set_timing(False)
    # the row scale out of a quantising descriptor is the existing call's too
    d0, d1 = torch.zeros(ec.M, device="cuda"), torch.zeros(ec.M, device="cuda")
    h.gemm_torch_actquant(inp.X, inp.b, out_dtype=dt, row_scale_out=d0)
    h.gemm_torch_ex(inp.X, inp.b, out_dtype=dt, quant="act", row_scale_out=d1)
    torch.cuda.synchronize()
    assert same_bytes(d0, d1) and bool((d0 > 0).all())
    inp.assert_unchanged(name)
    h.close()


# ---- 4. the in-place residual -------------------------------------------------------------------

def inplace_outputs(M, N, ydtype):
    """An aligned dense Y (every row starts on 16 bytes: the vector path where a
    lane's segment is full) and the odd view."""
    import torch
    dt = _tdtype(ydtype)
    ld = (N + 7) // 8 * 8 + 8
    dense = torch.empty((M + 2, ld), dtype=dt, device="cuda")
    odd = torch.empty((M + 2, N + 3), dtype=dt, device="cuda")
    assert dense.data_ptr() % 16 == 0
    return {"aligned": (dense, dense[1:M + 1, 0:N], (1, M + 1, 0, N)),
            "odd": (odd, odd[1:M + 1, 1:N + 1], (1, M + 1, 1, N + 1))}


@pytest.mark.parametrize("ydtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("name", ["walk-m16", "rows64-w128", "rx", "pc-m1", "rows128-w64"])
def test_epilogue_in_place(tsg, monkeypatch, name, ydtype):
    """add = Y (h += proj(x)) and, once, mul = Y: Y is the expectation computed
    from its previous contents, the sentinels around it are intact."""
    import torch
    fill, only = (_fill, _assert_only_view_written) if ydtype == "float32" else (_fill16, _assert_only_view_written16)
    key = family_key(name)
    ec = ecase(*key)
    h = open_handle(tsg, monkeypatch, name, ec.arrays)
    inp = Inputs(ec)
    other = "float16" if ydtype == "float32" else "float32"
    for which in ("add", "mul"):
        ex = expect(key, "relu2", ydtype if which == "mul" else other, ydtype if which == "add" else other, ydtype)
        mine, theirs = (ex.Rt, ex.Gt) if which == "add" else (ex.Gt, ex.Rt)
        obuf, oview = place(theirs)
        okeep = obuf.clone()
        for oname, (buf, view, box) in inplace_outputs(ec.M, ec.N, ydtype).items():
            tag = (name, ydtype, which, oname)
            fill(buf)
            view.copy_(mine.cuda())
            if which == "add":
                out = run_call(h, inp, view, "relu2", oview, view)
            else:
                out = run_call(h, inp, view, "relu2", view, oview)
            torch.cuda.synchronize()
            assert out is view
            assert_bits(_got_bits(view, ydtype), ex.bits, tag)
            only(buf, *box, tag)
        assert same_bytes(obuf, okeep)
    inp.assert_unchanged(name)
    h.close()


# ---- 5. alignment and raggedness ---------------------------------------------------------------------

ALIGN = collections.OrderedDict([
    ("n700-w128", ("rows64", 63, 193, 700, 128)),
    ("n301-w8", ("rows64", 130, 193, 301, 8)),
    ("n301-walk", ("walk", 16, 193, 301, 0)),
    ("n5-w8", ("rows64", 65, 193, 5, 8)),
    ("n5-rx", ("rx", 65, 193, 5, 0)),
])


@pytest.mark.parametrize("opdtype", YDTYPES)
@pytest.mark.parametrize("name", list(ALIGN))
def test_epilogue_operand_alignment(tsg, monkeypatch, name, opdtype):
    """The same operand values in a 16-byte-aligned dense buffer and in one
    offset by an element with an odd row stride: the same bits, and the
    expectation's.  A ragged last tile (N = 700 at width 128), N = 301 and
    N = 5 < 8; Y of the operands' type, dense-aligned and odd."""
    import torch
    fam, M, K, N, width = ALIGN[name]
    scaled = opdtype != "float32"  # (the fp32 run has no scales: the kernels' unscaled calls with an epilogue)
    key = (M, K, N, "float32", 0, scaled)
    ec = ecase(*key)
    for k in ("TSG_JIT_HALF", "TSG_JIT_PAIR", "TSG_KERNEL"):
        monkeypatch.delenv(k, raising=False)
    if fam == "rx":
        monkeypatch.setenv("TSG_KERNEL", "rx")
        h = tsg.TCSCDevice(*ec.arrays, K, N)
        h.set_small_m(1)
    elif fam == "walk":
        h = tsg.TCSCDevice(*ec.arrays, K, N)
    else:
        h = _jit_handle(tsg, ec.arrays, K, N, 64, width)
        assert h.jit_width(M) == width
    assert h.call_kernel(M) == KERNEL[fam]
    inp = Inputs(ec)
    ex = expect(key, "relu2", opdtype, opdtype, opdtype)
    dt = _tdtype(opdtype)
    ld = (N + 7) // 8 * 8
    results = []
    for layout in ("aligned", "offset"):
        if layout == "aligned":
            mbuf, abuf, ybuf = (torch.zeros((M, ld), dtype=dt, device="cuda") for _ in range(3))
            mview, aview, yview = mbuf[:, :N], abuf[:, :N], ybuf[:, :N]
            assert all(t.data_ptr() % 16 == 0 for t in (mview, aview, yview))
        else:
            mbuf, mview = place(ex.Gt, 1, 2 + N % 2)  # an odd row stride, one element off the buffer's base
            abuf, aview = place(ex.Rt, 1, 2 + N % 2)
            ybuf = torch.zeros((M + 2, N + 3 - (N % 2)), dtype=dt, device="cuda")
            yview = ybuf[1:M + 1, 1:N + 1]
            assert mview.stride(0) % 2 == 1 and aview.stride(0) % 2 == 1
        if layout == "aligned":
            mview.copy_(ex.Gt.cuda())
            aview.copy_(ex.Rt.cuda())
        out = run_call(h, inp, yview, "relu2", mview, aview)
        torch.cuda.synchronize()
        results.append(_got_bits(out, opdtype))
        assert_bits(results[-1], ex.bits, (name, opdtype, layout))
    assert np.array_equal(results[0], results[1])
    h.close()


# ---- 6. special values -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def special_case():
    """M = 5, N = 8, K = 40.  Column 0 of W is empty, so chain[:, 0] = +0; with
    b[0] = -0 and a negative rs[1] row 1 has y = -0 there, the other rows +0.
    rs[3] = 2^100 makes row 3 overflow under RELU2.  G holds 0, -0, inf and NaN
    and R holds +-inf at known places."""
    import oracle as O
    M, K, N = 5, 40, 8
    rng = np.random.default_rng(11)
    W = np.zeros((K, N), np.int32)
    for n in range(1, N):
        rows = rng.choice(K, size=3 + n, replace=False)
        W[rows, n] = rng.choice([-1, 1], size=rows.size)
    t = O.tcsc_encode(W)
    X = rng.integers(-8, 9, size=(M, K)).astype(np.float32)
    chain = O.base_tcsc(X, t, np.zeros(N, np.float32))
    assert (chain[:, 0] == 0).all() and not np.signbit(chain[:, 0]).any()
    b = np.linspace(-3, 3, N).astype(np.float32)
    b[0] = np.float32(-0.0)
    rs = np.array([1.0, -1.0, 0.5, 2.0 ** 100, 3.0], np.float32)
    with np.errstate(all="ignore"):
        y = expect32(chain, rs, None, b)
    assert np.signbit(y[1, 0]) and y[1, 0] == 0 and not np.signbit(y[0, 0]) and y[0, 0] == 0
    assert (np.abs(y[3]) > 2.0 ** 90).any() and (y[3] > 0).any()
    G = rng.uniform(0.5, 2.0, (M, N)).astype(np.float32)
    R = rng.uniform(-4.0, 4.0, (M, N)).astype(np.float32)
    G[0, 1], G[0, 2], G[0, 3], G[0, 4] = 0.0, -0.0, np.inf, np.nan
    G[3, :4] = (0.0, -0.0, np.inf, -np.inf)     # against the overflowed row: 0 * inf = NaN
    G[1, 0], G[2, 0] = -1.0, np.inf             # against y = -0 and y = +0
    R[0, 5], R[0, 6] = np.inf, -np.inf
    R[3, 4:8] = (np.inf, -np.inf, np.inf, -np.inf)  # inf + -inf = NaN where the product is +inf
    R[4, 0] = -0.0
    return t.arrays, X, b, rs, y, G, R, M, K, N


@pytest.mark.parametrize("act", ["relu", "relu2", "none"])
@pytest.mark.parametrize("family", ["walk", "rows64"])
def test_epilogue_special_values(tsg, family, act):
    import torch
    arrays, X, b, rs, y, G, R, M, K, N = special_case()
    with np.errstate(all="ignore"):
        want = tsg.epilogue_ref(y, act, None, G, R)
    if act != "none":
        assert want.view(np.uint32)[1, 0] == (np.float32(0.0) * G[1, 0] + R[1, 0]).astype(np.float32).view(np.uint32)
        r = tsg.epilogue_ref(y, act)
        assert not np.signbit(r[1, 0]) and r[1, 0] == 0, "relu(-0) is not +0"
    if act == "relu2":
        with np.errstate(all="ignore"):
            assert np.isinf(tsg.epilogue_ref(y, act)[3]).any(), "no RELU2 overflow"
    nan = np.isnan(want)
    assert nan.any() and np.isinf(want).any()
    if family == "walk":
        h = tsg.TCSCDevice(*arrays, K, N)
        assert h.call_kernel(M) == "tsg_tcsc_ell_kernel"
    else:
        h = _jit_handle(tsg, arrays, K, N, 64, 8)
        assert h.call_kernel(M) == "tsg_jit64_kernel"
    Xd, bd, rd = _dev(X), _dev(b), _dev(rs)
    mbuf, mview = place(torch.from_numpy(G))
    abuf, aview = place(torch.from_numpy(R))
    Y = h.gemm_torch_ex(Xd, bd, act=act, mul=mview, add=aview, row_scale=rd)
    torch.cuda.synchronize()
    g = Y.cpu().numpy()
    assert np.array_equal(np.isnan(g), nan), (family, act, "NaN positions differ")
    bad = (g.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not bad.any(), (family, act, int(bad.sum()), "elements differ", np.argwhere(bad)[:8].tolist())
    h.close()


# ---- 7. errors on a live handle ------------------------------------------------------------------------------

def _set(**kw):
    def f(d):
        for k, v in kw.items():
            setattr(d, k, v)
    return f


def error_mutations(N):
    """(the field the message must name, what to do to a valid PLAIN descriptor
    that has both operands): every error of the header's Errors paragraph."""
    nan, inf = float("nan"), float("inf")
    p = 0x1000  # a non-NULL pointer that is never read: the checks are host arithmetic
    return [
        ("struct_size", _set(struct_size=140)), ("struct_size", _set(struct_size=152)), ("struct_size", _set(struct_size=0)),
        ("reserved", _set(reserved=1)),
        ("in_mode", _set(in_mode=3)), ("in_mode", _set(in_mode=-1)),
        ("act", _set(act=4)), ("act", _set(act=-1)),
        ("xtype", _set(xtype=4)), ("xtype", _set(xtype=-1)),
        ("ytype", _set(ytype=3)), ("ytype", _set(ytype=-1)),
        ("multype", _set(multype=3)), ("multype", _set(multype=-1)),
        ("addtype", _set(addtype=3)), ("addtype", _set(addtype=-1)),
        ("ldY", _set(ldY=N - 1)), ("ldmul", _set(ldmul=N - 1)), ("ldadd", _set(ldadd=N - 1)),
        ("dalpha", _set(act=1, dalpha=None)),
        ("xtype", _set(in_mode=1, xtype=3)), ("xtype", _set(in_mode=2, xtype=3, eps=1e-5)),
        ("eps", _set(in_mode=2, eps=0.0)), ("eps", _set(in_mode=2, eps=-1.0)), ("eps", _set(in_mode=2, eps=nan)),
        ("eps", _set(in_mode=2, eps=inf)),
        ("dgamma", _set(dgamma=p)), ("dgamma", _set(in_mode=1, dgamma=p)),
        ("drow_scale", _set(in_mode=1, drow_scale=p)), ("drow_scale", _set(in_mode=2, eps=1e-5, drow_scale=p)),
        ("drow_scale_out", _set(drow_scale_out=p)),
    ]


def test_epilogue_errors_leave_y_untouched(tsg, monkeypatch):
    import torch
    key = family_key("walk-m16", "bfloat16")
    ec = ecase(*key)
    M, N = ec.M, ec.N
    h = open_handle(tsg, monkeypatch, "walk-m16", ec.arrays)
    inp = Inputs(ec)
    ex = expect(key, "relu2", "bfloat16", "bfloat16", "bfloat16")
    mbuf, mview = place(ex.Gt)
    abuf, aview = place(ex.Rt)
    buf = torch.empty((M + 2, 2 * N), dtype=torch.bfloat16, device="cuda")
    buf.view(torch.int16).fill_(SENT16)

    def valid():
        return tsg.tsg_gemm_ex(in_mode=0, act=3, dX=inp.X.data_ptr(), xtype=tsg.TSG_X_BF16, ytype=tsg.TSG_Y_BF16,
                               dcol_scale=inp.cs.data_ptr(), db=inp.b.data_ptr(), dalpha=inp.alpha.data_ptr(),
                               dmul=mview.data_ptr(), ldmul=mview.stride(0), multype=2, dadd=aview.data_ptr(),
                               ldadd=aview.stride(0), addtype=2, dY=buf[1:].data_ptr(), ldY=2 * N)
    for field, mutate in error_mutations(N):
        d = valid()
        mutate(d)
        with pytest.raises(tsg.TSGError, match=field) as e:
            h.gemm_dev_ex(d, M)
        assert e.value.code == 1, field  # TSG_ERR_ARG
    with pytest.raises(tsg.TSGError) as e:
        h.gemm_dev_ex(None, M)
    assert e.value.code == 1
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int16) == SENT16).all()), "a refused call wrote Y"
    h.gemm_dev_ex(valid(), M)  # the descriptor the mutations start from is a good one
    torch.cuda.synchronize()
    y = expect32(_chains(ec.M, ec.K, ec.N, "bfloat16", "float32", 0)[3], None, ec.cs, ec.b)
    want = _cast_bits(tsg.epilogue_ref(y, "relu2", None, ex.Gw, ex.Rw), "bfloat16")
    assert np.array_equal(_ybits(buf[1:M + 1, :N]), want)
    h.close()


# ---- 8. graph capture ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,inplace", [("rows64-w16", False), ("walk-m16", True)])
def test_epilogue_graph_capture_after_reserve(tsg, monkeypatch, name, inplace):
    """After reserve(M): one captured relu2 call with both operands on the
    64-row image, one captured in-place residual call on the walk; two replays,
    the second after the operands were rewritten in place."""
    import torch
    key = family_key(name, "bfloat16")
    ec = ecase(*key)
    M, N = ec.M, ec.N
    h = open_handle(tsg, monkeypatch, name, ec.arrays)
    h.reserve(M)
    work = h.info()["work_bytes"]
    inp = Inputs(ec)
    exs = [expect(key, "relu2", "float16", "bfloat16", "bfloat16", seed) for seed in (0, 1)]
    assert not np.array_equal(exs[0].bits, exs[1].bits)
    mbuf, mview = place(exs[0].Gt)
    abuf, aview = place(exs[0].Rt)
    buf = torch.empty((M + 2, N + 3), dtype=torch.bfloat16, device="cuda")
    view = buf[1:M + 1, 1:N + 1]
    add = view if inplace else aview
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture
        run_call(h, inp, view, "relu2", mview, add)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run_call(h, inp, view, "relu2", mview, add)
    assert h.info()["work_bytes"] == work
    for replay, ex in enumerate(exs):
        mview.copy_(ex.Gt.cuda())
        aview.copy_(ex.Rt.cuda())
        buf.view(torch.int16).fill_(SENT16)
        if inplace:
            view.copy_(ex.Rt.cuda())
        g.replay()
        torch.cuda.synchronize()
        assert_bits(_ybits(view), ex.bits, (name, "replay", replay))
        _assert_only_view_written16(buf, 1, M + 1, 1, N + 1, ("graph replay", replay))
    assert h.info()["work_bytes"] == work
    h.close()


# ---- 9. the motivating block ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ffn_case():
    """A gated FFN block with its residual, bf16 activations throughout, as
    three calls: up = norm-quant(x) W_up; g = relu2(norm-quant(x) W_gate) * up;
    h += act-quant(g) W_down.  Everything expected on the CPU."""
    import torch
    import oracle as O
    import tspgemm as T
    M, d, ffn, eps = 33, 256, 512, 1e-5
    rng = np.random.default_rng(2024)
    f = np.float32
    bf = lambda a: _round_to(a, "bfloat16")
    xt, xw = bf((rng.standard_normal((M, d)) * 1.5).astype(f))
    gamma = rng.uniform(0.5, 1.5, d).astype(f)
    W = {n: O.tcsc_encode(O.gen_ternary(k, nn, 4, seed)) for n, k, nn, seed in
         (("up", d, ffn, 1), ("gate", d, ffn, 2), ("down", ffn, d, 3))}
    cs = {n: (rng.uniform(0.5, 2.0, nn) * 2.0 ** e).astype(f) for n, nn, e in (("up", ffn, -2), ("gate", ffn, -2),
                                                                               ("down", d, -4))}
    b = {n: rng.uniform(-0.5, 0.5, nn).astype(f) for n, nn in (("up", ffn), ("gate", ffn), ("down", d))}
    xn, _ = T.rms_norm_ref(xw, gamma, eps)
    q, deq = T.act_quant_ref(xn)
    qf = q.astype(f)
    y_up = expect32(O.base_tcsc(qf, W["up"], np.zeros(ffn, f)), deq, cs["up"], b["up"])
    up_bits = _cast_bits(T.epilogue_ref(y_up, "none"), "bfloat16")
    upw = torch_from_bits(up_bits, "bfloat16")
    y_g = expect32(O.base_tcsc(qf, W["gate"], np.zeros(ffn, f)), deq, cs["gate"], b["gate"])
    g_bits = _cast_bits(T.epilogue_ref(y_g, "relu2", None, upw), "bfloat16")
    gw = torch_from_bits(g_bits, "bfloat16")
    assert np.isfinite(gw).all() and (gw != 0).mean() > 0.25
    q2, deq2 = T.act_quant_ref(gw)
    y_d = expect32(O.base_tcsc(q2.astype(f), W["down"], np.zeros(d, f)), deq2, cs["down"], b["down"])
    top = float(np.abs(y_d).max())
    ht, hw = bf((rng.uniform(-1.0, 1.0, (M, d)) * 2.0 ** int(np.ceil(np.log2(top)))).astype(f))
    h_bits = _cast_bits(T.epilogue_ref(y_d, "none", None, None, hw), "bfloat16")
    h_new = torch_from_bits(h_bits, "bfloat16")
    assert np.isfinite(h_new).all(), "the expected h is not finite in bf16"
    # the residual is non-trivial where the projection is at least an ulp of h: there h must change
    live = np.abs(y_d) >= np.abs(hw) * 2.0 ** -7
    assert live.mean() >= 0.5, live.mean()
    assert (h_new[live] != hw[live]).all(), "the residual add does not show"
    return types.SimpleNamespace(M=M, d=d, ffn=ffn, eps=eps, xt=xt, gamma=gamma, W=W, cs=cs, b=b, ht=ht,
                                 up_bits=up_bits, g_bits=g_bits, h_bits=h_bits)


def test_epilogue_gated_ffn_block(tsg):
    """Three calls, no elementwise pass: bit for bit the CPU's rms_norm_ref,
    act_quant_ref, the oracle's chains, expect32 and epilogue_ref."""
    import torch
    c = ffn_case()
    hs = {n: tsg.TCSCDevice(*c.W[n].arrays, k, nn) for n, k, nn in (("up", c.d, c.ffn), ("gate", c.d, c.ffn),
                                                                    ("down", c.ffn, c.d))}
    known = set(KERNEL.values())
    assert all(hs[n].call_kernel(c.M) in known for n in hs)
    x, gamma, h = c.xt.cuda(), _dev(c.gamma), c.ht.cuda()
    cs = {n: _dev(v) for n, v in c.cs.items()}
    b = {n: _dev(v) for n, v in c.b.items()}
    bf16 = torch.bfloat16
    up = hs["up"].gemm_torch_ex(x, b["up"], out_dtype=bf16, col_scale=cs["up"], quant="norm", gamma=gamma, eps=c.eps)
    g = hs["gate"].gemm_torch_ex(x, b["gate"], out_dtype=bf16, act="relu2", mul=up, col_scale=cs["gate"], quant="norm",
                                 gamma=gamma, eps=c.eps)
    out = hs["down"].gemm_torch_ex(g, b["down"], h, add=h, col_scale=cs["down"], quant="act")
    torch.cuda.synchronize()
    assert out is h
    assert_bits(_ybits(up), c.up_bits, "up")
    assert_bits(_ybits(g), c.g_bits, "gate")
    assert_bits(_ybits(h), c.h_bits, "h")
    for v in hs.values():
        v.close()


# ---- 10. a small seeded draw -------------------------------------------------------------------------------------------------

def draw_id(c):
    return f"{c.seed}-{c.family}-{c.M}x{c.K}x{c.N}-{c.act}"


@pytest.mark.parametrize("c", drawn_cases(), ids=draw_id)
def test_epilogue_drawn_case(tsg, monkeypatch, c):
    key = draw_key(c)
    h = open_handle(tsg, monkeypatch, c.family, ecase(*key).arrays, shape=(c.M, c.K, c.N))
    check_ex(h, key, c.ydtype, [(c.act, c.multype, c.addtype)], c, outs_kw=dict(c0=c.c0, pad=c.pad), seeds=[c.seed],
             lds=[(c.mul_ld, c.add_ld)])
    h.close()
