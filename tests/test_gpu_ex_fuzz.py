"""Seeded shape, mode and layout fuzz over the descriptor call
(tcsc_hip_gemm_dev_ex, TCSCDevice.gemm_torch_ex) with its fused epilogue,
through every kernel family on the GPU.  test_gpu_epilogue.py pins the
epilogue's arithmetic on PLAIN calls with fp32 X; test_gpu_call_fuzz.py walks the
indexing of the calls that the descriptor restates, without going through it.
This file is where the two meet: an epilogue on the quantising in_modes through
every family, walks with K above their LDS chunk with operands, N below a store
group, the three alignment decisions of the epilogue's store (Y, mul, add) in
every combination, the in-place forms, operands with row strides of their own
over many M tiles, unusual W, X off alignment.

The reference.  Every case is one gemm_torch_ex call, compared as integers, no
tolerance.  The expected Y is the contract of include/ternary_spgemm.h, step by
step: X widened exactly; NORMQUANT tspgemm.rms_norm_ref, both quantising modes
tspgemm.act_quant_ref; the oracle's chain (base_tcsc / base_blocked_tcsc) with a
zero bias; test_gpu_scaled.expect32 with the row scale (deq in the quantising
modes), the column scale and b; tspgemm.epilogue_ref with act, the widened mul
and the widened add; test_gpu_ytype._cast_bits for a 16-bit Y.  row_scale_out
must hold deq bit for bit.

After its call a case asserts the kernel that ran (call_kernel, and jit_width /
jit_waves / call_tile_rows where pinned), every element of the Y view, every
element of Y's buffer outside the view still the sentinel, the operands' buffers
byte-identical to before (an in-place operand is Y), row_scale_out's slice equal
to deq and its surroundings untouched, and X, b, alpha, the scales and gamma
byte-identical to before.

Inputs (build() asserts all of this on the CPU; test_ex_fuzz_ref.py runs it for
every case).  X, W, b, alpha and gamma are test_gpu_call_fuzz.build's, with its
edge-dependence conditions: W nonzero in rows 0 and K - 1 and columns 0 and
N - 1, X nonzero at both ends of every ordinary row, zeroing X[:, K - 1] (and a
chunked walk's last chunk) changes y, rows M - 1 and M - 2 of the expectation
differ.  Magnitude: rs and cs are U[0.5, 2); a case with a column scale (every
quantising case has one) carries the exact power of two 2^-e in it, e from the
largest |chain * rs * cs|, so that |y| <= 2^6 + 3 (test_gpu_epilogue.ecase's
bound: ReLU^2, the gate product and the residual sum stay finite in fp16); a
PLAIN case with the row scale only carries it there; a PLAIN case with no scale
(the _xy restatement) keeps the chain's magnitudes and has fp32 or bf16 Y and
operands and act none, prelu or relu.  The operands are test_gpu_epilogue.expect's:
G = +-U[0.5, 2), R[m, n] = U[-1, 1) * 2^ceil(log2 |a * G|) (1 where the product
is 0), each rounded to its own type.  A case with both operands and at least 200
elements whose a is non-zero must differ, in at least 10 % of those, from each
of the fused fp32(a * G + R), the add before the multiply, and a rounded to 16
bits first; RELU and RELU2 must differ from NONE in at least 25 % of all
elements.  A smaller case cannot meet a share on its own: build() returns its
counts and test_ex_fuzz_ref.py applies the same thresholds to its group's pool.
Every expectation is finite, also after the cast.  No case is redrawn or
dropped; the draw is a pure function of the case's seed.

The cases: DIRECTED, a named list of the smallest shapes that reach each
mechanism (thresholds restated next to test_gpu_call_fuzz's constants), then
PER_PAIR drawn cases for each (mode, family) pair from one default_rng(SEED)
stream."""
import collections
import functools
import itertools
import types

import numpy as np
import pytest

import test_gpu_actquant as A
import test_gpu_call_fuzz as CF
import test_gpu_epilogue as E
import test_gpu_normquant as NQ
from test_gpu_ldy import _assert_only_view_written, _fill
from test_gpu_scaled import _draw_scales, _got_bits, _outputs, _ybits_of, expect32
from test_gpu_xtype import _x_on_device
from test_gpu_ytype import YMAX, _assert_only_view_written16, _cast_bits, _fill16, torch_from_bits

pytestmark = pytest.mark.gpu

F = np.float32
SEED = 2028
PER_PAIR = 4

MODES = ("plain", "act", "norm")
QUANT = {"plain": None, "act": "act", "norm": "norm"}
FAMILIES = CF.FAMILIES
PAIRS = [(m, f) for m in MODES for f in FAMILIES]
KERNEL = CF.KERNEL
XDTYPES, YDTYPES, ACTS = CF.XDTYPES, CF.YDTYPES, E.ACTS
OPTYPES = (None,) + YDTYPES
TRIPLES = list(itertools.product(YDTYPES, YDTYPES, YDTYPES))  # (multype, addtype, ytype)
C0S = CF.C0S
PADS = CF.PADS + ("oa",)  # "oa": an odd row stride whose row 1 starts on 16 bytes (vec-pattern's ninth layout)
ESIZE = {"float32": 4, "float16": 2, "bfloat16": 2}
# vec-pattern: one letter each for Y, mul and add.  a: every row starts on 16 bytes; o: every row one
# element past; s: row 1 on 16 bytes and an odd row stride, the rows alternate
VEC_LAYOUTS = tuple("".join(p) for p in itertools.product("ao", repeat=3)) + ("s",)
VEC_SHAPES = [("rows64", 128, 65, 128), ("rows64", 16, 65, 128), ("rows128", 64, 130, 512), ("rx", 0, 130, 256)]
SMALL = 200   # fewer elements than this: the case's shares are pooled over its group

Case = collections.namedtuple(
    "Case", "name mode family M K N s w xdtype ydtype xoff act multype addtype inplace yform yc0 ypad mc0 mpad ac0 apad "
            "rs cs rs_out gamma eps smode width knob B vec seed")


@pytest.fixture(autouse=True)
def _oracle_built(oracle_mod):
    """The cached cases below import the oracle themselves: it is built first."""


def xdtypes_of(mode):
    return XDTYPES if mode == "plain" else XDTYPES[:3]


def pad_of(c0, N, pad):
    if pad == "m8":
        return (-(c0 + N)) % 8
    if pad == "oa":  # (ld + c0) a multiple of 8 elements and ld odd: c0 must be odd
        p = (-(2 * c0 + N)) % 8
        assert (c0 + N + p) % 2 == 1, (c0, N, "no odd stride with an aligned row 1")
        return p
    return pad


def ld_of(c0, N, pad):
    return c0 + N + pad_of(c0, N, pad)


def odd_pad(c0, N, least=0):
    """The smallest pad >= least that makes the row stride odd."""
    return least + (c0 + N + least + 1) % 2


_VEC_PLACE = {"a": (8, "m8"), "o": (1, "m8"), "s": (1, "oa")}


def _mk(name, mode, family, M, K, N, seed, s=4, w="rand", xdtype="float32", ydtype="float32", xoff=0, act="relu2",
        multype=None, addtype=None, inplace=None, yform="box", yplace=(1, 1), mplace=(2, 3), aplace=(2, 4), rs=False,
        cs=True, rs_out=None, gamma=None, eps=None, smode=None, width=0, knob=None, B=0, vec=None):
    """A Case with the fields a mode or family does not have at their neutral
    value, so that equal cases are equal tuples."""
    quant, norm = mode != "plain", mode == "norm"
    g = CF._mk(name, "scaled", family, M, K, N, seed, mode=smode, width=width, knob=knob, B=B)
    if inplace:  # the operand is Y: its type and its placement are Y's
        multype, addtype = (ydtype, addtype) if inplace == "mul" else (multype, ydtype)
        assert yform in ("odd", "aligned")
        yplace = (1, 2) if yform == "odd" else (0, (N + 7) // 8 * 8 + 8 - N)  # (test_gpu_epilogue.inplace_outputs)
    else:
        yform = "box"
    mplace = yplace if inplace == "mul" else mplace if multype else (0, 0)
    aplace = yplace if inplace == "add" else aplace if addtype else (0, 0)
    return Case(name, mode, family, M, K, N, s, w, xdtype, ydtype, xoff, act, multype, addtype, inplace, yform,
                *yplace, *mplace, *aplace, bool(rs) and not quant, bool(cs) or quant,
                bool(rs_out if rs_out is not None else quant) and quant, (gamma or "own") if norm else "none",
                (eps or 1e-5) if norm else 0.0, g.mode, g.width, g.knob, g.B, vec, seed)


def as_call_case(c):
    """The test_gpu_call_fuzz Case of the same X, W and handle: its builders and
    its _handle are reused as they are."""
    kind = {"act": "actquant", "norm": "normquant"}.get(c.mode, "scaled" if c.rs or c.cs else "typed")
    return CF._mk(c.name, kind, c.family, c.M, c.K, c.N, c.seed, s=c.s, w=c.w, xdtype=c.xdtype, ydtype=c.ydtype,
                  xoff=c.xoff, c0=0, pad=0, prelu=False, rs=c.rs, cs=c.cs, rs_out=c.rs_out, gamma=c.gamma, eps=c.eps,
                  mode=c.smode, width=c.width, knob=c.knob, B=c.B)


# ---- the directed cases --------------------------------------------------------------------

# the handles of the in-place group: (family, M, extra)
_INPLACE_HANDLES = [("pc", 2, {}), ("walk", 16, {}), ("rows64", 65, {}), ("rows64", 65, dict(knob="TSG_JIT_HALF")),
                    ("rows64", 65, dict(knob="TSG_JIT_PAIR")), ("rows64", 65, dict(knob="TSG_JIT_QBLOCK=16")),
                    ("rows128", 130, {}), ("rx", 70, {}), ("blocked", 70, dict(B=16)), ("blocked", 70, dict(B=64))]


def directed_cases():
    out = []

    def add(name, mode, family, M, K, N, **kw):
        out.append(_mk(name, mode, family, M, K, N, 1000 + len(out), **kw))

    y16 = ("float16", "bfloat16")
    # 1. a walk with K above its tile's LDS chunk (test_gpu_call_fuzz's four shapes) with relu2 and
    #    both operands in every mode; one case per shape in place
    for i, (M, K, N, smode) in enumerate([(16, 5120, 40, 2), (32, 5117, 40, 2), (3, 10240, 40, 3), (1, 41000, 24, 3)]):
        for j, mode in enumerate(MODES):
            x = ("int8", "float16")[i % 2] if mode == "plain" else ("bfloat16", "float16", "float32")[(i + j) % 3]
            inplace = ("add", "mul")[i % 2] if j == i % 3 else None
            add("chunked-walk-epi", mode, "walk", M, K, N, smode=smode, xdtype=x, ydtype=y16[(i + j) % 2],
                multype=OPTYPES[1 + (i + j) % 3], addtype=OPTYPES[1 + (i + 2 * j + 1) % 3], inplace=inplace,
                yform=("odd", "aligned")[i % 2], yplace=(i % 2, (1, 3)[j % 2]), gamma=("own", "slice")[i % 2])
    # 2. N below one store group (8), below one ELL slice (16) and one past each: the loaders'
    #    element-wise path with fewer than 8 valid columns, on every family
    for i, N in enumerate((1, 7, 9, 17)):
        for j, family in enumerate(FAMILIES):
            M, K, extra = CF._FAMILY_SHAPE[family]
            add("small-n-epi", MODES[(i + j) % 3], family, M, K, N, act=ACTS[(i + 2 * j) % 4], ydtype=y16[(i + j // 2) % 2],
                multype=y16[(i + j) % 2], addtype=y16[(i + j // 3) % 2], xdtype=XDTYPES[(i + j) % 3],
                yplace=((i + j) % 2, (0, 1, 3, "m8")[(i + 2 * j) % 4]), mplace=((j + 1) % 2, (1, 3)[i % 2]),
                aplace=(i % 3, ("m8", 0)[j % 2]), **extra)
    # 3. whole-segment views: the three alignment decisions of the epilogue's store, every combination,
    #    and an aligned row 1 with an odd stride on one operand
    n = 0
    for fi, (family, width, M, N0) in enumerate(VEC_SHAPES):
        for e in (0, 1):
            N = N0 + 8 * e
            for li, lay in enumerate(VEC_LAYOUTS):
                letters = lay if lay != "s" else ("asa", "aas")[(fi + e) % 2]
                mt, at, yt = TRIPLES[n % 27]
                add("vec-pattern", MODES[n % 3], family, M, 193, N, width=width, act=ACTS[(3 + n) % 4], ydtype=yt,
                    multype=mt, addtype=at, xdtype=XDTYPES[n % 3], yplace=_VEC_PLACE[letters[0]],
                    mplace=_VEC_PLACE[letters[1]], aplace=_VEC_PLACE[letters[2]], vec=letters)
                n += 1
    # 4. in place: add = Y and mul = Y in every mode on every handle; the types go round, Y is
    #    once the odd view and once the aligned dense view of test_gpu_epilogue.inplace_outputs
    for hi, (family, M, extra) in enumerate(_INPLACE_HANDLES):
        K = 200 if family == "blocked" else 193
        for mi, mode in enumerate(MODES):
            for fi, form in enumerate(("add", "mul")):
                yt = YDTYPES[(hi + mi) % 3]
                other = YDTYPES[(hi + mi + 1 + fi) % 3]
                add("in-place", mode, family, M, K, 130, inplace=form, yform=("odd", "aligned")[(hi + mi + fi) % 2],
                    ydtype=yt, multype=other, addtype=other, xdtype=XDTYPES[(hi + fi) % 3], **extra)
    # 5. operands with odd row strides of their own past two M tiles; the walk on the int8 copy
    #    over many M tiles
    shapes = [("rows64", dict(width=16)), ("rows128", {}), ("rx", {})]
    for i, M in enumerate((257, 300)):
        for j, (family, extra) in enumerate(shapes):
            add("many-m-tiles", ("act", "norm")[(i + j) % 2], family, M, 193, 130, rs_out=True, ydtype=YDTYPES[(i + j) % 3],
                multype=YDTYPES[(i + j + 1) % 3], addtype=YDTYPES[(i + j + 2) % 3], xdtype=XDTYPES[(i + j) % 3],
                yplace=(1, odd_pad(1, 130)), mplace=(2, odd_pad(2, 130, 2)), aplace=(1, odd_pad(1, 130, 6)), **extra)
    add("many-m-tiles", "act", "walk", 300, 388, 130, smode=2, rs_out=True, ydtype="bfloat16", multype="float16",
        addtype="float32", yplace=(1, odd_pad(1, 130)), mplace=(2, odd_pad(2, 130, 2)), aplace=(1, odd_pad(1, 130, 6)))
    # 6. an all-zero W with K > 0 (Y is the epilogue of b alone), a W with an empty column, a dense W
    for wi, (w, s) in enumerate((("zero", 4), ("rand", 64), ("rand", 1))):
        for mi, mode in enumerate(("act", "plain")):
            for fi, family in enumerate(("walk", "rows64")):
                add("unusual-w-epi", mode, family, 16 if family == "walk" else 65, 193, 130, w=w, s=s, width=16,
                    act=ACTS[1 + (wi + mi + fi) % 3], ydtype=YDTYPES[(wi + mi + fi) % 3], multype=YDTYPES[(wi + fi) % 3],
                    addtype=YDTYPES[(mi + fi + 1) % 3])
    # 7. X two and three elements into a larger buffer, with one operand
    for mode, xs in (("plain", ("float16", "bfloat16", "int8")), ("act", ("float16",)), ("norm", ("bfloat16",))):
        for i, xdtype in enumerate(xs):
            for xoff in (2, 3):
                family = ("walk", "rows64")[(i + xoff) % 2]
                op = dict(multype=YDTYPES[(i + xoff) % 3]) if (i + xoff) % 2 else dict(addtype=YDTYPES[(i + xoff) % 3])
                add("x-offset-epi", mode, family, 16 if family == "walk" else 65, 388, 130, xoff=xoff, xdtype=xdtype,
                    width=16, ydtype=YDTYPES[(i + xoff + 1) % 3], act=ACTS[(i + xoff) % 4], **op)
    for mode, xdtype in (("act", "bfloat16"), ("norm", "float16")):  # (both 16-bit types in both quantising modes)
        for xoff in (2, 3):
            family = ("rows64", "walk")[xoff % 2]
            add("x-offset-epi", mode, family, 16 if family == "walk" else 65, 388, 130, xoff=xoff, xdtype=xdtype, width=16,
                ydtype=YDTYPES[xoff % 3], act="relu", addtype="bfloat16")
    return out


# ---- the drawn cases --------------------------------------------------------------------------

def drawn_cases(counter=None):
    """PER_PAIR cases per (mode, family) pair from one stream.  The X and Y
    types, the 64-row image's width and knob, the 128-row image's width and a
    blocked handle's B go round their lists; everything else is drawn.
    counter, a list, receives one entry per case drawn."""
    rng = np.random.default_rng(SEED)
    out = []
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    for mi, mode in enumerate(MODES):
        combos = list(itertools.product(xdtypes_of(mode), YDTYPES))
        for fi, family in enumerate(FAMILIES):
            for j in range(PER_PAIR):
                i = fi * PER_PAIR + j
                xdtype, ydtype = combos[i % len(combos)]
                N = int(rng.integers(1, 1301)) if rng.random() < CF.OFF_POOL else pick(CF.N_POOL)
                K = int(rng.integers(1, 3001)) if rng.random() < CF.OFF_POOL else pick(CF.K_POOL)
                B = (16, 64)[j % 2] if family == "blocked" else 0
                K = max(K, B)
                # the 1-row producer/consumer tiles take M <= 4; the walk stays at M <= 32 unless N <= 512
                top = 4 if family == "pc" else 33 if family == "walk" and N > 512 else CF.M_POOL[-1]
                M = pick([m for m in CF.M_POOL if m <= top])
                smode = 0 if family == "pc" else 1
                if family == "walk":
                    smode = 3 if M <= 4 else pick((0, 2, 3)) if M <= CF.ELL_MID_M else pick((2, 3))
                width, knob = CF._ROWS64_SHAPES[mi * PER_PAIR + j] if family == "rows64" else (0, None)
                if family == "rows128":
                    width = CF._ROWS128_WIDTHS[mi * PER_PAIR + j]
                act, mt, at = pick(ACTS), pick(OPTYPES), pick(OPTYPES)
                places = [(pick(C0S), pick(CF.PADS)) for _ in range(3)]
                inplace, yform = pick((None, None, "add", "mul")), pick(("odd", "aligned"))
                scales = pick(("both", "row", "col", "none"))
                s, xoff, rs_out = pick(CF.SPARS), int(rng.integers(0, 4)), rng.random() < 0.75
                gamma, eps = pick(("none", "own", "slice")), pick((1e-5, 1e-6))
                if mt is None and at is None and act in ("none", "prelu"):
                    at = "bfloat16"  # (a descriptor without an epilogue is test 3 of test_gpu_epilogue.py)
                if {"mul": mt, "add": at}.get(inplace) != ydtype:
                    inplace = None   # in place only where the types allow it
                if mode == "plain" and scales == "none":
                    if ydtype == "float16":
                        scales = "col"  # (the chain's magnitudes do not fit an fp16 Y)
                    else:               # the _xy restatement: fp32 or bf16, no square
                        mt, at = (t if t != "float16" else "bfloat16" for t in (mt, at))
                        act = "relu" if act == "relu2" else act
                out.append(_mk("drawn", mode, family, M, K, N, 5000 + len(out), s=s, xdtype=xdtype, ydtype=ydtype, xoff=xoff,
                               act=act, multype=mt, addtype=at, inplace=inplace, yform=yform, yplace=places[0],
                               mplace=places[1], aplace=places[2], rs=scales in ("both", "row"),
                               cs=scales in ("both", "col"), rs_out=rs_out, gamma=gamma, eps=eps, smode=smode, width=width,
                               knob=knob, B=B))
                if counter is not None:
                    counter.append(out[-1].seed)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(directed_cases() + drawn_cases())


def case_id(c):
    return f"{c.seed}-{c.name}-{c.mode}-{c.family}-{c.M}x{c.K}x{c.N}"


# ---- the case builder ------------------------------------------------------------------------------

def _count(x, y, where=None):
    d = x.view(np.uint32) != y.view(np.uint32)
    return (int(d.sum()), d.size) if where is None else (int(d[where].sum()), int(where.sum()))


def share_ok(name, differ, total):
    return differ >= (0.25 if name == "relu" else 0.10) * total


@functools.lru_cache(maxsize=None)
def build(c):
    """One case's inputs, operands and expectation, computed once, never
    modified; the module docstring's input conditions are asserted here."""
    import oracle as O
    import tspgemm as T
    M, K, N = c.M, c.K, c.N
    g_ = as_call_case(c)
    quant = c.mode != "plain"
    assert c.mode in MODES and c.family in FAMILIES and c.s in CF.SPARS and c.xdtype in xdtypes_of(c.mode), c
    assert c.act in ACTS and c.multype in OPTYPES and c.addtype in OPTYPES and c.ydtype in YDTYPES, c
    assert M >= 1 and K >= max(1, c.B) and N >= 1 and 0 <= c.xoff <= 3, c
    assert c.multype or c.addtype or c.act in ("relu", "relu2"), (c, "the case has no epilogue")
    assert (c.cs or not quant) and not (c.rs and quant) and (c.rs_out <= quant), c
    if not (c.rs or c.cs):  # the _xy restatement keeps the chain's magnitudes
        assert not quant and c.act != "relu2" and "float16" not in (c.ydtype, c.multype, c.addtype), c
    if c.family == "pc":  # what the planner asks of the 1-row producer/consumer tiles
        assert c.smode == 0 and M <= 4 and M * N <= CF.ELL_PC_MAX_MN and K <= CF.ELL_MAX_C[0], c
    # the three placements
    lds = {}
    for name, t, c0, pad in (("Y", c.ydtype, c.yc0, c.ypad), ("mul", c.multype, c.mc0, c.mpad),
                             ("add", c.addtype, c.ac0, c.apad)):
        if t:
            assert c0 >= 0 and pad in PADS + tuple(range(17)) and pad_of(c0, N, pad) >= 0, (c, name)
            lds[name] = ld_of(c0, N, pad)
    if c.inplace:
        op = c.inplace
        assert (c.multype if op == "mul" else c.addtype) == c.ydtype and lds[op] == lds["Y"], (c, "in place")
        assert (c.mc0, c.mpad) == (c.yc0, c.ypad) if op == "mul" else (c.ac0, c.apad) == (c.yc0, c.ypad), c
    if c.vec:  # every row of the view (rows 1 .. M of its buffer) as the letter says, by construction
        assert N % 8 == 0 and c.multype and c.addtype and not c.inplace, c
        for letter, name, t, c0 in zip(c.vec, ("Y", "mul", "add"), (c.ydtype, c.multype, c.addtype),
                                       (c.yc0, c.mc0, c.ac0)):
            first, step = (lds[name] + c0) * ESIZE[t], lds[name] * ESIZE[t]
            if letter == "a":
                assert first % 16 == 0 and step % 16 == 0, (c, name)
            elif letter == "o":
                assert first % 16 == ESIZE[t] and step % 16 == 0, (c, name)
            else:
                assert first % 16 == 0 and lds[name] % 2 == 1, (c, name)
    if c.name == "many-m-tiles":
        assert M > 256 and len(set(lds.values())) == 3 and all(v % 2 for v in lds.values()) and c.rs_out, (c, lds)

    klast = K // c.B * c.B - 1 if c.B else K - 1
    W = CF._make_w(g_, klast)
    zeros = np.zeros(N, F)
    if c.B:
        arrays = O.blocked_tcsc_encode(W, c.B)
        run = lambda Xc: O.base_blocked_tcsc(Xc, arrays, zeros, K, N, c.B)
    else:
        t = O.tcsc_encode(W)
        arrays = t.arrays
        run = lambda Xc: O.base_tcsc(Xc, t, zeros, threads=8 if Xc.shape[0] >= 8 else 0)
    b = np.linspace(-3, 3, N).astype(F)
    alpha = np.linspace(-0.5, 0.5, N).astype(F)
    rs, cs = _draw_scales(M, N, 0, c.seed)
    g = NQ._gamma(K) if c.gamma != "none" else None
    Xt, Xw = CF._make_x(g_, 0, klast)

    def chain_of(Xw_):
        """(the oracle's chain, deq) -- X through the mode's front end."""
        Xc, deq = Xw_, None
        if c.mode == "norm":
            Xc = T.rms_norm_ref(Xc, g, c.eps)[0]
        if quant:
            q, deq = T.act_quant_ref(Xc)
            Xc = q.astype(F)
        chain = run(Xc)
        assert np.isfinite(chain).all() and not np.signbit(chain[chain == 0]).any()
        return chain, deq

    chain, deq = chain_of(Xw)
    # the magnitude: the exact power of two that brings the largest |chain * rs * cs| under 2^6
    e = 0
    if c.rs or c.cs:
        r0 = deq if quant else rs if c.rs else None
        top = float(np.abs(expect32(chain, r0, cs if c.cs else None, zeros)).max())
        e = int(np.ceil(np.log2(top))) - 6 if top > 0 else 0
        scaled = ((cs if c.cs else rs).astype(np.float64) * 2.0 ** -e).astype(F)
        assert np.array_equal(scaled.astype(np.float64) * 2.0 ** e, (cs if c.cs else rs).astype(np.float64)), (c, e)
        cs, rs = (scaled, rs) if c.cs else (cs, scaled)

    def y_of(chain_, deq_, rows=slice(None)):
        r = deq_ if quant else rs[rows] if c.rs else None
        return expect32(chain_, r, cs if c.cs else None, b)

    y32 = y_of(chain, deq)
    assert np.isfinite(y32).all(), (c, "y is not finite")
    if c.rs or c.cs:
        assert float(np.abs(y32).max()) <= 2.0 ** 6 + 3, (c, float(np.abs(y32).max()))

    # the operands (test_gpu_epilogue.expect's recipe) and the expectation
    al = alpha if c.act == "prelu" else None
    rng = np.random.default_rng(c.seed + 31)
    a = T.epilogue_ref(y32, c.act, al)
    Gt = Gw = Rt = Rw = None
    if c.multype:
        G = (rng.uniform(0.5, 2.0, a.shape) * rng.choice([-1.0, 1.0], a.shape)).astype(F)
        Gt, Gw = E._round_to(G, c.multype)
    if c.addtype:
        p = np.abs(a.astype(np.float64) * (Gw if c.multype else 1.0))
        R = (rng.uniform(-1.0, 1.0, a.shape) * 2.0 ** np.ceil(np.log2(np.where(p > 0, p, 1.0)))).astype(F)
        Rt, Rw = E._round_to(R, c.addtype)
    want32 = T.epilogue_ref(y32, c.act, al, Gw, Rw)
    assert np.isfinite(want32).all(), (c, "the expectation is not finite")
    if c.ydtype != "float32":
        assert float(np.abs(want32).max()) <= YMAX[c.ydtype], (c, "the expectation overflows the Y type")
    want = _ybits_of(want32, c.ydtype)
    if c.ydtype != "float32":
        assert np.array_equal(want, _cast_bits(want32, c.ydtype)) and np.isfinite(torch_from_bits(want, c.ydtype)).all()

    # the discrimination conditions: (differing, of) per name; asserted here where the case is
    # large enough, pooled over the group by test_ex_fuzz_ref.py where it is not
    shares, pooled = {}, {}
    if c.act in ("relu", "relu2"):
        shares["relu"] = _count(a, y32)
    if c.multype and c.addtype:
        nz = a != 0
        d64 = np.float64
        t16 = c.multype if c.multype != "float32" else "bfloat16"
        shares["fused"] = _count((a.astype(d64) * Gw.astype(d64) + Rw.astype(d64)).astype(F), want32, nz)
        shares["add before multiply"] = _count(((a + Rw).astype(F) * Gw).astype(F), want32, nz)
        shares["a rounded to 16 bits first"] = _count(((E._round_to(a, t16)[1] * Gw).astype(F) + Rw).astype(F), want32, nz)
    for name, (differ, total) in shares.items():
        if total >= SMALL:
            assert share_ok(name, differ, total), (c, name, "is told apart from the contract in only", differ, "of", total)
        else:
            pooled[name] = (differ, total)

    if c.w == "zero":  # Y is the epilogue of b alone
        assert not W.any() and K > 0
        flat = np.ascontiguousarray(np.broadcast_to(b, (M, N)), F)
        assert np.array_equal(want, _ybits_of(T.epilogue_ref(flat, c.act, al, Gw, Rw), c.ydtype)), c
    else:
        assert W[0].any() and W[klast].any() and W[:, 0].any() and W[:, N - 1].any(), c
        ordinary = CF._ordinary_rows(g_)
        assert (Xw[ordinary][:, [0, klast]] != 0).all(), (c, "X is zero at an end of a row")
        head = slice(0, min(M, 8))  # (rows are independent: a change in these rows is a change)
        X2 = Xw[head].copy()
        X2[:, klast] = 0
        assert not np.array_equal(y_of(*chain_of(X2), head), y32[head]), (c, "X[:, K - 1] does not reach y")
        nch, k_last_chunk = CF.walk_chunks(g_)
        if nch > 1:
            assert CF.walk_tile(M, K) != 2, (c, "the 8-row tile's chunk depends on its image")
            X3 = Xw[head].copy()
            X3[:, k_last_chunk:] = 0
            assert 0 < k_last_chunk < K and not np.array_equal(y_of(*chain_of(X3), head), y32[head]), \
                (c, "the last chunk does not reach y")
        if M >= 2:
            assert not np.array_equal(want[M - 1], want[M - 2]), (c, "rows M - 1 and M - 2 agree")
        if c.name == "unusual-w-epi" and c.s == 64:
            assert (np.abs(W).sum(axis=0) == 0).any(), (c, "no column of W is empty")
    if c.mode == "act":  # the row maximum is where the recipe put it: the quantisation has an edge to lose
        assert np.abs(T.act_quant_ref(Xw)[0]).max() == 127
    for arr in (Xw, b, alpha, rs, cs, y32, want32, want):
        arr.setflags(write=False)
    return types.SimpleNamespace(arrays=arrays, Xt=Xt, Xw=Xw, b=b, alpha=alpha, rs=rs if c.rs else None,
                                 cs=cs if c.cs else None, g=g, deq=deq, y32=y32, Gt=Gt, Gw=Gw, Rt=Rt, Rw=Rw, want32=want32,
                                 want=want, e=e, lds=lds, pooled=pooled, nnz=int(np.count_nonzero(W)))


# ---- the GPU check ---------------------------------------------------------------------------------

def _assert_vec(c, letter, name, t):
    ptr, es = t.data_ptr(), t.element_size()
    if letter == "a":
        assert ptr % 16 == 0 and t.stride(0) * es % 16 == 0, (c, name, ptr % 16, t.stride(0))
    elif letter == "o":
        assert ptr % 16 == es and t.stride(0) * es % 16 == 0, (c, name, ptr % 16, t.stride(0))
    else:
        assert ptr % 16 == 0 and t.stride(0) % 2 == 1, (c, name, ptr % 16, t.stride(0))


@pytest.mark.parametrize("c", cases(), ids=case_id)
def test_ex_fuzz(tsg, monkeypatch, c):
    import torch
    for k in CF.KNOBS:
        monkeypatch.delenv(k, raising=False)
    if c.family == "rx":
        monkeypatch.setenv("TSG_KERNEL", "rx")
    if c.knob:
        name, _, value = c.knob.partition("=")
        monkeypatch.setenv(name, value or "1")
    bc = build(c)
    M, N, K = c.M, c.N, c.K
    h = CF._handle(tsg, as_call_case(c), bc.arrays)
    Xd = _x_on_device(bc.Xt, c.xoff)
    assert Xd.data_ptr() % (4 * Xd.element_size()) == c.xoff * Xd.element_size()
    gbuf, gd = NQ._gamma_dev(bc.g, K, c.gamma == "slice")
    inp = E.Inputs(bc, X=Xd, extra=[("gamma", gbuf)])
    # Y: the sentinel box, or for a case in place the odd / the aligned view of inplace_outputs
    if c.inplace:
        buf, view, box = E.inplace_outputs(M, N, c.ydtype)[c.yform]
        fill, only = (_fill, _assert_only_view_written) if c.ydtype == "float32" else (_fill16, _assert_only_view_written16)
        assert c.yform == "odd" or view.data_ptr() % 16 == 0
    else:
        (buf, view, box, fill, only), = _outputs(M, N, c.ydtype, c0=c.yc0, pad=pad_of(c.yc0, N, c.ypad)).values()
    assert tuple(view.shape) == (M, N) and (M == 1 or view.stride(0) == bc.lds["Y"]), (c, view.stride())
    fill(buf)
    mbuf, mview = E.place(bc.Gt, c.mc0, pad_of(c.mc0, N, c.mpad)) if c.inplace != "mul" else (None, view)
    abuf, aview = E.place(bc.Rt, c.ac0, pad_of(c.ac0, N, c.apad)) if c.inplace != "add" else (None, view)
    if c.inplace:
        view.copy_((bc.Gt if c.inplace == "mul" else bc.Rt).cuda())
    for name, t in (("mul", mview), ("add", aview)):
        assert t is None or M == 1 or t.stride(0) == bc.lds[name], (c, name, t.stride())
    if c.vec:
        for letter, name, t in zip(c.vec, ("Y", "mul", "add"), (view, mview, aview)):
            _assert_vec(c, letter, name, t)
    keep = [None if t is None else t.clone() for t in (mbuf, abuf)]
    rbuf, rd_out = A._scale_out(M) if c.rs_out else (None, None)
    out = h.gemm_torch_ex(Xd, inp.b, view, act=c.act, alpha=inp.alpha if c.act == "prelu" else None, mul=mview, add=aview,
                          row_scale=inp.rs, col_scale=inp.cs, quant=QUANT[c.mode], gamma=gd,
                          eps=c.eps if c.mode == "norm" else None, row_scale_out=rd_out)
    torch.cuda.synchronize()
    assert out is view
    CF.assert_bits(_got_bits(view, c.ydtype), bc.want, c, "descriptor")
    only(buf, *box, tuple(c))
    for t, k, n in zip((mbuf, abuf), keep, ("mul", "add")):
        assert t is None or E.same_bytes(t, k), (tuple(c), n, "buffer was written")
    if c.rs_out:
        A._assert_scale_out(rbuf, M, bc.deq, tuple(c))
    inp.assert_unchanged(tuple(c))
    h.close()
