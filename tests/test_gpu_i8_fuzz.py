"""Seeded shape, mode and layout fuzz over the four integer matrix-core kernels
(tsg_i8mfma_kernel, tsg_i8gemv_kernel, tsg_i8glu_kernel, tsg_i8glu_gemv_kernel)
as fuzz families of their own, then structured W and isolation through the same
kernels.  test_gpu_i8mfma.py, test_gpu_i8gemv.py and test_gpu_glu.py pin these
kernels on short hand-picked lists over one dense uniform W; test_gpu_ex_fuzz.py
is pinned to the add streams.  This file gives the integer kernels what the add
streams have: directed cases at every boundary of their tilings, drawn cases,
every operand type, in-place operands, odd and aligned views, unusual W.

The families.  i8mfma and glu_tile are the 128-row tile kernels (at M <= 32 under
set_i8_small(1), where most of a tile's rows are padding); i8gemv and glu_gemv
the split-K kernels (M <= 32).  Every handle is pinned with set_i8_mfma(2); a case
asserts call_i8_kernel(M) (1 or 2) and, for split-K, i8gemv_pick / i8glu_pick
against the tile columns and waves restated here.

The reference.  Compared as integers, no tolerance.  The chain is numpy's int64
product q @ W (asserted |chain| <= 2^24); then the contract's fp32 steps one
rounding per line (test_gpu_i8mfma._ref), tspgemm.epilogue_ref and
test_gpu_ytype._cast_bits; for GLU test_gpu_glu._want.  In the quantising modes q
and deq are tspgemm.act_quant_ref's (after tspgemm.rms_norm_ref for norm) and
row_scale_out must hold deq bit for bit.  A plain-TCSC family case also runs the
same call under set_i8_mfma(1), the add streams; a GLU case without a mul of its
own is, one case in four, also compared with the two-call sequence.

After each call: every element of the Y view, every element of Y's buffer outside
the view still the sentinel, the operands' buffers byte-identical (an in-place
operand is Y), row_scale_out's surroundings untouched, and X, b, b_up, alpha, both
column scales, the row scale and gamma byte-identical.

Inputs (build() asserts all of this on the CPU; test_i8_fuzz_ref.py runs it for
every case).  X, W and gamma are test_gpu_call_fuzz's builders'; b = linspace(-3,
3, N), b_up = linspace(0.5, -0.25, N) with every other sign flipped (u has both
signs next to either sign of y however sparse W is).  W is nonzero in rows 0 and K - 1 and in
columns 0 and N - 1, zeroing X[:, K - 1] changes y, rows M - 1 and M - 2 of the
expectation differ.  Magnitude: a scaled case carries an exact power of two in
its column scale (a PLAIN case with the row scale only: there) so that |y| <=
2^6 + 3, and a GLU case with col_scale_up one there so that |u| <= 2 + 0.5: relu2,
the up product, the mul product and the residual sum then stay finite in fp16.  A
case that lacks one of these scales keeps the chain's magnitudes and has fp32 or
bf16 Y and operands and no relu2.  The operands are test_gpu_epilogue.expect's
recipe.  Shares (test_gpu_ex_fuzz's thresholds, pooled over a group's cases below
SMALL elements by the CPU twin): with both operands the expectation differs in at
least 10 % of the elements whose a is nonzero from the fused multiply-add, the
add before the multiply and a rounded to 16 bits first; relu and relu2 differ
from none in at least 25 %.  GLU adds two: with the gate and up images swapped
the expectation changes in at least 10 % of its elements, and act(y) * u differs
from act(y * u) in at least 10 % of the elements where y < 0 (under act none y * u
is symmetric and neither difference exists: both hold for the other three
activations, which are the asymmetric ones).  Every expectation is
finite, also after the cast.  No case is skipped or redrawn; the draw is a pure
function of the case's seed."""
import collections
import functools
import itertools
import types

import numpy as np
import pytest

import test_gpu_actquant as A
import test_gpu_call_fuzz as CF
import test_gpu_epilogue as E
import test_gpu_ex_fuzz as XF
import test_gpu_glu as GL
import test_gpu_i8mfma as I8
import test_gpu_normquant as NQ
from test_gpu_ldy import _assert_only_view_written, _dev, _fill
from test_gpu_scaled import _draw_scales, _got_bits, _outputs, _ybits_of
from test_gpu_wstruct import FAMILY_NAMES, families
from test_gpu_xtype import _x_on_device
from test_gpu_ytype import YMAX, _assert_only_view_written16, _cast_bits, _fill16, torch_from_bits

pytestmark = pytest.mark.gpu

F = np.float32
SEED = 2029
PER_PAIR = 6
SMALL = 200

# tsg_internal.h
I8_TILE_M = I8_TILE_N = 128   # kI8TileM, kI8TileN
I8_WAVE_N = 64                # kI8WaveN
I8_KSTEP = 64                 # kI8KStep
I8_GEMV_MAX_M = 32            # kI8GemvMaxM
I8_GEMV_CUS = 256             # kI8GemvCUs: tn = 64 from N / 64 >= 256 on
GEMV_CAP = {32: 16, 64: 8}    # kI8GemvWaves32, kI8GemvWaves64
GLU_CAP = 8                   # kI8GluWaves

MODES = XF.MODES
FAMILIES = ("i8mfma", "i8gemv", "glu_tile", "glu_gemv")
GLU = ("glu_tile", "glu_gemv")
SPLITK = ("i8gemv", "glu_gemv")
PAIRS = [(m, f) for m in MODES for f in FAMILIES]
YDTYPES, ACTS, OPTYPES, TRIPLES = XF.YDTYPES, XF.ACTS, XF.OPTYPES, XF.TRIPLES
QX = CF.XDTYPES[:3]           # X types of the quantising modes
WS = ("rand", "zero", "zero_up", "zero_gate", "emptycol", "signcols")

Case = collections.namedtuple(
    "Case", "name mode family M K N s w xdtype xoff ydtype act multype addtype inplace yform yc0 ypad mc0 mpad ac0 apad "
            "rs cs csu rs_out gamma eps cross seed")


@pytest.fixture(autouse=True)
def _oracle_built(oracle_mod):
    """The cached cases below import the oracle themselves: it is built first."""


def gemv_pick(K, N):
    """(tile columns, waves): i8gemv_pick of tsg_internal.h restated."""
    tn = 64 if N // I8_WAVE_N >= I8_GEMV_CUS else 32
    nks, S = -(-K // I8_KSTEP), 1
    while 2 * S <= GEMV_CAP[tn] and 2 * S <= nks:
        S *= 2
    return tn, S


def glu_pick(K):
    nks, S = -(-K // I8_KSTEP), 1
    while 2 * S <= GLU_CAP and 2 * S <= nks:
        S *= 2
    return 32, S


def pick_of(c):
    return gemv_pick(c.K, c.N) if c.family == "i8gemv" else glu_pick(c.K) if c.family == "glu_gemv" else None


def wave_steps(K, S):
    """k-steps of each of the S waves: wave w takes steps w, w + S, ..."""
    nks = -(-K // I8_KSTEP)
    return [len(range(w, nks, S)) for w in range(S)]


def kernel_of(c):
    """What call_i8_kernel(M) must say: 2 the split-K kernel, 1 the tile kernel."""
    return 2 if c.family in SPLITK else 1


def _mk(name, mode, family, M, K, N, seed, s=2, w="rand", xdtype=None, xoff=0, ydtype="float32", act="relu2", multype=None,
        addtype=None, inplace=None, yform="box", yplace=(1, 1), mplace=(2, 3), aplace=(2, 4), rs=False, cs=True, csu=True,
        rs_out=None, gamma=None, eps=None, cross=None):
    quant, norm, glu = mode != "plain", mode == "norm", family in GLU
    if inplace:  # the operand is Y: its type and its placement are Y's
        multype, addtype = (ydtype, addtype) if inplace == "mul" else (multype, ydtype)
        assert yform in ("odd", "aligned")
        yplace = (1, 2) if yform == "odd" else (0, (N + 7) // 8 * 8 + 8 - N)
    else:
        yform = "box"
    mplace = yplace if inplace == "mul" else mplace if multype else (0, 0)
    aplace = yplace if inplace == "add" else aplace if addtype else (0, 0)
    if cross is None:  # one GLU case in four (those that the two-call sequence can state)
        cross = glu and multype is None and seed % 4 == 0
    return Case(name, mode, family, M, K, N, s, w, xdtype or ("float32" if quant else "int8"), xoff, ydtype, act, multype,
                addtype, inplace, yform, *yplace, *mplace, *aplace, bool(rs) and not quant, bool(cs) or quant,
                bool(csu) and glu, bool(rs_out if rs_out is not None else quant) and quant,
                (gamma or "own") if norm else "none", (eps or 1e-5) if norm else 0.0, bool(cross) and glu and multype is None,
                seed)


def unscaled(c):
    """The case keeps the chain's magnitudes somewhere: fp32 / bf16 only, no relu2."""
    return not (c.rs or c.cs) or (c.family in GLU and not c.csu)


# ---- the directed cases --------------------------------------------------------------------

TILE_MS = (63, 64, 65, 127, 128, 129)
TILE_NS = (31, 32, 33, 63, 64, 65, 127, 128, 129)
TILE_KS = (15, 16, 17, 63, 64, 65)
SMALL_MS = (1, 5, 32)
SPLIT_MS = (1, 3, 4, 5, 8, 9, 28, 29, 31, 32)
SPLIT_NS = (31, 32, 33, 63, 64, 65, 577)
# K -> what it is the smallest K for (S and steps per wave derive from the pick)
GEMV_KS = (64, 65, 128, 192, 256, 448, 512, 576, 1024, 1088, 1100, 3072)
GLU_KS = (64, 65, 128, 192, 256, 448, 512, 576, 1088, 1100, 1536)
ALIGN_KS = (208, 193, 207)    # K % 16 = 0, 1, 15
ALIGN_OFFS = (0, 1, 4, 15)


def _eshape(family):
    """The small shape a family runs in the epilogue, 16-byte and W groups: a ragged second tile each way."""
    return (9, 200, 40) if family in SPLITK else (65, 100, 70)


def directed_cases():
    out = []
    y16 = ("float16", "bfloat16")

    def add(name, mode, family, M, K, N, **kw):
        out.append(_mk(name, mode, family, M, K, N, 1000 + len(out), **kw))

    def places(i, N):
        """Y once at an odd offset with an odd ldY, once with ldY a multiple of 8."""
        return dict(yplace=(1, XF.odd_pad(1, N)) if i % 2 == 0 else ((0, 1, 4, 8)[i // 2 % 4], "m8"))

    # 1. the tile kernels: M, N and K below, at and one past a wave tile and a workgroup tile (the GLU
    #    tile is 64 columns wide with 32-column wave halves; a wave with nw >= N is dead); K = 16: one
    #    16-byte A load; three M tiles with a ragged last one; K = 0 and 1; M <= 32 under set_i8_small(1)
    for family in ("i8mfma", "glu_tile"):
        for i, M in enumerate(TILE_MS):
            for j, N in enumerate(TILE_NS):
                n = i * len(TILE_NS) + j
                add("tile-edge", MODES[n % 3], family, M, TILE_KS[(i + j) % 6], N, act=ACTS[n % 4], ydtype=YDTYPES[n % 3],
                    xdtype=QX[n % 3] if n % 3 else None, **places(n, N))
        for i, (M, K, N) in enumerate([(257, 193, 130), (257, 64, 65), (40, 0, 40), (129, 0, 65), (65, 1, 33), (130, 1, 129)]):
            add("tile-shape", "plain" if K == 0 else MODES[i % 3], family, M, K, N, act=ACTS[(1 + i) % 4],
                ydtype=YDTYPES[i % 3], addtype=YDTYPES[(i + 1) % 3], xdtype=QX[i % 3] if K and i % 3 else None)
        for i, M in enumerate(SMALL_MS):
            for j, (K, N) in enumerate(((200, 33), (64, 129), (17, 64))):
                n = i * 3 + j
                add("tile-small-m", MODES[n % 3], family, M, K, N, act=ACTS[n % 4], ydtype=YDTYPES[n % 3],
                    multype=YDTYPES[(n + 1) % 3], xdtype=QX[n % 3] if n % 3 else None, **places(n, N))
    # 2. the 16-byte rule of the A loads: K % 16 in {0, 1, 15} with X at byte offsets 0, 1, 4, 15 of a
    #    larger int8 buffer; a quantising call's X is the scratch: K only
    for family in FAMILIES:
        M, _, N = _eshape(family)
        for i, K in enumerate(ALIGN_KS):
            for j, off in enumerate(ALIGN_OFFS):
                add("x-16-bytes", "plain", family, M, K, N, xoff=off, act=ACTS[(i + j) % 4], ydtype=YDTYPES[(i + j) % 3])
            for j, mode in enumerate(("act", "norm")):
                add("x-16-bytes", mode, family, M, K, N, xdtype=QX[(i + j) % 3], act=ACTS[(i + j + 2) % 4],
                    ydtype=YDTYPES[(i + j + 1) % 3], gamma=("own", "slice")[i % 2])
    # 3. the split-K kernels: every S of the pick, k-steps equal to S and not divisible by it, waves
    #    with 1, 2 and 3 steps (the pipeline is two deep); every M around the register rows (register
    #    r holds rows 8 (r / 4) + r % 4 and 4 below); N around the 32-column tile and the granule, 577:
    #    10 granules padded to 16 (padding workgroups in the XCD numbering)
    for family, Ks in (("i8gemv", GEMV_KS), ("glu_gemv", GLU_KS)):
        for i, K in enumerate(Ks):
            add("split-k", MODES[i % 3], family, SPLIT_MS[i % 10], K, SPLIT_NS[i % 7], act=ACTS[i % 4],
                ydtype=YDTYPES[i % 3], addtype=YDTYPES[(i + 1) % 3], xdtype=QX[i % 3] if i % 3 else None, **places(i, SPLIT_NS[i % 7]))
        for i, M in enumerate(SPLIT_MS):
            add("split-m", MODES[(i + 1) % 3], family, M, (192, 200, 448)[i % 3], (33, 65, 130)[i % 3], act=ACTS[(i + 1) % 4],
                ydtype=YDTYPES[(i + 1) % 3], multype=YDTYPES[i % 3], xdtype=QX[i % 3] if (i + 1) % 3 else None,
                **places(i + 1, (33, 65, 130)[i % 3]))
        for i, N in enumerate(SPLIT_NS):
            add("split-n", MODES[(i + 2) % 3], family, (5, 32, 9)[i % 3], (200, 576)[i % 2], N, act=ACTS[(i + 2) % 4],
                ydtype=YDTYPES[(i + 2) % 3], multype=YDTYPES[i % 3], addtype=YDTYPES[(i + 1) % 3],
                xdtype=QX[i % 3] if (i + 2) % 3 else None, **places(i, N))
    # the 64-column tile of tsg_i8gemv_kernel (N / 64 >= 256), with an epilogue and a 16-bit Y
    for i, N in enumerate((16384, 16390)):
        add("split-tn64", "plain", "i8gemv", (32, 3)[i], 192, N, act=("relu2", "prelu")[i], ydtype=y16[i],
            multype=y16[1 - i], addtype=y16[i], yplace=((0, "m8"), (1, XF.odd_pad(1, N)))[i])
    # 4. the epilogue and the output side on all four kernels: the 27 type triples in rotation with the
    #    activations; add = Y and mul = Y in place; the scale combinations (without a scale: fp32 or
    #    bf16, no relu2); GLU: col_scale_up with and without col_scale
    for fi, family in enumerate(FAMILIES):
        M, K, N = _eshape(family)
        for n, (mt, at, yt) in enumerate(TRIPLES):
            add("triples", MODES[(n + fi) % 3], family, M, K, N, act=ACTS[(n + fi) % 4], multype=mt, addtype=at, ydtype=yt,
                xdtype=QX[n % 3] if (n + fi) % 3 else None, mplace=((2, 3), (1, "m8"))[n % 2],
                aplace=((0, "m8"), (2, 4))[n // 2 % 2], **places(n, N))
        for n, (mt, at) in enumerate(((yt, None) for yt in YDTYPES)):  # mul and add apart
            add("one-operand", MODES[n % 3], family, M, K, N, act=ACTS[(n + 1) % 4], multype=mt, ydtype=YDTYPES[(n + 1) % 3],
                xdtype=QX[n % 3] if n % 3 else None)
            add("one-operand", MODES[(n + 1) % 3], family, M, K, N, act=ACTS[(n + 2) % 4], addtype=mt,
                ydtype=YDTYPES[(n + 2) % 3], xdtype=QX[n % 3] if (n + 1) % 3 else None)
        for n, (form, yform) in enumerate(itertools.product(("add", "mul"), ("odd", "aligned"))):
            for mi, mode in enumerate(MODES):
                yt = YDTYPES[(n + mi + fi) % 3]
                other = YDTYPES[(n + mi + fi + 1) % 3]
                add("in-place", mode, family, M, K, N, inplace=form, yform=yform, ydtype=yt, multype=other, addtype=other,
                    act=ACTS[(n + mi) % 4], xdtype=QX[(n + mi) % 3] if mi else None)
        for n, (rs, cs) in enumerate(((True, False), (False, True), (True, True), (False, False))):
            bare = not (rs or cs)
            add("scales", "plain", family, M, K, N, rs=rs, cs=cs, act=("relu", "prelu")[n % 2] if bare else ACTS[n % 4],
                ydtype=("float32", "bfloat16")[n % 2] if bare else YDTYPES[n % 3], addtype="bfloat16" if bare else y16[n % 2])
        if family in GLU:
            for n, (cs, mode) in enumerate(((True, "plain"), (False, "plain"), (True, "act"), (True, "norm"))):
                add("scales-up", mode, family, M, K, N, cs=cs, csu=True, rs=n == 1, act=ACTS[n % 4], ydtype=YDTYPES[n % 3],
                    addtype=y16[n % 2], xdtype=QX[n % 3] if mode != "plain" else None)
                add("scales-up", mode, family, M, K, N, cs=cs, csu=False, rs=n == 1, act=("relu", "prelu", "none")[n % 3],
                    ydtype=("float32", "bfloat16")[n % 2], addtype="bfloat16", xdtype=QX[n % 3] if mode != "plain" else None)
    # 5. unusual W: all zero with K > 0 (Y is the epilogue of b; GLU: act(b) * b_up), an all-zero up and an
    #    all-zero gate W, a W with an empty column, a fully dense W with all +1 in one column and all -1
    #    in the next under X rows of 127 and of -128 (K = 1100: a sign or accumulator mix-up shows)
    for fi, family in enumerate(FAMILIES):
        M, K, N = _eshape(family)
        ws = ("zero", "emptycol", "signcols") + (("zero_up", "zero_gate") if family in GLU else ())
        for wi, w in enumerate(ws):
            for mi, mode in enumerate(("plain",) if w == "signcols" else ("plain", "act")):
                add("unusual-w", mode, family, M, 1100 if w == "signcols" else K, N, w=w, s=64 if w == "emptycol" else 2,
                    act=ACTS[1 + (wi + mi + fi) % 3], ydtype=YDTYPES[(wi + mi + fi) % 3], multype=YDTYPES[(wi + fi) % 3],
                    addtype=YDTYPES[(mi + fi + 1) % 3], xdtype=QX[wi % 3] if mi else None)
    return out


# ---- the drawn cases --------------------------------------------------------------------------

K_POOL = sorted(set(CF.K_POOL) | {64, 65, 1024, 1100})
N_POOL = sorted(set(CF.N_POOL) | {32, 33, 577})
M_TILE = sorted(set(CF.M_POOL) | {257})


def drawn_cases(counter=None):
    """PER_PAIR cases per (mode, family) pair from one stream, drawn as
    test_gpu_ex_fuzz.drawn_cases draws; the X and Y types go round their lists."""
    rng = np.random.default_rng(SEED)
    out = []
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    for mi, mode in enumerate(MODES):
        xs = ("int8",) if mode == "plain" else QX
        combos = list(itertools.product(xs, YDTYPES))
        for fi, family in enumerate(FAMILIES):
            for j in range(PER_PAIR):
                i = fi * PER_PAIR + j
                xdtype, ydtype = combos[i % len(combos)]
                N = int(rng.integers(1, 1301)) if rng.random() < CF.OFF_POOL else pick(N_POOL)
                K = int(rng.integers(1, 3001)) if rng.random() < CF.OFF_POOL else pick(K_POOL)
                M = pick([m for m in (M_TILE if family not in SPLITK else CF.M_POOL)
                          if family not in SPLITK or m <= I8_GEMV_MAX_M])
                act, mt, at = pick(ACTS), pick(OPTYPES), pick(OPTYPES)
                places = [(pick(CF.C0S), pick(CF.PADS)) for _ in range(3)]
                inplace, yform = pick((None, None, "add", "mul")), pick(("odd", "aligned"))
                scales = pick(("both", "row", "col", "none"))
                s, rs_out = pick(CF.SPARS), rng.random() < 0.75
                xoff = int(rng.integers(0, 16)) if mode == "plain" else int(rng.integers(0, 4))
                gamma, eps, csu = pick(("none", "own", "slice")), pick((1e-5, 1e-6)), rng.random() < 0.75
                if mt is None and at is None and act in ("none", "prelu") and family not in GLU:
                    at = "bfloat16"  # (a descriptor without an epilogue is the plain call)
                if {"mul": mt, "add": at}.get(inplace) != ydtype:
                    inplace = None   # in place only where the types allow it
                if mode != "plain":
                    scales = "col"
                bare = scales == "none" or (family in GLU and not csu)
                if bare and ydtype == "float16":
                    scales, csu, bare = ("col" if scales == "none" else scales), True, False
                if bare:  # the chain's magnitudes: fp32 or bf16, no square
                    mt, at = (t if t != "float16" else "bfloat16" for t in (mt, at))
                    act = "relu" if act == "relu2" else act
                out.append(_mk("drawn", mode, family, M, K, N, 5000 + len(out), s=s, xdtype=xdtype, ydtype=ydtype, xoff=xoff,
                               act=act, multype=mt, addtype=at, inplace=inplace, yform=yform, yplace=places[0],
                               mplace=places[1], aplace=places[2], rs=scales in ("both", "row"),
                               cs=scales in ("both", "col"), csu=csu, rs_out=rs_out, gamma=gamma, eps=eps))
                if counter is not None:
                    counter.append(out[-1].seed)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(directed_cases() + drawn_cases())


def case_id(c):
    return f"{c.seed}-{c.name}-{c.mode}-{c.family}-{c.M}x{c.K}x{c.N}"


# ---- the case builder ------------------------------------------------------------------------------

def _call_case(c, seed=None):
    """The test_gpu_call_fuzz Case whose X and W builders this case reuses."""
    kind = {"act": "actquant", "norm": "normquant"}.get(c.mode, "scaled")
    return CF._mk(c.name, kind, "rx", c.M, c.K, c.N, c.seed if seed is None else seed, s=c.s, xdtype=c.xdtype)


def _ws(c):
    """(gate W, up W or None)."""
    K, N, glu = c.K, c.N, c.family in GLU
    if K == 0:
        z = np.zeros((0, N), np.int32)
        return z, (z if glu else None)
    if c.w == "signcols":
        Wg = np.where(np.arange(N)[None, :] % 2 == 0, 1, -1).astype(np.int32) * np.ones((K, 1), np.int32)
        return Wg, (-Wg if glu else None)
    Wg = CF._make_w(_call_case(c), K - 1)
    Wu = CF._make_w(_call_case(c, c.seed + 100000), K - 1) if glu else None
    if c.w == "emptycol":
        for W in (Wg, Wu):
            if W is not None:
                W[:, N // 2] = 0
                if not W[0].any():
                    W[0, 0] = 1
                if not W[K - 1].any():
                    W[K - 1, N - 1] = -1
    if c.w in ("zero", "zero_gate"):
        Wg = np.zeros_like(Wg)
    if c.w in ("zero", "zero_up") and glu:
        Wu = np.zeros_like(Wu)
    return Wg, Wu


def _x(c):
    """(X in its type as a CPU tensor, its widened fp32 copy)."""
    import torch
    M, K = c.M, c.K
    if K == 0:
        return torch.zeros((M, 0), dtype=torch.int8), np.zeros((M, 0), F)
    if c.w == "signcols":  # rows of 127, of -128 and, last, alternating
        X = np.where(np.arange(M)[:, None] % 2 == 0, 127, -128).astype(np.int8) * np.ones((1, K), np.int8)
        X[M - 1, ::2] = 5
        return torch.from_numpy(X), X.astype(F)
    return CF._make_x(_call_case(c), 0, K - 1)


def _count(x, y, where=None):
    d = x.view(np.uint32) != y.view(np.uint32)
    return (int(d.sum()), d.size) if where is None else (int(d[where].sum()), int(where.sum()))


def share_ok(name, differ, total):
    return differ >= (0.25 if name == "relu" else 0.10) * total


def _pow2_into(scale, top, bound):
    """scale * 2^-e, e the least integer with top * 2^-e <= 2^bound, exactly."""
    e = int(np.ceil(np.log2(top))) - bound if top > 0 else 0
    out = (scale.astype(np.float64) * 2.0 ** -e).astype(F)
    assert np.array_equal(out.astype(np.float64) * 2.0 ** e, scale.astype(np.float64)), e
    return out


@functools.lru_cache(maxsize=None)
def build(c):
    """One case's inputs, operands and expectation, computed once, never
    modified; the module docstring's input conditions are asserted here."""
    import oracle as O
    import tspgemm as T
    M, K, N = c.M, c.K, c.N
    glu, quant = c.family in GLU, c.mode != "plain"
    assert c.mode in MODES and c.family in FAMILIES and c.s in CF.SPARS and c.w in WS, c
    assert c.xdtype in (QX if quant else ("int8",)) and 0 <= c.xoff <= (3 if quant else 15), c
    assert c.act in ACTS and c.multype in OPTYPES and c.addtype in OPTYPES and c.ydtype in YDTYPES, c
    assert 1 <= M <= 257 and (M <= I8_GEMV_MAX_M or c.family not in SPLITK) and K >= 0 and N >= 1, c
    assert (K > 0 or not quant) and (N < 16384 or K == 192), c
    assert (c.cs or not quant) and not (c.rs and quant) and (c.rs_out <= quant) and (c.csu <= glu), c
    assert glu or c.multype or c.addtype or c.act in ("relu", "relu2") or not (c.rs or c.cs) or c.name != "drawn", c
    if unscaled(c):
        assert c.act != "relu2" and "float16" not in (c.ydtype, c.multype, c.addtype), c
    lds = {}
    for name, t, c0, pad in (("Y", c.ydtype, c.yc0, c.ypad), ("mul", c.multype, c.mc0, c.mpad),
                             ("add", c.addtype, c.ac0, c.apad)):
        if t:
            assert c0 >= 0 and XF.pad_of(c0, N, pad) >= 0, (c, name)
            lds[name] = XF.ld_of(c0, N, pad)
    if c.inplace:
        op = c.inplace
        assert (c.multype if op == "mul" else c.addtype) == c.ydtype and lds[op] == lds["Y"], (c, "in place")

    Wg, Wu = _ws(c)
    arrays = O.tcsc_encode(Wg).arrays
    arrays_up = O.tcsc_encode(Wu).arrays if glu else None
    b = np.linspace(-3, 3, N).astype(F)
    bu = (np.linspace(0.5, -0.25, N) * np.where(np.arange(N) % 2, -1.0, 1.0)).astype(F) if glu else None
    alpha = np.linspace(-0.5, 0.5, N).astype(F)
    rs, cs = _draw_scales(M, N, 0, c.seed)
    csu = _draw_scales(M, N, 0, c.seed + 5)[1] if c.csu else None
    g = NQ._gamma(K) if c.gamma != "none" else None
    Xt, Xw = _x(c)

    def front(Xw_):
        """(q int8, deq or None): X through the mode's front end."""
        if not quant:
            q = Xw_.astype(np.int8)
            assert np.array_equal(q.astype(F), Xw_)
            return q, None
        return T.act_quant_ref(T.rms_norm_ref(Xw_, g, c.eps)[0] if c.mode == "norm" else Xw_)

    q, deq = front(Xw)
    rs_, cs_ = (rs if c.rs else None), (cs if c.cs else None)
    # the magnitudes: exact powers of two, y under 2^6 and u under 2^1
    zb = np.zeros(N, F)
    if c.rs or c.cs:
        r0 = deq if quant else rs_
        top = float(np.abs(I8._ref(q, Wg, zb, r0, cs_)).max())
        if c.cs:
            cs_ = _pow2_into(cs_, top, 6)
        else:
            rs_ = _pow2_into(rs_, top, 6)
    if c.csu:
        csu = _pow2_into(csu, float(np.abs(I8._ref(q, Wu, zb, deq if quant else rs_, csu)).max()), 1)

    def y_of(q_, deq_, rows=slice(None), W=Wg, bias=b, col=None):
        col = cs_ if W is Wg else csu
        return I8._ref(q_, W, bias, deq_ if quant else None if rs_ is None else rs_[rows], col)

    y32 = y_of(q, deq)
    u32 = y_of(q, deq, W=Wu, bias=bu) if glu else None
    assert np.isfinite(y32).all() and (u32 is None or np.isfinite(u32).all()), c
    if c.rs or c.cs:
        assert float(np.abs(y32).max()) <= 2.0 ** 6 + 3, (c, float(np.abs(y32).max()))
    if c.csu:
        assert float(np.abs(u32).max()) <= 2.0 + 0.5, (c, float(np.abs(u32).max()))

    # the operands (test_gpu_epilogue.expect's recipe) and the expectation
    al = alpha if c.act == "prelu" else None
    rng = np.random.default_rng(c.seed + 31)
    ay = T.epilogue_ref(y32, c.act, al)
    a = (ay * u32).astype(F) if glu else ay
    Gt = Gw = Rt = Rw = None
    if c.multype:
        G = (rng.uniform(0.5, 2.0, a.shape) * rng.choice([-1.0, 1.0], a.shape)).astype(F)
        Gt, Gw = E._round_to(G, c.multype)
    if c.addtype:
        p = np.abs(a.astype(np.float64) * (Gw if c.multype else 1.0))
        R = (rng.uniform(-1.0, 1.0, a.shape) * 2.0 ** np.ceil(np.log2(np.where(p > 0, p, 1.0)))).astype(F)
        Rt, Rw = E._round_to(R, c.addtype)
    r_ = deq if quant else rs_

    def want_of(Wa, Wb, ba, bb, ca, cb):
        if glu:
            return GL._want(T, q, Wa, Wb, ba, bb, c.act, r_, ca, cb, al, Gw, Rw)
        return T.epilogue_ref(y32, c.act, al, Gw, Rw)

    want32 = want_of(Wg, Wu, b, bu, cs_, csu)
    assert np.isfinite(want32).all(), (c, "the expectation is not finite")
    if c.ydtype != "float32":
        assert float(np.abs(want32).max()) <= YMAX[c.ydtype], (c, "the expectation overflows the Y type")
    want = _ybits_of(want32, c.ydtype)
    if c.ydtype != "float32":
        assert np.array_equal(want, _cast_bits(want32, c.ydtype)) and np.isfinite(torch_from_bits(want, c.ydtype)).all()

    # the discrimination conditions: (differing, of) per name; asserted here where the case is large
    # enough, pooled over the group by test_i8_fuzz_ref.py where it is not
    shares, pooled = {}, {}
    if c.act in ("relu", "relu2"):
        shares["relu"] = _count(ay, y32)
    # the multiply and the add the fused forms would contract: (a, its factor) before the residual
    fa, fg = (a, Gw) if c.multype else (ay, u32) if glu else (None, None)
    if fg is not None and c.addtype and K > 0:  # (K = 0: b * b_up is exact, there is no rounding to contract)
        nz, d64 = fa != 0, np.float64
        t16 = c.multype if c.multype not in (None, "float32") else "bfloat16"
        shares["fused"] = _count((fa.astype(d64) * fg.astype(d64) + Rw.astype(d64)).astype(F), want32, nz)
        shares["add before multiply"] = _count(((fa + Rw).astype(F) * fg).astype(F), want32, nz)
        shares["a rounded to 16 bits first"] = _count(((E._round_to(fa, t16)[1] * fg).astype(F) + Rw).astype(F), want32, nz)
    if glu and K > 0 and c.w == "rand" and c.act != "none":  # (y * u is symmetric: act none tells neither)
        shares["gate and up swapped"] = _count(want_of(Wu, Wg, bu, b, csu, cs_), want32)
        late = T.epilogue_ref((y32 * u32).astype(F), c.act, al)
        shares["activation after the multiply"] = _count(late, a, y32 < 0)
    for name, (differ, total) in shares.items():
        if total >= SMALL:
            assert share_ok(name, differ, total), (c, name, "is told apart from the contract in only", differ, "of", total)
        else:
            pooled[name] = (differ, total)

    # edge dependence
    if c.w == "zero" or K == 0:  # Y is the epilogue of b alone; GLU: act(b) * b_up
        flat = np.ascontiguousarray(np.broadcast_to(b, (M, N)), F)
        fa_ = T.epilogue_ref(flat, c.act, al)
        if glu:
            fa_ = (fa_ * bu[None, :]).astype(F)
            assert np.array_equal(want, _ybits_of(T.epilogue_ref(fa_, "none", None, Gw, Rw), c.ydtype)), c
        else:
            assert np.array_equal(want, _ybits_of(T.epilogue_ref(flat, c.act, al, Gw, Rw), c.ydtype)), c
        assert not Wg.any() and (Wu is None or not Wu.any())
    else:
        for W in (Wg, Wu):
            if W is not None and W.any():
                assert W[0].any() and W[K - 1].any() and W[:, 0].any() and W[:, N - 1].any(), c
        if c.w == "zero_up":
            assert not Wu.any() and Wg.any() and np.array_equal(u32, np.broadcast_to(bu, (M, N)))
        if c.w == "zero_gate":
            assert not Wg.any() and Wu.any() and np.array_equal(y32, np.broadcast_to(b, (M, N)))
        if c.w == "emptycol":
            assert not Wg[:, N // 2].any(), (c, "no column of W is empty")
        if c.w == "signcols":
            assert (np.abs(Wg) == 1).all() and (Wg[:, 0::2] == 1).all() and (Wg[:, 1::2] == -1).all() and K >= 1100
        head = slice(0, min(M, 8))
        X2 = Xw[head].copy()
        X2[:, K - 1] = 0
        q2, deq2 = front(X2)
        Wd, bd_ = (Wu, bu) if c.w == "zero_gate" else (Wg, b)
        assert not np.array_equal(y_of(q2, deq2, head, W=Wd, bias=bd_), (u32 if c.w == "zero_gate" else y32)[head]), \
            (c, "X[:, K - 1] does not reach y")
        if M >= 2:
            assert not np.array_equal(want[M - 1], want[M - 2]), (c, "rows M - 1 and M - 2 agree")
    if c.mode == "act":
        assert np.abs(q).max() == 127
    for arr in (Xw, b, alpha, y32, want32, want) + tuple(x for x in (rs_, cs_, csu, bu) if x is not None):
        arr.setflags(write=False)
    return types.SimpleNamespace(arrays=arrays, arrays_up=arrays_up, Xt=Xt, Xw=Xw, q=q, b=b, bu=bu, alpha=alpha, rs=rs_,
                                 cs=cs_, csu=csu, g=g, deq=deq, y32=y32, u32=u32, Gt=Gt, Gw=Gw, Rt=Rt, Rw=Rw, want32=want32,
                                 want=want, lds=lds, pooled=pooled, Wg=Wg, Wu=Wu)


# ---- the GPU check ---------------------------------------------------------------------------------

def open_handle(tsg, arrays, K, N, M, kernel):
    """A plain handle pinned to the integer kernels; kernel 1: the tile kernel (at
    M <= 32 by set_i8_small(1)), 2: the split-K kernel."""
    h = tsg.TCSCDevice(*arrays, K, N)
    h.set_i8_mfma(2)
    h.set_i8_small(1 if kernel == 1 and M <= I8_GEMV_MAX_M else 0)
    assert h.call_i8_kernel(M) == kernel and h.call_i8_mfma(M) == 1, (M, K, N, kernel, h.call_i8_kernel(M))
    return h


def assert_pick(tsg, c):
    if c.family == "i8gemv":
        assert tsg.i8gemv_pick(c.K, c.N) == gemv_pick(c.K, c.N), (c, tsg.i8gemv_pick(c.K, c.N))
    if c.family == "glu_gemv":
        assert tsg.i8glu_pick(c.K, c.N) == glu_pick(c.K), (c, tsg.i8glu_pick(c.K, c.N))


def x_on_device(c, Xt):
    """X on the GPU: an int8 X `xoff` bytes into a larger int8 buffer (torch's
    allocations start on 16 bytes), a float X `xoff` elements into one."""
    import torch
    if c.mode != "plain":
        return _x_on_device(Xt, c.xoff)
    M, K = Xt.shape
    store = torch.zeros(M * K + 32, dtype=torch.int8, device="cuda")
    Xd = store[c.xoff:c.xoff + M * K].view(M, K)
    Xd.copy_(Xt)
    assert Xd.data_ptr() % 16 == c.xoff and Xd.is_contiguous()
    return Xd


@pytest.mark.parametrize("c", cases(), ids=case_id)
def test_i8_fuzz(tsg, c):
    import torch
    bc = build(c)
    M, N, K = c.M, c.N, c.K
    glu = c.family in GLU
    hg = open_handle(tsg, bc.arrays, K, N, M, kernel_of(c))
    hu = open_handle(tsg, bc.arrays_up, K, N, M, kernel_of(c)) if glu else None
    assert_pick(tsg, c)
    Xd = x_on_device(c, bc.Xt)
    gbuf, gd = NQ._gamma_dev(bc.g, K, c.gamma == "slice")
    bud = _dev(bc.bu) if glu else None
    cud = _dev(bc.csu) if bc.csu is not None else None
    inp = E.Inputs(bc, X=Xd, extra=[("gamma", gbuf), ("b_up", bud), ("col_scale_up", cud)])
    if c.inplace:
        buf, view, box = E.inplace_outputs(M, N, c.ydtype)[c.yform]
        fill, only = (_fill, _assert_only_view_written) if c.ydtype == "float32" else (_fill16, _assert_only_view_written16)
        assert c.yform == "odd" or view.data_ptr() % 16 == 0
    else:
        (buf, view, box, fill, only), = _outputs(M, N, c.ydtype, c0=c.yc0, pad=XF.pad_of(c.yc0, N, c.ypad)).values()
    assert tuple(view.shape) == (M, N) and (M == 1 or view.stride(0) == bc.lds["Y"]), (c, view.stride())
    mbuf, mview = E.place(bc.Gt, c.mc0, XF.pad_of(c.mc0, N, c.mpad)) if c.inplace != "mul" else (None, view)
    abuf, aview = E.place(bc.Rt, c.ac0, XF.pad_of(c.ac0, N, c.apad)) if c.inplace != "add" else (None, view)
    keep = [None if t is None else t.clone() for t in (mbuf, abuf)]
    norm = c.mode == "norm"

    def check(call, what):
        fill(buf)
        if c.inplace:
            view.copy_((bc.Gt if c.inplace == "mul" else bc.Rt).cuda())
        rbuf, rd_out = A._scale_out(M) if c.rs_out else (None, None)
        out = call(rd_out)
        torch.cuda.synchronize()
        assert out is view
        CF.assert_bits(_got_bits(view, c.ydtype), bc.want, c, what)
        only(buf, *box, (tuple(c), what))
        for t, k, n in zip((mbuf, abuf), keep, ("mul", "add")):
            assert t is None or E.same_bytes(t, k), (tuple(c), what, n, "buffer was written")
        if c.rs_out:
            A._assert_scale_out(rbuf, M, bc.deq, (tuple(c), what))
        inp.assert_unchanged((tuple(c), what))

    def kw(rd_out, **over):
        d = dict(act=c.act, alpha=inp.alpha if c.act == "prelu" else None, mul=mview, add=aview, row_scale=inp.rs,
                 col_scale=inp.cs, quant=XF.QUANT[c.mode], gamma=gd, eps=c.eps if norm else None, row_scale_out=rd_out)
        d.update(over)
        return d

    if glu:
        check(lambda rd_out: hg.gemm_torch_glu(hu, Xd, inp.b, bud, view, col_scale_up=cud, **kw(rd_out)), c.family)
        if c.cross:  # the two-call sequence on the add streams: u in fp32, then the gate call with mul = u
            for h in (hg, hu):
                h.set_i8_mfma(1)
                assert h.call_i8_kernel(M) == 0
            U = hu.gemm_torch_ex(Xd, bud, row_scale=inp.rs, col_scale=cud, quant=XF.QUANT[c.mode], gamma=gd,
                                 eps=c.eps if norm else None)
            check(lambda rd_out: hg.gemm_torch_ex(Xd, inp.b, view, **kw(rd_out, mul=U)), "two calls")
    else:
        check(lambda rd_out: hg.gemm_torch_ex(Xd, inp.b, view, **kw(rd_out)), c.family)
        hg.set_i8_mfma(1)  # the same call on the add streams
        assert hg.call_i8_kernel(M) == 0
        check(lambda rd_out: hg.gemm_torch_ex(Xd, inp.b, view, **kw(rd_out)), "add streams")
    hg.close()
    if hu is not None:
        hu.close()


# ---- structured W --------------------------------------------------------------------------------------

WS_KS = (600, 601)
WS_SHAPES = {"i8mfma": [(130, 140), (130, 1100)], "glu_tile": [(130, 140), (130, 1100)],
             "i8gemv": [(5, 140), (32, 140)], "glu_gemv": [(5, 140), (32, 140)]}


def ws_cases():
    """(family, W family name): each runs K in WS_KS and the family's (M, N) list; GLU once with the
    structured W as the gate and a uniform random up, once the reverse."""
    return [(f, w) for f in FAMILIES for w in FAMILY_NAMES]


@functools.lru_cache(maxsize=None)
def ws_x(M, K):
    X = np.random.default_rng(31 * M + K).integers(-127, 128, size=(M, K)).astype(np.int8)
    X[0, 0], X[-1, -1] = -127, 127
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def ws_uniform(K, N):
    import oracle as O
    W = O.gen_ternary(K, N, 2, 77 + K + N)
    W.setflags(write=False)
    return W


def ws_build(family, wname, M, K, N, swap=False):
    """(gate W, up W or None, X, b, b_up, the expected fp32 bits) of one structured call."""
    import tspgemm as T
    W = families(K, N)[wname]
    X, b = ws_x(M, K), np.linspace(-3, 3, N).astype(F)
    if family not in GLU:
        return W, None, X, b, None, I8._ref(X, W, b).view(np.uint32)
    other, bu = ws_uniform(K, N), np.linspace(0.5, -0.25, N).astype(F)
    Wg, Wu = (other, W) if swap else (W, other)
    return Wg, Wu, X, b, bu, GL._want(T, X, Wg, Wu, b, bu, "none").view(np.uint32)


@pytest.mark.parametrize("family,wname", ws_cases(), ids=lambda v: str(v))
def test_i8_structured_w(tsg, oracle_mod, family, wname):
    kernel = 2 if family in SPLITK else 1
    for K in WS_KS:
        for M, N in WS_SHAPES[family]:
            for swap in (False, True) if family in GLU else (False,):
                Wg, Wu, X, b, bu, want = ws_build(family, wname, M, K, N, swap)
                hg = open_handle(tsg, oracle_mod.tcsc_encode(Wg).arrays, K, N, M, kernel)
                Xd, bd = _dev(X), _dev(b)
                if family in GLU:
                    hu = open_handle(tsg, oracle_mod.tcsc_encode(Wu).arrays, K, N, M, kernel)
                    got = hg.gemm_torch_glu(hu, Xd, bd, _dev(bu), act="none")
                    hu.close()
                else:
                    got = hg.gemm_torch_x(Xd, bd)
                bad = I8._bits(got) != want
                assert not bad.any(), (family, wname, M, K, N, swap, int(bad.sum()), np.argwhere(bad)[:4].tolist())
                hg.close()


# ---- isolation ---------------------------------------------------------------------------------------------

ISO_SHAPES = [(33, 200, 33), (5, 200, 33), (33, 208, 33), (5, 208, 33)]


ISO_CASES = [(f, *s) for f in FAMILIES for s in ISO_SHAPES if s[0] <= I8_GEMV_MAX_M or f not in SPLITK]


def iso_family_of(kind, M):
    """The stale-scratch sequences name a kind, "i8" or "glu": its split-K kernel at M <= 32, else its tile kernel."""
    return {"i8": ("i8mfma", "i8gemv"), "glu": ("glu_tile", "glu_gemv")}[kind][M <= I8_GEMV_MAX_M]


@functools.lru_cache(maxsize=None)
def iso_build(family, M, K, N, seed=0):
    """A PLAIN int8 call with every operand: prelu, both scales (GLU: the up column scale too)."""
    import tspgemm as T
    rng = np.random.default_rng(1000 * M + K + seed)
    glu = family in GLU
    Wg, Wu = I8._w(K, N, K + N), (I8._w(K, N, K + N + 1) if glu else None)
    X = rng.integers(-127, 128, size=(M, K)).astype(np.int8)
    b, bu = np.linspace(-3, 3, N).astype(F), np.linspace(0.5, -0.25, N).astype(F)
    alpha = np.linspace(-0.5, 0.5, N).astype(F)
    rs, cs, csu = (rng.uniform(0.004, 0.01, M).astype(F), rng.uniform(0.02, 0.08, N).astype(F),
                   rng.uniform(0.002, 0.008, N).astype(F))
    if glu:
        want = GL._want(T, X, Wg, Wu, b, bu, "prelu", rs, cs, csu, alpha)
    else:
        want = T.epilogue_ref(I8._ref(X, Wg, b, rs, cs), "prelu", alpha=alpha)
    assert np.isfinite(want).all()
    return types.SimpleNamespace(Wg=Wg, Wu=Wu, X=X, b=b, bu=bu, alpha=alpha, rs=rs, cs=cs, csu=csu,
                                 want=want.view(np.uint32))


def _poisoned(a, fill, lead=5, tail=7):
    """a (1-D or 2-D, contiguous) in the middle of a device buffer of `fill`."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.full((lead + t.numel() + tail,), fill, dtype=t.dtype, device="cuda")
    buf[lead:lead + t.numel()] = t.reshape(-1).cuda()
    return buf[lead:lead + t.numel()].view(t.shape)


@pytest.mark.parametrize("family,M,K,N", ISO_CASES, ids=lambda v: str(v))
def test_i8_poisoned_neighbours(tsg, oracle_mod, family, M, K, N):
    """X in the middle (48 bytes in: 16-byte aligned, so K = 208 takes the 16-byte loads and K = 200
    the byte-wise ones) of an int8 buffer of 127, then of -128; b, b_up, alpha and the scales inside
    NaN-filled buffers: Y's bits are the reference's under both.  The tile families at M = 5 run
    under set_i8_small(1).  The poison only surrounds valid memory."""
    fam = family
    ic = iso_build(fam, M, K, N)
    kernel = 2 if fam in SPLITK else 1
    hg = open_handle(tsg, oracle_mod.tcsc_encode(ic.Wg).arrays, K, N, M, kernel)
    hu = open_handle(tsg, oracle_mod.tcsc_encode(ic.Wu).arrays, K, N, M, kernel) if fam in GLU else None
    nan = float("nan")
    for poison in (127, -128):
        Xd = _poisoned(ic.X, poison, lead=16 * 3, tail=16 * 3)
        bd, ad, rd, cd = (_poisoned(v, nan) for v in (ic.b, ic.alpha, ic.rs, ic.cs))
        if hu is not None:
            Y = hg.gemm_torch_glu(hu, Xd, bd, _poisoned(ic.bu, nan), act="prelu", alpha=ad, row_scale=rd, col_scale=cd,
                                  col_scale_up=_poisoned(ic.csu, nan))
        else:
            Y = hg.gemm_torch_ex(Xd, bd, act="prelu", alpha=ad, row_scale=rd, col_scale=cd)
        assert np.array_equal(I8._bits(Y), ic.want), (family, M, K, N, poison)
    hg.close()
    if hu is not None:
        hu.close()


@functools.lru_cache(maxsize=None)
def stale_build(family, M, K, N, quant, scale):
    """A quantising relu2 call; scale: the magnitude of X (the longer call's is large)."""
    import tspgemm as T
    rng = np.random.default_rng(100 * M + K + (quant == "norm"))
    glu = family in GLU
    Wg, Wu = I8._w(K, N, K + N), (I8._w(K, N, K + N + 1) if glu else None)
    X = (rng.standard_normal((M, K)) * scale).astype(F)
    g = rng.uniform(0.5, 1.5, K).astype(F) if quant == "norm" else None
    b, bu = np.linspace(-3, 3, N).astype(F), np.linspace(0.5, -0.25, N).astype(F)
    cs, csu = rng.uniform(0.02, 0.08, N).astype(F), rng.uniform(0.002, 0.008, N).astype(F)
    q, deq = T.act_quant_ref(T.rms_norm_ref(X, g, 1e-5)[0] if quant == "norm" else X)
    if glu:
        want = GL._want(T, q, Wg, Wu, b, bu, "relu2", deq, cs, csu)
        swapped = GL._want(T, q, Wu, Wg, bu, b, "relu2", deq, csu, cs)
    else:
        want, swapped = I8._ref(q, Wg, b, deq, cs), None
    assert np.isfinite(want).all()
    return types.SimpleNamespace(Wg=Wg, Wu=Wu, X=X, g=g, b=b, bu=bu, cs=cs, csu=csu, deq=deq.view(np.uint32),
                                 want=want.view(np.uint32), swapped=None if swapped is None else swapped.view(np.uint32))




STALE = [(k, q) for k in ("i8", "glu") for q in ("act", "norm")]
STALE_K, STALE_N = 200, 65


def _plain_want(ic, quant):
    """The plain quantising descriptor call on the gate W."""
    import tspgemm as T
    q, deq = T.act_quant_ref(T.rms_norm_ref(ic.X, ic.g, 1e-5)[0] if quant == "norm" else ic.X)
    return I8._ref(q, ic.Wg, ic.b, deq, ic.cs).view(np.uint32)


class Stale:
    """One handle (GLU: the gate and the up handle) under set_i8_mfma(2) and the staged
    device inputs of its calls: call(M, form) allocates nothing once (M, scale) is staged
    and Y and out are given, so it can be captured."""

    def __init__(self, tsg, oracle_mod, kind, quant):
        self.kind, self.quant, self.dev = kind, quant, {}
        ic = stale_build(iso_family_of(kind, 130), 130, STALE_K, STALE_N, quant, 300.0)
        self.hg = tsg.TCSCDevice(*oracle_mod.tcsc_encode(ic.Wg).arrays, STALE_K, STALE_N)
        self.hu = tsg.TCSCDevice(*oracle_mod.tcsc_encode(ic.Wu).arrays, STALE_K, STALE_N) if kind == "glu" else None
        self.pin()

    def handles(self):
        return [h for h in (self.hg, self.hu) if h is not None]

    def pin(self):
        for h in self.handles():
            h.set_i8_mfma(2)
            h.set_i8_small(0)
            assert h.call_i8_kernel(130) == 1 and h.call_i8_kernel(33) == 1 and h.call_i8_kernel(5) == 2

    def stage(self, M, scale):
        if (M, scale) not in self.dev:
            ic = stale_build(iso_family_of(self.kind, M), M, STALE_K, STALE_N, self.quant, scale)
            assert np.array_equal(ic.Wg, stale_build(iso_family_of(self.kind, 130), 130, STALE_K, STALE_N, self.quant, 300.0).Wg)
            d = {n: _dev(getattr(ic, n)) for n in ("X", "b", "bu", "cs", "csu")}
            d["g"] = None if ic.g is None else _dev(ic.g)
            self.dev[(M, scale)] = (ic, d)
        return self.dev[(M, scale)]

    def call(self, M, form="glu", scale=3.0, Y=None, out=None):
        """-> (Y, row_scale_out, the expected Y bits, the case)."""
        import torch
        ic, d = self.stage(M, scale)
        out = torch.zeros(M, device="cuda") if out is None else out
        kw = dict(quant=self.quant, gamma=d["g"], eps=1e-5 if self.quant == "norm" else None, row_scale_out=out)
        if self.kind == "glu" and form == "glu":
            Y = self.hg.gemm_torch_glu(self.hu, d["X"], d["b"], d["bu"], Y, col_scale=d["cs"], col_scale_up=d["csu"], **kw)
            return Y, out, ic.want, ic
        if self.kind == "glu" and form == "swapped":
            Y = self.hu.gemm_torch_glu(self.hg, d["X"], d["bu"], d["b"], Y, col_scale=d["csu"], col_scale_up=d["cs"], **kw)
            return Y, out, ic.swapped, ic
        Y = self.hg.gemm_torch_ex(d["X"], d["b"], Y, col_scale=d["cs"], **kw)
        return Y, out, _plain_want(ic, self.quant), ic

    def close(self):
        for h in self.handles():
            h.close()


def _assert_stale(res, what):
    import torch
    Y, out, want, ic = res
    torch.cuda.synchronize()
    assert np.array_equal(I8._bits(Y), want), (what, "Y")
    assert np.array_equal(I8._bits(out), ic.deq), (what, "row_scale_out")


@pytest.mark.parametrize("kind,quant", STALE, ids=lambda v: str(v))
def test_i8_stale_scratch(tsg, oracle_mod, kind, quant):
    """One handle: a quantising call at M = 130 with large X, then at M = 33 (the tile kernel) and
    M = 5 (the split-K kernel) with other X and the same K: the int8 scratch and deq still hold the
    longer call's rows past M.  Then a quantising call on the add streams, which share the scratch
    allocation, and back.  GLU: gate/up, up/gate, a plain quantising call on the gate handle, the
    first again."""
    s = Stale(tsg, oracle_mod, kind, quant)
    form = "glu" if kind == "glu" else "plain"
    _assert_stale(s.call(130, form, scale=300.0), (kind, quant, 130))
    for M in (33, 5):
        _assert_stale(s.call(M, form), (kind, quant, M))
    s.hg.set_i8_mfma(1)  # the add streams on the same scratch
    assert s.hg.call_i8_kernel(33) == 0
    _assert_stale(s.call(33, "plain"), (kind, quant, "add streams", 33))
    s.pin()
    _assert_stale(s.call(130, form, scale=300.0), (kind, quant, "back", 130))
    _assert_stale(s.call(5, form), (kind, quant, "back", 5))
    if kind == "glu":
        for M in (33, 5):
            for f in ("glu", "swapped", "plain", "glu"):
                _assert_stale(s.call(M, f), (kind, quant, f, M))
    s.close()


@pytest.mark.parametrize("kind,quant", STALE, ids=lambda v: str(v))
def test_i8_graph_replay_over_stale_scratch(tsg, oracle_mod, kind, quant):
    """After reserve(130) / reserve_glu(hu, 130): a captured quantising M = 33 call (the tile kernel)
    and a captured M = 5 call (the split-K kernel), each replayed twice after an eager M = 130 call
    has overwritten the scratch; each replay equals the reference and the eager result."""
    import torch
    s = Stale(tsg, oracle_mod, kind, quant)
    form = "glu" if kind == "glu" else "plain"
    if kind == "glu":
        s.hg.reserve_glu(s.hu, 130)
    else:
        s.hg.reserve(130)
    _assert_stale(s.call(130, form, scale=300.0), (kind, quant, 130))
    for M in (33, 5):
        Y, out, want, ic = s.call(M, form)  # eager: stages the inputs, and its outputs are the capture's
        _assert_stale((Y, out, want, ic), (kind, quant, M, "eager"))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            s.call(M, form, Y=Y, out=out)
        for replay in range(2):
            _assert_stale(s.call(130, form, scale=300.0), (kind, quant, "eager 130"))
            Y.zero_()
            out.zero_()
            g.replay()
            _assert_stale((Y, out, want, ic), (kind, quant, M, "replay", replay))
        del g  # destroyed here (it synchronises the device), not by a garbage collection inside a later capture
    s.close()
