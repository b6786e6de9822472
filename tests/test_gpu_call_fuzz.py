"""Seeded shape and layout fuzz over the typed, scaled and quantising
device-pointer calls (gemm_torch_into / _x / _xy, gemm_torch_scaled,
gemm_torch_actquant, gemm_torch_normquant) through every kernel family on the
GPU.  The feature files (test_gpu_ldy, _xtype, _ytype, _scaled, _actquant,
_normquant) pin the arithmetic of these calls on a short list of shapes; this
file is about their indexing everywhere else: K past the walk's LDS chunk, N
below one store group, views whose every row takes the vector stores, K below
a quad, the row pass at its sum shape's boundaries, X two and three elements
off alignment, empty, all-zero and dense W.

The reference.  Everything is compared as integers, no tolerance.  The expected
Y is the contract of include/ternary_spgemm.h: X widened exactly; for normquant
tspgemm.rms_norm_ref, for actquant and normquant tspgemm.act_quant_ref; the
oracle's chain (base_tcsc / base_blocked_tcsc) with a zero bias;
test_gpu_scaled.expect32 with the row scale (deq for the quantising calls), the
column scale and b, then the PReLU rule; test_gpu_ytype._cast_bits for a 16-bit
Y.  row_scale_out must hold deq bit for bit.

One case is a Case tuple (below).  After its call(s) -- the plain call, and the
PReLU call too where the case has prelu -- it asserts the kernel that ran
(call_kernel, and jit_width / jit_waves / call_tile_rows where pinned), every
element of the view, every element of the [M + 2, ldY] buffer outside the view
still the sentinel, row_scale_out's slice equal to deq and its surroundings
untouched, and X, b, alpha, the scales and gamma byte-identical to before.

Inputs (build() asserts all of this on the CPU; test_call_fuzz_ref.py runs it
for every case).  typed / scaled: init_x_frac (int8: integer draws) through
test_gpu_ytype._x_for.  actquant: test_gpu_actquant._build_x's near-tie rows
where K >= 64 (its all-zero row and its row below the eps moved to rows 0 and 1:
the "ordinary" rows below are the others), below that uniform rows with the row
maximum at a drawn k.
normquant: uniform rows times 3 * U[0.5, 2) (the arithmetic-order variants are
the feature files' business).  b = linspace(-3, 3, N), alpha = linspace(-0.5,
0.5, N), cs = U[0.5, 2), rs as test_gpu_scaled._scase draws it.  Unless W is the
all-zero one: rows 0 and K - 1 and columns 0 and N - 1 of W hold a nonzero (one
is set where the draw left none), X is nonzero at k = 0 and K - 1 in every
ordinary row, zeroing X[:, K - 1] changes the expectation, for a chunked walk
zeroing X from the last chunk's first k on changes it, and rows M - 1 and M - 2
of the expectation differ.  (A blocked handle drops the K rows past its last
whole block, BlockedTCSC.h:17: K - 1 is there the last row of that block, and K
is at least B.)  The expectation is finite and within the Y type's range; where
it is not, X is scaled by an exact power of two as _x_for's shift does (an int8
X by an arithmetic shift).  RMSNorm undoes any scale of X, so a normquant case
is asserted only: |xn| <= sqrt(K) * 1.5 and |q| <= 127 bound its Y far below
fp16's range at these K.  No case is redrawn or dropped.

The cases: DIRECTED, a named list of the smallest shapes that reach each
mechanism (thresholds restated from tsg_internal.h / tsg_plan.cpp next to the
constants below), then PER_PAIR drawn cases for each (kind, family) pair from
one default_rng(SEED) stream, M, K and N from edge pools around the tile, chunk
and store-group sizes plus a few off-pool draws."""
import collections
import functools
import itertools
import types

import numpy as np
import pytest

import test_gpu_actquant as A
import test_gpu_normquant as NQ
from test_gpu_ldy import _dev, _jit_handle
from test_gpu_scaled import _draw_scales, _got_bits, _outputs, _ybits_of, expect32
from test_gpu_xtype import _tdtype, _x_on_device
from test_gpu_ytype import YMAX, _x_for

pytestmark = pytest.mark.gpu

F = np.float32
SEED = 2027
PER_PAIR = 4

KINDS = ("typed", "scaled", "actquant", "normquant")
QUANT = ("actquant", "normquant")
FAMILIES = ("pc", "walk", "rows64", "rows128", "rx", "blocked")
PAIRS = [(k, f) for k in KINDS for f in FAMILIES]  # every pair exists (blocked: the plain call only)
KERNEL = {"pc": "tsg_tcsc_ell_pc_kernel", "walk": "tsg_tcsc_ell_kernel", "rows64": "tsg_jit64_kernel",
          "rows128": "tsg_jit_kernel", "rx": "tsg_tcsc_rx_kernel", "blocked": "tsg_jit_kernel"}
XDTYPES = ("float32", "float16", "bfloat16", "int8")
YDTYPES = ("float32", "float16", "bfloat16")
C0S = (0, 1, 4, 8)
PADS = (0, 1, 3, "m8")  # "m8": whatever makes ldY a multiple of 8
SPARS = (1, 2, 4, 16, 64)
KNOBS = ("TSG_JIT_HALF", "TSG_JIT_PAIR", "TSG_JIT_QBLOCK", "TSG_JIT_XDIRECT", "TSG_KERNEL")

# tsg_internal.h kEllTileM / kEllMaxC: the walk's M tiles and the K rows one LDS chunk of each holds
ELL_TILE_M = (1, 4, 8, 16, 32)
ELL_MAX_C = (40956, 10236, 5116, 2556, 1276)
# tsg_plan.h kEllMidM, tsg_plan.cpp kEllPcRowsMaxMN
ELL_MID_M = 32
ELL_PC_MAX_MN = 32768

Case = collections.namedtuple(
    "Case", "name kind family M K N s w xdtype ydtype xoff c0 pad prelu rs cs rs_out gamma eps mode width knob B seed")


@pytest.fixture(autouse=True)
def _oracle_built(oracle_mod):
    """The cached cases below import the oracle themselves: it is built first."""


def xdtypes_of(kind):
    return XDTYPES[:3] if kind in QUANT else XDTYPES


def walk_tile(M, K):
    """Index into ELL_TILE_M of the tile a forced walk runs (tsg_plan.cpp
    pick_ell_variant with small_m >= 2, before its producer/consumer rule)."""
    one8 = K <= ELL_MAX_C[2]
    if one8 and 8 < M <= ELL_MID_M:
        return 2
    if one8 and M > ELL_MID_M:
        return max(i for i in (2, 3, 4) if i == 2 or K <= ELL_MAX_C[i])
    v = 0
    while v + 1 < len(ELL_TILE_M) and M > ELL_TILE_M[v]:
        v += 1
    return v


def walk_chunks(c):
    """(chunks, first k of the last chunk) of a walk case: K above the tile's
    chunk is walked in chunks of that size (tsg_host.cpp build_ell_image)."""
    if c.family != "walk":
        return 1, 0
    C = ELL_MAX_C[walk_tile(c.M, c.K)]
    nch = max(1, -(-c.K // C))
    return nch, (nch - 1) * C


def pad_of(c):
    return (-(c.c0 + c.N)) % 8 if c.pad == "m8" else c.pad


def _mk(name, kind, family, M, K, N, seed, s=4, w="rand", xdtype="float32", ydtype="float32", xoff=0, c0=1, pad=1,
        prelu=True, rs=None, cs=True, rs_out=None, gamma=None, eps=None, mode=None, width=0, knob=None, B=0):
    """A Case with the fields a kind or family does not have at their neutral
    value, so that equal cases are equal tuples."""
    quant, norm = kind in QUANT, kind == "normquant"
    if family != "walk":  # set_small_m: the planner's own pick for pc, never the walk for the others
        mode = 0 if family == "pc" else 1
    elif mode is None:    # every call on the walk; M <= 4 without the producer/consumer tiles
        mode = 3 if M <= 4 else 2
    if family == "blocked":
        prelu, B = False, B or 64
    return Case(name, kind, family, M, K, N, s, w, xdtype, ydtype, xoff, c0, pad, bool(prelu),
                bool(rs if rs is not None else kind == "scaled") and kind == "scaled",
                bool(cs) and kind != "typed", bool(rs_out if rs_out is not None else quant) and quant,
                (gamma or "own") if norm else "none", (eps or 1e-5) if norm else 0.0, mode,
                width if family in ("rows64", "rows128") else 0, knob if family == "rows64" else None, B, seed)


# ---- the directed cases --------------------------------------------------------------------

# (family, M, K, extra) of the small shape each family runs in the N and W groups
_FAMILY_SHAPE = {"pc": (2, 193, {}), "walk": (16, 193, {}), "rows64": (65, 193, dict(width=16)),
                 "rows128": (130, 193, {}), "rx": (70, 193, {}), "blocked": (70, 200, dict(B=16))}


def directed_cases():
    out = []

    def add(name, kind, family, M, K, N, **kw):
        out.append(_mk(name, kind, family, M, K, N, 1000 + len(out), **kw))

    # 1. the walk restaging X per K chunk under every kind: K above the tile's chunk
    #    (16-row tile 2556 -> 3 chunks, quad loads; 32-row tile 1276 -> 5 chunks, scalar loads;
    #    4-row tile 10236 -> 2 chunks; 1-row tile 40956 -> 2 chunks)
    for i, (M, K, N, mode) in enumerate([(16, 5120, 40, 2), (32, 5117, 40, 2), (3, 10240, 40, 3), (1, 41000, 24, 3)]):
        x_typed, x_scaled = ("int8", "float16") if i % 2 == 0 else ("float16", "int8")
        add("chunked-walk", "typed", "walk", M, K, N, mode=mode, xdtype=x_typed, ydtype="float16", c0=i % 2)
        add("chunked-walk", "scaled", "walk", M, K, N, mode=mode, xdtype=x_scaled, ydtype="bfloat16", c0=1 - i % 2)
        add("chunked-walk", "actquant", "walk", M, K, N, mode=mode, xdtype="bfloat16", ydtype="float16", pad=3)
        add("chunked-walk", "normquant", "walk", M, K, N, mode=mode, xdtype=("float16", "float32")[i % 2],
            ydtype=("bfloat16", "float32")[i // 2], gamma=("own", "slice")[i % 2])
    # 2. the walk on the q8 copy over many M tiles, past the scratch's 128-row step
    for M, K, N in ((300, 388, 130), (129, 193, 40)):
        for kind in QUANT:
            add("walk-many-m-tiles", kind, "walk", M, K, N, mode=2, rs_out=True, ydtype=("float32", "bfloat16")[M % 2])
    # 3. N below one store group (8), below one ELL slice (16) and one past each
    for i, N in enumerate((1, 7, 9, 17)):
        for j, family in enumerate(FAMILIES):
            M, K, extra = _FAMILY_SHAPE[family]
            add("small-n", KINDS[(i + j) % 4], family, M, K, N, ydtype=("float16", "bfloat16")[(i + j // 2) % 2],
                c0=(i + j) % 2, pad=(0, 1, 3, "m8")[(i + 2 * j) % 4], **extra)
    # 4. views whose every row takes the 16-byte stores: an aligned column offset, ldY a multiple
    #    of 8, N a whole number of segments (and one group more)
    for i, (family, width, M, N) in enumerate([("rows64", 128, 65, 128), ("rows64", 16, 65, 128),
                                               ("rows128", 64, 130, 512), ("rx", 0, 130, 256)]):
        for j, ydtype in enumerate(YDTYPES):
            for e in (0, 1):
                add("whole-segment-view", ("typed", "scaled")[(i + j + e) % 2], family, M, 193, N + 8 * e, width=width,
                    ydtype=ydtype, c0=8, pad="m8", xdtype=XDTYPES[(i + j + e) % 4])
    # 5. K below a quad and a pair under the quantising staging
    for i, K in enumerate((1, 2, 3, 4, 5)):
        for j, (family, width) in enumerate([("walk", 0), ("rows64", 128), ("rows64", 8), ("rows128", 0)]):
            kind = QUANT[(i + j) % 2]
            add("tiny-k", kind, family, (5, 70)[(i + j // 2) % 2], K, 40, width=width, mode=2,
                gamma="slice" if K in (3, 5) else "own", xdtype=XDTYPES[(i + j) % 3])
    # 6. the row pass's 256 partial sums where the lanes' iteration counts start to differ
    for i, K in enumerate((255, 256, 257, 260, 512, 1024)):
        for xoff in (0, 1):
            family = ("walk", "rows64")[(i + xoff) % 2]
            add("row-sum-boundary", "normquant", family, 16 if family == "walk" else 65, K, 40, xoff=xoff, width=16,
                xdtype=("float32", "bfloat16", "float16")[i % 3], eps=(1e-5, 1e-6)[xoff])
    # 7. the row layout's 188-row chunks (TSG_JIT_QBLOCK unset): one and two chunks, and 4 past
    for i, K in enumerate((188, 192, 376, 380)):
        for j, M in enumerate((64, 65)):
            add("row-layout-chunk-edge", QUANT[(i + j) % 2], "rows64", M, K, 130, width=(16, 128)[j])
    # 8. the quantisation scratch's 128-row allocation step
    for i, M in enumerate((128, 129, 257)):
        for j, family in enumerate(("rows64", "rows128")):
            add("scratch-step", QUANT[(i + j) % 2], family, M, 193, 40, width=(16, 64)[j])
    # 9. X two and three elements into a larger buffer (16-bit X at offset 2: 4-byte aligned, not 8)
    for kind in ("typed", "actquant"):
        for i, xdtype in enumerate(xdtypes_of(kind)):
            for xoff in (2, 3):
                family = ("walk", "rows64")[(i + xoff) % 2]
                add("x-offset", kind, family, 16 if family == "walk" else 65, 388, 130, xoff=xoff, xdtype=xdtype,
                    width=16, ydtype=YDTYPES[(i + xoff) % 3])
    # 10. an all-zero W with K > 0, a W with empty columns, a dense W
    for w, s in (("zero", 4), ("rand", 64), ("rand", 1)):
        for kind in ("scaled", "actquant"):
            for family in ("walk", "rows64"):
                add("unusual-w", kind, family, 16 if family == "walk" else 65, 193, 130, w=w, s=s, width=16,
                    ydtype=("float32", "float16")[kind == "scaled"])
    return out


# ---- the drawn cases --------------------------------------------------------------------------

def _around(values):
    return sorted({v + d for v in values for d in (-1, 0, 1) if v + d >= 1})


M_POOL = _around((1, 4, 8, 16, 32, 64, 128, 192, 256))
K_POOL = _around((4, 96, 188, 192, 256, 376, 384, 512, 1024, 1276))
N_POOL = _around((8, 16, 64, 128, 256, 512, 1024))
OFF_POOL = 0.15         # share of K and of N draws that are uniform instead: K up to 3000, N up to 1300
_ROWS64_SHAPES = [(128, None), (64, "TSG_JIT_QBLOCK=16"), (32, None), (16, "TSG_JIT_QBLOCK=8"), (8, None), (0, None),
                  (0, "TSG_JIT_HALF"), (0, "TSG_JIT_PAIR"), (128, "TSG_JIT_QBLOCK=8"), (64, None),
                  (32, "TSG_JIT_QBLOCK=16"), (16, None), (8, "TSG_JIT_QBLOCK=16"), (0, "TSG_JIT_HALF"),
                  (0, "TSG_JIT_PAIR"), (0, None)]
_ROWS128_WIDTHS = [64, 32, 16, 8, 0, 0, 64, 32, 16, 8, 0, 64, 32, 16, 8, 0]


def drawn_cases(counter=None):
    """PER_PAIR cases per (kind, family) pair from one stream.  The X and Y
    types, the 64-row image's width and knob and the 128-row image's width go
    round their lists (coverage does not depend on luck); everything else is
    drawn.  counter, a list, receives one entry per case drawn."""
    rng = np.random.default_rng(SEED)
    out = []
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    for ki, kind in enumerate(KINDS):
        combos = list(itertools.product(xdtypes_of(kind), YDTYPES))
        for fi, family in enumerate(FAMILIES):
            for j in range(PER_PAIR):
                i = fi * PER_PAIR + j
                xdtype, ydtype = combos[i % len(combos)]
                N = int(rng.integers(1, 1301)) if rng.random() < OFF_POOL else pick(N_POOL)
                K = int(rng.integers(1, 3001)) if rng.random() < OFF_POOL else pick(K_POOL)
                B = pick((16, 64)) if family == "blocked" else 0
                K = max(K, B)
                # the 1-row producer/consumer tiles take M <= 4; the walk stays at M <= 32 unless N <= 512
                top = 4 if family == "pc" else 33 if family == "walk" and N > 512 else M_POOL[-1]
                M = pick([m for m in M_POOL if m <= top])
                mode = 0 if family == "pc" else 1
                if family == "walk":
                    mode = 3 if M <= 4 else pick((0, 2, 3)) if M <= ELL_MID_M else pick((2, 3))
                width, knob = _ROWS64_SHAPES[ki * PER_PAIR + j] if family == "rows64" else (0, None)
                if family == "rows128":
                    width = _ROWS128_WIDTHS[ki * PER_PAIR + j]
                scales = pick(("both", "row", "col"))
                case = _mk("drawn", kind, family, M, K, N, 5000 + len(out), s=pick(SPARS), xdtype=xdtype, ydtype=ydtype,
                           xoff=int(rng.integers(0, 4)), c0=pick(C0S), pad=pick(PADS), prelu=rng.random() < 0.5,
                           rs=scales != "col", cs=scales != "row" if kind == "scaled" else rng.random() < 0.5,
                           rs_out=rng.random() < 0.75, gamma=pick(("none", "own", "slice")), eps=pick((1e-5, 1e-6)),
                           mode=mode, width=width, knob=knob, B=B)
                out.append(case)
                if counter is not None:
                    counter.append(case.seed)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(directed_cases() + drawn_cases())


def case_id(c):
    return f"{c.seed}-{c.name}-{c.kind}-{c.family}-{c.M}x{c.K}x{c.N}"


# ---- the case builder ------------------------------------------------------------------------------

def _ordinary_rows(c):
    """Rows that are neither the all-zero row nor the row below the eps of _build_x."""
    rows = np.ones(c.M, bool)
    if c.kind == "actquant" and c.K >= 64 and A._rows_plan(c.M)[2]:
        rows[:2] = False  # (_make_x moves them to the front)
    return rows


def _make_x(c, shift, klast):
    """(X in its type as a CPU tensor, its widened fp32 copy)."""
    import torch
    M, K = c.M, c.K
    rng = np.random.default_rng(c.seed + 77)
    if c.kind in ("typed", "scaled"):
        Xt, Xw = _x_for(M, K, c.xdtype, c.seed, 0 if c.xdtype == "int8" else shift)
        if c.xdtype == "int8" and shift:
            Xw = (Xt.numpy().astype(np.int32) >> shift).astype(F)
    else:
        if c.kind == "actquant" and K >= 64:
            # (its all-zero row and its row below the eps first, not last: rows M - 2 and M - 1
            # of Y would both be b in a 16-bit Y)
            X = np.roll(A._build_x(M, K, c.seed)[0], 2 if A._rows_plan(M)[2] else 0, axis=0)
        else:
            X = rng.uniform(-1.0, 1.0, size=(M, K)) * (3.0 * rng.uniform(0.5, 2.0, size=(M, 1)))
            if c.kind == "actquant":  # the row maximum at a drawn k
                top = 3.0 * rng.uniform(0.5, 2.0, size=M) * np.where(np.arange(M) % 2, -1.0, 1.0)
                X[np.arange(M), rng.integers(0, K, size=M)] = top
        X = (X.astype(F) * F(2.0 ** -shift)).astype(F)
        Xw = torch.from_numpy(X).to(_tdtype(c.xdtype)).to(torch.float32).numpy()
    Xw = np.array(Xw, F)
    for k in (0, klast):  # nonzero at both ends of every ordinary row (1 is exact in every type)
        Xw[(Xw[:, k] == 0) & _ordinary_rows(c), k] = 1
    Xt = torch.from_numpy(Xw).to(_tdtype(c.xdtype))
    assert np.array_equal(Xt.to(torch.float32).numpy(), Xw) and np.isfinite(Xw).all()
    return Xt, Xw


def _make_w(c, klast):
    import oracle as O
    K, N = c.K, c.N
    if c.w == "zero":
        return np.zeros((K, N), np.int32)
    W = O.gen_ternary(K, N, c.s, c.seed)
    rng = np.random.default_rng(c.seed + 99)
    W[klast + 1:] = 0  # (a blocked handle does not encode them)
    if not W[0].any():
        W[0, rng.integers(N)] = 1
    if not W[klast].any():
        W[klast, rng.integers(N)] = -1
    if not W[:, 0].any():
        W[rng.integers(klast + 1), 0] = 1
    if not W[:, N - 1].any():
        W[rng.integers(klast + 1), N - 1] = -1
    return W


@functools.lru_cache(maxsize=None)
def build(c):
    """One case's inputs and expectations, computed once, never modified; the
    module docstring's input conditions are asserted here."""
    import oracle as O
    import tspgemm as T
    M, K, N = c.M, c.K, c.N
    assert c.kind in KINDS and c.family in FAMILIES and c.s in SPARS and c.xdtype in xdtypes_of(c.kind), c
    assert M >= 1 and K >= max(1, c.B) and N >= 1 and c.c0 in C0S and c.pad in PADS and 0 <= c.xoff <= 3, c
    if c.family == "pc":  # what the planner asks of the 1-row producer/consumer tiles
        assert c.mode == 0 and M <= 4 and M * N <= ELL_PC_MAX_MN and K <= ELL_MAX_C[0], c
    klast = K // c.B * c.B - 1 if c.B else K - 1
    W = _make_w(c, klast)
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
    quant = c.kind in QUANT
    rs, cs = _draw_scales(M, N, 0 if quant else 4 if c.xdtype == "int8" else 12, c.seed)
    g = NQ._gamma(K) if c.gamma != "none" else None

    def expect(Xw, rows=slice(None)):
        """{'plain' | 'prelu': fp32 Y}, deq -- the contract, step by step (Xw: these rows of X)."""
        Xc, deq = Xw, None
        if c.kind == "normquant":
            Xc = T.rms_norm_ref(Xc, g, c.eps)[0]
        if quant:
            q, deq = T.act_quant_ref(Xc)
            Xc = q.astype(F)
        chain = run(Xc)
        assert not np.signbit(chain[chain == 0]).any()
        r = deq if quant else rs[rows] if c.rs else None
        with np.errstate(over="ignore", invalid="ignore"):
            return {key: expect32(chain, r, cs if c.cs else None, b, al) for key, al in (("plain", None),
                                                                                        ("prelu", alpha))}, deq

    # finite in the Y type: the exact power of two that brings the largest magnitude under 2^15
    # (fp16; the bias is not scaled, 2^15 + 3 < 65504) or 2^100
    shift = 0
    Xt, Xw = _make_x(c, 0, klast)
    y, deq = expect(Xw)
    top = max(float(np.abs(np.nan_to_num(v.astype(np.float64), nan=np.inf)).max()) for v in y.values())
    limit = 2.0 ** 15 if c.ydtype == "float16" else 2.0 ** 100
    if top > limit and c.kind != "normquant":
        shift = int(np.ceil(np.log2(top / limit)))
        assert c.xdtype != "int8" or shift <= 5, (c, "an int8 X cannot be scaled by", shift)
        Xt, Xw = _make_x(c, shift, klast)
        y, deq = expect(Xw)
    want = {}
    for key, v in y.items():
        assert np.isfinite(v).all(), (c, key, "the expectation is not finite")
        if c.ydtype != "float32":
            assert float(np.abs(v).max()) <= YMAX[c.ydtype], (c, key, "the expectation overflows the Y type")
        want[key] = _ybits_of(v, c.ydtype)
        want[key].setflags(write=False)

    if c.w == "zero":  # Y is b through the epilogue
        assert not W.any() and K > 0
        flat = {"plain": np.broadcast_to(b, (M, N)), "prelu": np.broadcast_to(np.where(b > 0, b, alpha * b), (M, N))}
        for key in want:
            assert np.array_equal(want[key], _ybits_of(np.ascontiguousarray(flat[key], F), c.ydtype)), (c, key)
    else:
        assert W[0].any() and W[klast].any() and W[:, 0].any() and W[:, N - 1].any(), c
        ordinary = _ordinary_rows(c)
        assert (Xw[ordinary][:, [0, klast]] != 0).all(), (c, "X is zero at an end of a row")
        head = slice(0, min(M, 8))  # (rows are independent: a change in these rows is a change)
        X2 = Xw[head].copy()
        X2[:, klast] = 0
        assert not np.array_equal(expect(X2, head)[0]["plain"], y["plain"][head]), (c, "X[:, K - 1] does not reach Y")
        nch, k_last_chunk = walk_chunks(c)
        if nch > 1:
            assert walk_tile(M, K) != 2, (c, "the 8-row tile's chunk depends on its image")
            X3 = Xw[head].copy()
            X3[:, k_last_chunk:] = 0
            assert 0 < k_last_chunk < K and not np.array_equal(expect(X3, head)[0]["plain"], y["plain"][head]), \
                (c, "the last chunk does not reach Y")
        if M >= 2:
            assert not np.array_equal(want["plain"][M - 1], want["plain"][M - 2]), (c, "rows M - 1 and M - 2 agree")
        if c.name == "unusual-w" and c.s == 64:
            assert (np.abs(W).sum(axis=0) == 0).any(), (c, "no column of W is empty")
    if c.kind == "actquant":  # the row maximum is where the recipe put it: the quantisation has an edge to lose
        assert np.abs(T.act_quant_ref(Xw)[0]).max() == 127
    for a in (Xw, b, alpha, rs, cs):
        a.setflags(write=False)
    nnz = int(np.count_nonzero(W))
    return types.SimpleNamespace(arrays=arrays, Xt=Xt, Xw=Xw, b=b, alpha=alpha, rs=rs if c.rs else None,
                                 cs=cs if c.cs else None, g=g, deq=deq, want=want, shift=shift, nnz=nnz)


def assert_bits(got, want, c, key):
    """The failure names the case's whole tuple, how many elements differ and the first few."""
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    first = [(int(m), int(n), hex(int(got[m, n])), hex(int(want[m, n]))) for m, n in bad[:6]]
    raise AssertionError(f"{c}: the {key} call: {len(bad)} of {want.size} elements differ; "
                         f"first (row, column, got, want): {first}")


# ---- the GPU check ---------------------------------------------------------------------------------

def _handle(tsg, c, arrays):
    M, K, N = c.M, c.K, c.N
    if c.family in ("rows64", "rows128"):
        rows = 64 if c.family == "rows64" else 128
        h = _jit_handle(tsg, arrays, K, N, rows, c.width)
        assert h.call_kernel(M) == KERNEL[c.family] and h.call_tile_rows(M) == rows, (c, h.call_kernel(M))
        if c.width:
            assert h.jit_width(M) == c.width and h.jit_waves(M) == 8, (c, h.jit_width(M), h.jit_waves(M))
        return h
    if c.family == "blocked":
        h = tsg.TCSCDevice.from_blocked(*arrays, K, N, c.B)
    else:
        h = tsg.TCSCDevice(*arrays, K, N)
    h.set_small_m(c.mode)
    if c.family == "rx":
        assert h.kernel_name() == KERNEL["rx"], (c, h.kernel_name())
    assert h.call_kernel(M) == KERNEL[c.family], (c, h.call_kernel(M))
    if c.family in ("pc", "walk"):
        assert h.call_tile_rows(M) == 0, c
    return h


def _call(h, c, Xd, bd, view, al, rd, cd, gd, rd_out):
    x32, y32 = c.xdtype == "float32", c.ydtype == "float32"
    if c.kind == "typed":  # the narrowest entry point that can express the case
        if x32 and y32:
            return h.gemm_torch_into(Xd, bd, view, alpha=al)
        if y32:
            return h.gemm_torch_x(Xd, bd, view, alpha=al)
        return h.gemm_torch_xy(Xd, bd, view, alpha=al)
    if c.kind == "scaled":
        return h.gemm_torch_scaled(Xd, bd, view, alpha=al, row_scale=rd, col_scale=cd)
    if c.kind == "actquant":
        return h.gemm_torch_actquant(Xd, bd, view, alpha=al, col_scale=cd, row_scale_out=rd_out)
    return h.gemm_torch_normquant(Xd, bd, gd, c.eps, view, alpha=al, col_scale=cd, row_scale_out=rd_out)


@pytest.mark.parametrize("c", cases(), ids=case_id)
def test_call_fuzz(tsg, monkeypatch, c):
    import torch
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if c.family == "rx":
        monkeypatch.setenv("TSG_KERNEL", "rx")
    if c.knob:
        name, _, value = c.knob.partition("=")
        monkeypatch.setenv(name, value or "1")
    bc = build(c)
    M, N, K = c.M, c.N, c.K
    h = _handle(tsg, c, bc.arrays)
    Xd = _x_on_device(bc.Xt, c.xoff)
    assert Xd.data_ptr() % (4 * Xd.element_size()) == c.xoff * Xd.element_size()
    bd, ad = _dev(bc.b), _dev(bc.alpha)
    rd = _dev(bc.rs) if bc.rs is not None else None
    cd = _dev(bc.cs) if bc.cs is not None else None
    gbuf, gd = NQ._gamma_dev(bc.g, K, c.gamma == "slice")
    named = [(t, n) for t, n in ((Xd, "X"), (bd, "b"), (ad, "alpha"), (rd, "row_scale"), (cd, "col_scale"),
                                 (gbuf, "gamma")) if t is not None]
    keep = [t.clone() for t, _ in named]
    (buf, view, box, fill, only), = _outputs(M, N, c.ydtype, c0=c.c0, pad=pad_of(c)).values()
    assert tuple(view.shape) == (M, N) and (M == 1 or view.stride(0) == c.c0 + N + pad_of(c))
    for key in ("plain", "prelu") if c.prelu else ("plain",):
        fill(buf)
        rbuf, rd_out = A._scale_out(M) if c.rs_out else (None, None)
        out = _call(h, c, Xd, bd, view, ad if key == "prelu" else None, rd, cd, gd, rd_out)
        torch.cuda.synchronize()
        assert out is view
        assert_bits(_got_bits(view, c.ydtype), bc.want[key], c, key)
        only(buf, *box, (tuple(c), key))
        if c.rs_out:
            A._assert_scale_out(rbuf, M, bc.deq, (tuple(c), key))
    for (t, n), k in zip(named, keep):
        assert torch.equal(t.view(torch.int8), k.view(torch.int8)), (tuple(c), n, "was written")
    h.close()
