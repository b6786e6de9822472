// tsg_x16mfma.hip -- fp16 / bf16 activations on the matrix cores
// (tsg_x16mfma_kernel): dense over W, fp32 accumulators, for the unquantised
// device calls whose X is fp16 or bf16 on a plain-TCSC handle with K <= 131072
// that opted in (tcsc_hip_set_x16_mfma; tsg_plan.h call_x16_mfma).
//
// What it stores.  W unpacks to +-1.0 and 0.0 of X's own type, so every product
// is x, -x or 0, exact; v_mfma_f32_32x32x16_{bf16,f16} adds them into fp32
// accumulators in an order the library does not promise (fixed for a given
// call shape: run-to-run deterministic).  That is NOT the serial BaseTCSC chain
// of the add streams: the two agree byte for byte only where every partial sum
// is exact in fp32 (the contract and its error bound: include/ternary_spgemm.h).
// A dense pass multiplies by W's zeros too: an inf or NaN in a row of X makes
// that row of Y unspecified (inf * 0) and no other.  Everything after the chain
// is the walks' epilogue, finish_store1 (tsg_epilogue.h): scale_bias, the PReLU
// rule, the fused epilogue and the one rounding of tsg_ytype.h, one element per
// lane by the register map of tsg_i8frag.h (mfma_row).
//
// Split.  Workgroup: 256 threads = 4 waves side by side, tile 128 rows x 256
// columns; a wave owns 128 x 64 -- one 64-column granule of the image -- as
// 4 x 2 accumulator tiles of 32 x 32 (128 accumulator registers).  Unpacking
// costs more here than in tsg_i8mfma.hip (an image dword becomes eight operand
// dwords, not four), so the tile is tall: each unpacked B fragment feeds four
// row tiles, which is what 256 registers per wave allow next to the
// accumulators (two workgroups share a CU by the launch bounds, so one wave's
// unpacking overlaps another's matrix instructions).  A call with M <= 64 runs
// the kernel built with two row tiles per wave (template RT).  Grid: one workgroup per (M tile, column tile), the column tile
// fastest -- neighbours share the X tile in L2.  K goes by in steps of 64: four
// matrix instructions deep.
//
// A (activations).  The step's 128 rows x 64 elements (128 B per row) are
// loaded from the caller's X in place by the whole workgroup -- thread t the
// 16-byte pieces (row t / 8 + 32 j, eighth t % 8), j < 4, so eight
// neighbouring lanes read one row's 128 contiguous bytes: one 16-byte
// load each where K % 8 == 0 and X is 16-byte aligned, else element by
// element; rows >= M and k >= K are zero with the address clamped, nothing
// outside [X, X + M K) is read -- one step ahead, into registers, and stored
// to the other half of a double-buffered LDS tile after the step's matrix
// instructions: one barrier per step.  LDS row pitch 144 B = 128 + 16.  A
// fragment read is a ds_read_b128 of lane l at (32 rt + l % 32) * 144 + 64 kk +
// 32 (l / 32) + 16 t; the LDS serves a b128 read 16 lanes at a time (64 banks
// x 4 B = 16 slots of 16 B), and the 16 lanes of a group are 16 consecutive
// rows at one k offset, slot (9 row + c) mod 16: 9 is odd, so they fall on 16
// distinct slots -- conflict-free.  (A group of 16 stores is two rows x eight
// pieces, slots 9 r .. 9 r + 7 and 9 r + 9 .. 9 r + 16: one slot of 16 is hit
// twice; there are 4 stores per thread and step against 16 fragment reads.)
//
// B (weights).  The packed image of tsg_i8mfma.hip (tsg_internal.h I8Geom), no
// second format: a lane's 16 bytes of a (granule, step) are one load, requested
// one step ahead; no index, no LDS.  Dword 2 c2 + kk holds the lane's 16
// entries k = 64 ks + 32 kk + 16 (lane / 32) + e of column 32 c2 + lane % 32
// and feeds two matrix instructions, t = 0 (e < 8) and t = 1; the lane's A
// fragment of instruction t is its row's 8 elements at the same k, so a
// matrix instruction's sum over 16 k pairs the right elements whatever order
// the hardware walks them in.  x16_unpack turns the codes into 16-bit patterns
// with v_perm_b32 (below).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tsg_epilogue.h"
#include "tsg_i8frag.h"
#include "tsg_internal.h"
#include "tsg_ytype.h"

namespace tsg {

namespace {

constexpr int kX16Pitch = 2 * kI8KStep + 16;  // LDS bytes per row (header: the bank argument)

typedef float v16f __attribute__((ext_vector_type(16)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));

// The high and the low byte of +1.0 (table byte 0: code kI8Pos), -1.0 (byte 2:
// kI8Neg) and 0.0 (byte 3: kI8Zero) in the X type: the codes are v_perm_b32
// selectors into these tables as they are
template <int XT>
struct X16Tab;
template <>
struct X16Tab<kXBF16> {  // 0x3f80, 0xbf80, 0x0000
    static constexpr uint32_t hi = 0x00bf003fu, lo = 0x00800080u;
    typedef v8bf frag;
};
template <>
struct X16Tab<kXF16> {  // 0x3c00, 0xbc00, 0x0000
    static constexpr uint32_t hi = 0x00bc003cu, lo = 0u;
    typedef v8h frag;
};
static_assert(kI8Pos == 0 && kI8Neg == 2 && kI8Zero == 3, "the codes index the byte tables");

// Entries 4 d .. 4 d + 3 of a packed dword (bits [8 b + 2 d, + 2) of byte b) ->
// two operand dwords, {entry 4 d, 4 d + 1} and {4 d + 2, 4 d + 3}.  The four
// codes, masked in place, select the four high bytes H and the four low bytes
// L from the tables (both sources the table: selectors 0-3 mean its bytes
// however the sources are numbered); a second v_perm_b32 interleaves them,
// selectors 4-7 the bytes of its first source (H), 0-3 of its second (L).  An
// fp16 pattern has a zero low byte: selector 12, the constant 0x00, and no L.
// Per packed dword: 4 x (shift, and, 2 or 1 table v_perm, 2 v_perm) = 23 (bf16)
// or 19 (fp16) VALU instructions for the B operands of 8 matrix instructions.
template <int XT>
__device__ __forceinline__ void x16_unpack(uint32_t w, int d, uint32_t &o0, uint32_t &o1)
{
    const uint32_t m = (w >> (2 * d)) & 0x03030303u;
    const uint32_t H = __builtin_amdgcn_perm(X16Tab<XT>::hi, X16Tab<XT>::hi, m);
    if (X16Tab<XT>::lo != 0) {
        const uint32_t L = __builtin_amdgcn_perm(X16Tab<XT>::lo, X16Tab<XT>::lo, m);
        o0 = __builtin_amdgcn_perm(H, L, 0x05010400u);
        o1 = __builtin_amdgcn_perm(H, L, 0x07030602u);
    } else {
        o0 = __builtin_amdgcn_perm(H, H, 0x050c040cu);
        o1 = __builtin_amdgcn_perm(H, H, 0x070c060cu);
    }
}

__device__ __forceinline__ v16f x16_mfma(v8bf a, v8bf b, v16f c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ v16f x16_mfma(v8h a, v8h b, v16f c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

}  // namespace

template <int XT, int RT, bool PRELU>
__global__ __launch_bounds__(kX16Threads, 2) void tsg_x16mfma_kernel(
    const uint16_t *__restrict__ X, const uint4 *__restrict__ img, const float *__restrict__ b,
    const float *__restrict__ alpha, const float *__restrict__ rs, const float *__restrict__ cs, Epi ep,
    float *__restrict__ Y, int64_t ldY, int ytype, int M, int N, int K, int nks, int ntiles, int xvec)
{
    typedef typename X16Tab<XT>::frag frag;
    __shared__ __attribute__((aligned(16))) uint8_t xs[2][kX16TileM * kX16Pitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nt = blockIdx.x % ntiles, mt = blockIdx.x / ntiles;
    const int m0 = mt * kX16TileM, nw = nt * kX16TileN + kI8WaveN * wave;  // the wave's tile: rows m0 .., columns nw ..
    const bool live = nw < N;                                               // (uniform) it holds an element of Y
    // the wave's B stream, step ks at bw[64 ks]; a wave past N has no granule of its own and reads none
    const uint4 *bw = img + (size_t)(live ? nw / kI8WaveN : 0) * nks * 64 + lane;

    // the thread's four pieces of a step's A tile -- rows ar, ar + 32, ar + 64,
    // ar + 96 of the tile at the step's elements ak .. ak + 7 -- global -> registers ...
    const int ar = tid >> 3, ak = 8 * (tid & 7);
    uint4 areg[4];
    auto aload = [&](int ks) {
        const int k = ks * kI8KStep + ak;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int m = m0 + ar + 32 * j;
            // elements of the piece inside X (K % 8 == 0: all 8 or none)
            const int n = m < M && k < K ? min(8, K - k) : 0;
            const uint16_t *src = X + (n > 0 ? (size_t)m * K + k : 0);
            if (xvec) {
                const uint4 v = *reinterpret_cast<const uint4 *>(src);
                areg[j] = n > 0 ? v : make_uint4(0, 0, 0, 0);
            } else {
                uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
                for (int e = 0; e < 8; e++)
                    if (e < n) w[e >> 1] |= (uint32_t)src[e] << (16 * (e & 1));
                areg[j] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
    };
    // ... -> the LDS tile `buf`
    auto astore = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; j++)
            *reinterpret_cast<uint4 *>(&xs[buf][(ar + 32 * j) * kX16Pitch + 2 * ak]) = areg[j];
    };

    v16f acc[RT][2];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int c2 = 0; c2 < 2; c2++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[rt][c2][r] = 0.0f;

    // one step's matrix instructions, from the LDS tile at xb and the image bytes bq
    auto step = [&](const uint8_t *xb, const uint4 &bq) {
        const uint32_t bword[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
        for (int kk = 0; kk < 2; kk++)
#pragma unroll
            for (int t = 0; t < 2; t++) {
                frag a[RT];
#pragma unroll
                for (int rt = 0; rt < RT; rt++)
                    a[rt] = *reinterpret_cast<const frag *>(xb + 32 * rt * kX16Pitch + 64 * kk + 16 * t);
#pragma unroll
                for (int c2 = 0; c2 < 2; c2++) {
                    uint4 u;
                    x16_unpack<XT>(bword[2 * c2 + kk], 2 * t, u.x, u.y);
                    x16_unpack<XT>(bword[2 * c2 + kk], 2 * t + 1, u.z, u.w);
                    const frag bf = __builtin_bit_cast(frag, u);
#pragma unroll
                    for (int rt = 0; rt < RT; rt++) acc[rt][c2] = x16_mfma(a[rt], bf, acc[rt][c2]);
                }
            }
    };

    uint4 bq = make_uint4(0, 0, 0, 0);
    if (nks > 0) {
        bq = bw[0];
        aload(0);
        astore(0);
    }
    __syncthreads();
    const int arow = (lane & 31) * kX16Pitch + 32 * (lane >> 5);
    for (int ks = 0; ks < nks; ks++) {
        const bool more = ks + 1 < nks;
        const uint4 bn = bw[(size_t)(more ? ks + 1 : ks) * 64];  // the next step's B, in flight over this one
        if (more) aload(ks + 1);
        step(xs[ks & 1] + arow, bq);  // (a wave past N too, on granule 0: no branch around the accumulators)
        if (more) astore((ks + 1) & 1);
        bq = bn;
        __syncthreads();  // the next tile is written; this one's reads are done
    }
    if (!live) return;

    const int yt = ytype & kYTypeMask;
    const bool has_rs = rs != nullptr, has_cs = cs != nullptr, epi = (ytype & kYEpi) != 0;
    // rows outermost, so that a row's scale is loaded once and used at once
    int nn[2];
    float bn[2], an[2], cn[2];
#pragma unroll
    for (int c2 = 0; c2 < 2; c2++) {
        const int n = nn[c2] = nw + 32 * c2 + (lane & 31);
        bn[c2] = n < N ? b[n] : 0.0f;
        an[c2] = PRELU && n < N ? alpha[n] : 0.0f;
        cn[c2] = has_cs && n < N ? cs[n] : 0.0f;
    }
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int m = m0 + 32 * rt + mfma_row(r, lane);
            if (m >= M) continue;
            const float rm = has_rs ? rs[m] : 0.0f;
#pragma unroll
            for (int c2 = 0; c2 < 2; c2++)
                if (nn[c2] < N)
                    finish_store1<PRELU>(Y, yt, epi, ldY, ep, m, nn[c2], acc[rt][c2][r], has_rs, rm, has_cs, cn[c2], bn[c2],
                                         an[c2]);
        }
}

namespace {

template <int XT, int RT>
auto x16_kernel2(bool prelu)
{
    return prelu ? tsg_x16mfma_kernel<XT, RT, true> : tsg_x16mfma_kernel<XT, RT, false>;
}

// low: every row of Y is in the upper half of the one M tile -- two row tiles
auto x16_kernel(bool bf16, bool low, bool prelu)
{
    return bf16 ? (low ? x16_kernel2<kXBF16, 2>(prelu) : x16_kernel2<kXBF16, 4>(prelu))
                : (low ? x16_kernel2<kXF16, 2>(prelu) : x16_kernel2<kXF16, 4>(prelu));
}

}  // namespace

int launch_tcsc_x16mfma(const void *X, int xtype, const uint32_t *img, int K, const YOut &o)
{
    if (!mfma_grid_ok(o.M, o.N, kX16TileM, kX16TileN, kX16Threads)) return -2;  // (run_mfma refuses it first)
    if (xtype != kXF16 && xtype != kXBF16) return -2;
    const int64_t ntiles = (o.N + kX16TileN - 1) / kX16TileN, mtiles = (o.M + kX16TileM - 1) / kX16TileM;
    const dim3 grid((unsigned)(ntiles * mtiles)), block(kX16Threads);
    auto *kernel = x16_kernel(xtype == kXBF16, o.M <= 64, o.prelu);
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)o.stream, static_cast<const uint16_t *>(X),
                       reinterpret_cast<const uint4 *>(img), o.b, o.alpha, o.rs, o.cs, o.ep, static_cast<float *>(o.Y), o.ldY,
                       o.kernel_ytype(false), o.M, o.N, K, i8_nks(K), (int)ntiles, x_vec_ok(X, K, 8));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace tsg
