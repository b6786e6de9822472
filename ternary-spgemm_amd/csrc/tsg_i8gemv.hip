// tsg_i8gemv.hip -- the int8-activation calls with 1 <= M <= 32 (decode shapes)
// on the integer matrix cores (tsg_i8gemv_kernel): K split across the waves of
// a workgroup, one workgroup per column tile, over the packed image the handle
// already holds for tsg_i8mfma_kernel (tsg_internal.h I8Geom).
//
// Why K may be split.  tsg_i8mfma.hip's argument: X is integer-valued with
// |x| <= 128 and W ternary, so every partial sum of a chain -- of any subset of
// its terms, in any order -- is an integer of magnitude <= 128 K <= 2^24.  The
// int32 sums of the waves' k ranges therefore add up to the chain's value
// whatever the order, v_cvt_f32_i32 of it is exact, and it is what the fp32 add
// streams store.  For the same reason each (column half, k half) of a step has
// an int32 accumulator tile of its own, summed at the end: back-to-back matrix
// instructions never wait for one another.
//
// Split.  Workgroup: S waves (S = blockDim.x / 64, the launcher's choice from
// 1, 2, 4, 8, 16; tsg_internal.h i8gemv_pick) and one column tile of TN = 32
// or 64 columns; all M <= 32 rows are one v_mfma_i32_32x32x32_i8 row tile.
// Wave w takes the k-steps (64 k each) w, w + S, ...: the workgroup's
// concurrent B loads are one contiguous run of the image.  No workgroup shares
// an output with another: no atomics, no workspace.  With TN = 32 the two
// halves of a 64-column granule are separate workgroups reading alternate 8
// bytes of the same lines, so the grid is numbered to put them on one XCD and
// its L2 (tsg_i8frag.h i8_splitk_tile).
//
// B (weights).  Per step a lane's 16 bytes (TN = 64) or its contiguous 8 bytes
// of column half c2 (TN = 32: dwords 2 c2 and 2 c2 + 1) are one load, global
// memory to registers, unpacked there by i8_unpack (tsg_i8frag.h).
//
// A (activations).  No wave reads a k range another wave of its workgroup
// reads, so X is not staged in LDS: a lane loads its two fragments of a step
// from global memory (tsg_i8frag.h i8_afrag_pair, by the read rule of
// i8_apiece; X is at most 32 K bytes, in L2 for every workgroup after the
// first).
//
// Latency.  kI8GemvDepth steps of A and B are in flight in registers before
// the first matrix instruction, and a slot is reloaded as soon as it is
// consumed; the K loop has no barrier and no LDS access.  A slot past the
// wave's last step holds a zero A (and any B): its matrix instructions add 0,
// so the loop body has no branch around them.
//
// Reduce and store.  Each wave sums its k halves and writes its accumulator
// registers to LDS as [wave][register][lane] ints -- a register's 64 lanes are
// 64 consecutive dwords: conflict-free -- one barrier, then wave w takes the
// registers w, w + S, ... (a register is a row group: tsg_i8frag.h mfma_row),
// sums their S partials, converts, and finishes the element it holds through
// finish_store1 (tsg_epilogue.h).  Registers whose rows are all >= M are
// neither written nor read.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tsg_epilogue.h"
#include "tsg_i8frag.h"
#include "tsg_internal.h"
#include "tsg_ytype.h"

namespace tsg {

namespace {

// Steps in flight per wave, chosen by measurement (the "depth"
// lines of profiles/i8gemv_ab.jsonl): 2 / 4 / 8 steps give 0.0109 / 0.0112 /
// 0.0116 ms at (M, K, N) = (32, 4096, 16384), the one cell above the rate at
// which calls are issued (0.0096-0.0103 in all the others, whatever the depth).
// 2 is the fastest there and the smallest: 70 / 106 VGPRs against 90 / 130.
#ifndef TSG_I8GEMV_DEPTH
#define TSG_I8GEMV_DEPTH 2
#endif
constexpr int kI8GemvDepth = TSG_I8GEMV_DEPTH;

}  // namespace

template <int TN, bool PRELU>
__global__ __launch_bounds__(TN == 64 ? 64 * kI8GemvWaves64 : 64 * kI8GemvWaves32) void tsg_i8gemv_kernel(
    const int8_t *__restrict__ X, const uint32_t *__restrict__ img, const float *__restrict__ b,
    const float *__restrict__ alpha, const float *__restrict__ rs, const float *__restrict__ cs, Epi ep,
    float *__restrict__ Y, int64_t ldY, int ytype, int M, int N, int K, int nks, int xvec)
{
    extern __shared__ int red[];  // [S][NR][64]
    constexpr int C2 = TN / 32, NR = 16 * C2, D = kI8GemvDepth;
    const int lane = threadIdx.x & 63, S = (int)(blockDim.x >> 6);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // the workgroup's tile: granule ct of 64 columns, and of it column half `half` (TN = 32)
    const I8SplitKTile t = TN == 32 ? i8_splitk_tile((int)blockIdx.x) : I8SplitKTile{(int)blockIdx.x, 0};
    const int ct = t.ct, half = t.half, n0 = kI8WaveN * ct + 32 * half;
    if (n0 >= N) return;  // (uniform) a workgroup of the grid's padding to 16

    const uint32_t *bw = img + ((size_t)ct * nks * 64 + lane) * 4 + 2 * half;  // step ks at bw + 256 ks
    const int row = lane & 31, kl = 16 * (lane >> 5);
    const int8_t *xr = i8_arow(X, row, M, K);
    const int cnt = i8_wave_steps(nks, w, S);

    uint32_t bq[D][2 * C2];
    v4i a[D][2];
    // the wave's j-th step into slot d (past its last step: a zero A)
    auto load = [&](int d, int j) {
        if (j < cnt) {
            const int ks = w + j * S;
            const uint32_t *p = bw + (size_t)ks * 256;
            if (TN == 64) {
                const uint4 v = *reinterpret_cast<const uint4 *>(p);
                bq[d][0] = v.x, bq[d][1] = v.y, bq[d][2] = v.z, bq[d][3] = v.w;
            } else {
                const uint2 v = *reinterpret_cast<const uint2 *>(p);
                bq[d][0] = v.x, bq[d][1] = v.y;
            }
            i8_afrag_pair(xr, row < M, kl, ks, K, xvec, a[d]);
        } else {
            i8_afrag_zero(a[d]);
        }
    };

    v16i acc[C2][2];
#pragma unroll
    for (int c2 = 0; c2 < C2; c2++)
#pragma unroll
        for (int kk = 0; kk < 2; kk++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[c2][kk][r] = 0;
#pragma unroll
    for (int d = 0; d < D; d++) {
#pragma unroll
        for (int f = 0; f < 2 * C2; f++) bq[d][f] = 0;
        load(d, d);
    }
    for (int i = 0; i < cnt; i += D) {
#pragma unroll
        for (int d = 0; d < D; d++) {
#pragma unroll
            for (int c2 = 0; c2 < C2; c2++)
#pragma unroll
                for (int kk = 0; kk < 2; kk++)
                    acc[c2][kk] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[d][kk], i8_unpack(bq[d][2 * c2 + kk]),
                                                                        acc[c2][kk], 0, 0, 0);
            load(d, i + d + D);
        }
    }

    // register j = 16 c2 + r of the wave -> red[(w NR + j) 64 + lane]
#pragma unroll
    for (int c2 = 0; c2 < C2; c2++)
#pragma unroll
        for (int r = 0; r < 16; r++)
            if (mfma_row0(r) < M) red[(w * NR + 16 * c2 + r) * 64 + lane] = acc[c2][0][r] + acc[c2][1][r];
    __syncthreads();

    const int yt = ytype & kYTypeMask;
    const bool has_rs = rs != nullptr, has_cs = cs != nullptr, epi = (ytype & kYEpi) != 0;
    for (int j = w; j < NR; j += S) {
        const int r = j & 15, m = mfma_row(r, lane), n = n0 + 32 * (j >> 4) + (lane & 31);
        if (mfma_row0(r) >= M) continue;  // (uniform) a register of padding rows
        int sum = 0;
        for (int s = 0; s < S; s++) sum += red[(s * NR + j) * 64 + lane];
        if (m >= M || n >= N) continue;
        finish_store1<PRELU>(Y, yt, epi, ldY, ep, m, n, (float)sum, has_rs, has_rs ? rs[m] : 0.0f, has_cs,
                             has_cs ? cs[n] : 0.0f, b[n], PRELU ? alpha[n] : 0.0f);
    }
}

int launch_tcsc_i8gemv(const int8_t *X, const uint32_t *img, int K, const YOut &o)
{
    if (o.M < 1 || o.M > kI8GemvMaxM) return -2;  // (the plan sends no other call here)
    const I8GemvPick p = i8gemv_pick(K, o.N);
    // TN = 64: one workgroup per granule; TN = 32: two, the granules padded to
    // a multiple of 8 (the XCD numbering above; the padding returns at once)
    const int64_t granules = ((int64_t)o.N + kI8WaveN - 1) / kI8WaveN;
    const int64_t wgs = p.tn == 64 ? granules : (granules + 7) / 8 * 16;
    const dim3 grid((unsigned)wgs), block(64 * p.S);
    const size_t lds = (size_t)p.S * (p.tn / 2) * 64 * sizeof(int);
    auto *kernel = p.tn == 64 ? (o.prelu ? tsg_i8gemv_kernel<64, true> : tsg_i8gemv_kernel<64, false>)
                              : (o.prelu ? tsg_i8gemv_kernel<32, true> : tsg_i8gemv_kernel<32, false>);
    hipLaunchKernelGGL(kernel, grid, block, lds, (hipStream_t)o.stream, X, img, o.b, o.alpha, o.rs, o.cs, o.ep,
                       static_cast<float *>(o.Y), o.ldY, o.kernel_ytype(false), o.M, o.N, K, i8_nks(K), x_vec_ok(X, K, 16));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace tsg
