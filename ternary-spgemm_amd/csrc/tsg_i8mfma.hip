// tsg_i8mfma.hip -- the int8-activation calls on the integer matrix cores
// (tsg_i8mfma_kernel): dense over W, int32 accumulators, for every device call
// whose activations are int8 after the input stage (an int8 X, or the q of an
// actquant / normquant call) on a plain-TCSC handle with K <= 131072.
//
// Why it stores the bits the fp32 add streams store.  X is integer-valued with
// |x| <= 128 and W is ternary, so every partial sum of a column's chain is an
// integer of magnitude <= 128 K <= 128 * 131072 = 2^24.  fp32 holds every
// integer up to 2^24 exactly, so each add of the fp32 chain is exact and the
// chain equals the integer dot product converted to fp32, whatever the order;
// the int32 accumulator (|sum| <= 2^24, no overflow) converted with
// v_cvt_f32_i32 (exact below 2^24, and never -0, like the chain) IS that value.
// Everything after it is the walks' epilogue, finish_store1 (tsg_epilogue.h):
// scale_bias, the PReLU rule, the fused epilogue and the one rounding of
// tsg_ytype.h, one element per lane.
//
// Split.  Workgroup: 256 threads = 4 waves as 2 x 2, tile 128 rows x 128
// columns; a wave owns 64 x 64 as 2 x 2 accumulator tiles of
// v_mfma_i32_32x32x32_i8 (64 accumulator registers); two workgroups share a CU
// (launch bounds), so one wave's unpacking overlaps the other's matrix
// instructions.  Grid: one workgroup per (M tile, column tile), the column tile
// fastest -- neighbours share the X tile in L2.  K goes by in steps of 64, two
// matrix instructions deep.
//
// A (activations).  The step's 128 x 64 bytes go through the double-buffered
// LDS tile of tsg_i8frag.h (the piece order, the 80-byte pitch and its bank
// argument are there; the load is i8_apiece's rule), one step ahead, one
// barrier per step.
//
// B (weights).  The packed image (tsg_internal.h) goes from global memory to
// registers: a lane's 16 bytes of a step are one load, a wave's 1 KiB of a step
// contiguous, requested one step ahead.  No index, no LDS.  Each of the four
// dwords unpacks in registers to a fragment of 16 int8 {0x00, 0x01, 0xff} and
// is used for both of the wave's row tiles.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tsg_epilogue.h"
#include "tsg_i8frag.h"
#include "tsg_internal.h"
#include "tsg_ytype.h"

namespace tsg {

template <bool PRELU>
__global__ __launch_bounds__(kI8Threads, 2) void tsg_i8mfma_kernel(
    const int8_t *__restrict__ X, const uint4 *__restrict__ img, const float *__restrict__ b,
    const float *__restrict__ alpha, const float *__restrict__ rs, const float *__restrict__ cs, Epi ep,
    float *__restrict__ Y, int64_t ldY, int ytype, int M, int N, int K, int nks, int ntiles, int xvec)
{
    __shared__ __attribute__((aligned(16))) uint8_t xs[2][kI8TileM * kI8Pitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int nt = blockIdx.x % ntiles, mt = blockIdx.x / ntiles;
    const int m0 = mt * kI8TileM, n0 = nt * kI8TileN;
    const int mw = m0 + 64 * wm, nw = n0 + kI8WaveN * wn;  // the wave's tile
    const bool live = mw < M && nw < N;                     // (uniform) it holds an element of Y
    const uint4 *bw = img + (size_t)(nt * 2 + wn) * nks * 64 + lane;  // the wave's B stream: step ks at bw[64 ks]

    v16i acc[2][2];
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int c2 = 0; c2 < 2; c2++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[rt][c2][r] = 0;

    // the thread's two pieces of a step's A tile (tsg_i8frag.h), global -> registers
    const int8_t *xr[2];
    uint4 areg[2];
#pragma unroll
    for (int j = 0; j < 2; j++) xr[j] = i8_arow(X, m0 + ((tid + kI8Threads * j) >> 2), M, K);
    auto aload = [&](int ks) {
#pragma unroll
        for (int j = 0; j < 2; j++)
            areg[j] = i8_apiece(xr[j], m0 + ((tid + kI8Threads * j) >> 2) < M, ks * kI8KStep + 16 * (tid & 3), K, xvec);
    };
    uint4 bq = make_uint4(0, 0, 0, 0);
    if (nks > 0) {
        bq = bw[0];
        aload(0);
        i8_atile_store(xs[0], areg);
    }
    __syncthreads();
    const int arow = i8_afrag_offset(64 * wm, lane);
    for (int ks = 0; ks < nks; ks++) {
        const bool more = ks + 1 < nks;
        const uint4 bn = bw[(size_t)(more ? ks + 1 : ks) * 64];  // the next step's B, in flight over this one
        if (more) aload(ks + 1);
        if (live) {
            v4i a[2][2];
            i8_afrags(xs[ks & 1] + arow, a);
            const uint32_t bword[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
            for (int c2 = 0; c2 < 2; c2++)
#pragma unroll
                for (int kk = 0; kk < 2; kk++) {
                    const v4i bf = i8_unpack(bword[2 * c2 + kk]);
#pragma unroll
                    for (int rt = 0; rt < 2; rt++)
                        acc[rt][c2] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[rt][kk], bf, acc[rt][c2], 0, 0, 0);
                }
        }
        if (more) i8_atile_store(xs[(ks + 1) & 1], areg);
        bq = bn;
        __syncthreads();  // the next tile is written; this one's reads are done
    }
    if (!live) return;

    const int yt = ytype & kYTypeMask;
    const bool has_rs = rs != nullptr, has_cs = cs != nullptr, epi = (ytype & kYEpi) != 0;
#pragma unroll
    for (int c2 = 0; c2 < 2; c2++) {
        const int n = nw + 32 * c2 + (lane & 31);
        if (n >= N) continue;
        const float bn = b[n], an = PRELU ? alpha[n] : 0.0f, cn = has_cs ? cs[n] : 0.0f;
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int m = mw + 32 * rt + mfma_row(r, lane);
                if (m >= M) continue;
                finish_store1<PRELU>(Y, yt, epi, ldY, ep, m, n, (float)acc[rt][c2][r], has_rs, has_rs ? rs[m] : 0.0f,
                                     has_cs, cn, bn, an);
            }
    }
}

int launch_tcsc_i8mfma(const int8_t *X, const uint32_t *img, int K, const YOut &o)
{
    if (!mfma_grid_ok(o.M, o.N, kI8TileM, kI8TileN, kI8Threads)) return -2;  // (run_mfma refuses it first)
    const int64_t ntiles = (o.N + kI8TileN - 1) / kI8TileN, mtiles = (o.M + kI8TileM - 1) / kI8TileM;
    const dim3 grid((unsigned)(ntiles * mtiles)), block(kI8Threads);
    auto *kernel = o.prelu ? tsg_i8mfma_kernel<true> : tsg_i8mfma_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)o.stream, X, reinterpret_cast<const uint4 *>(img), o.b, o.alpha,
                       o.rs, o.cs, o.ep, static_cast<float *>(o.Y), o.ldY, o.kernel_ytype(false), o.M, o.N, K, i8_nks(K),
                       (int)ntiles, x_vec_ok(X, K, 16));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace tsg
