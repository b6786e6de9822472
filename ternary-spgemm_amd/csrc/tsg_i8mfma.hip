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
// Everything after it is the walks' epilogue, through the shared helpers:
// scale_bias (tsg_scale.h), the PReLU rule, epi_store1 (tsg_epilogue.h) and the
// one rounding of tsg_ytype.h, one element per lane.
//
// Split.  Workgroup: 256 threads = 4 waves as 2 x 2, tile 128 rows x 128
// columns; a wave owns 64 x 64 as 2 x 2 accumulator tiles of
// v_mfma_i32_32x32x32_i8 (64 accumulator registers); two workgroups share a CU
// (launch bounds), so one wave's unpacking overlaps the other's matrix
// instructions.  Grid: one workgroup per (M tile, column tile), the column tile
// fastest -- neighbours share the X tile in L2.  K goes by in steps of 64, two
// matrix instructions deep.
//
// A (activations).  The step's 128 x 64 bytes are loaded by the whole workgroup
// -- thread t the 16-byte pieces t and t + 256, piece p = (row p / 4, k quarter
// p % 4), so four neighbouring lanes read one row's 64 contiguous bytes: one
// 16-byte load each where K % 16 == 0 and X is 16-byte aligned, else byte by
// byte; rows >= M and k >= K are zero and nothing outside [X, X + M K) is
// read -- one step ahead, into registers, and stored to the other half of a
// double-buffered LDS tile after the step's matrix instructions: one barrier
// per step.  LDS row pitch 80 B = 64 + 16.  A fragment read is a ds_read_b128
// of lane l at (row0 + l % 32) * 80 + 32 kk + 16 (l / 32); the LDS serves a
// b128 read 16 lanes at a time (64 banks x 4 B = 16 slots of 16 B), and the 16
// lanes of a group are 16 consecutive rows at one k offset, slot (5 row + c)
// mod 16: 5 is odd, so they fall on 16 distinct slots -- conflict-free.  (The
// stores, rows r .. r + 3 x 4 quarters per group, collide two ways on 3 of 16
// slots; there are 2 per thread and step against 4 fragment reads.)
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
#include "tsg_scale.h"
#include "tsg_ytype.h"

namespace tsg {

namespace {

constexpr int kI8Pitch = kI8KStep + 16;  // LDS bytes per row (header: the bank argument)
constexpr int kI8Threads = 256;

}  // namespace

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

    // the thread's two pieces of a step's A tile, global -> registers ...
    uint4 areg[2];
    auto aload = [&](int ks) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int p = tid + kI8Threads * j, m = m0 + (p >> 2), k = ks * kI8KStep + 16 * (p & 3);
            if (xvec) {  // K % 16 == 0: a piece is inside a row or past its end
                const bool in = m < M && k < K;
                const uint4 v = *reinterpret_cast<const uint4 *>(X + (in ? (size_t)m * K + k : 0));
                areg[j] = in ? v : make_uint4(0, 0, 0, 0);
            } else {
                uint32_t w[4] = {0, 0, 0, 0};
                if (m < M)
                    for (int e = 0; e < 16 && k + e < K; e++)
                        w[e >> 2] |= (uint32_t)(uint8_t)X[(size_t)m * K + k + e] << (8 * (e & 3));
                areg[j] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
    };
    // ... -> the LDS tile `buf`
    auto astore = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int p = tid + kI8Threads * j;
            *reinterpret_cast<uint4 *>(&xs[buf][(p >> 2) * kI8Pitch + 16 * (p & 3)]) = areg[j];
        }
    };

    v16i acc[2][2];
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int c2 = 0; c2 < 2; c2++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[rt][c2][r] = 0;

    uint4 bq = make_uint4(0, 0, 0, 0);
    if (nks > 0) {
        bq = bw[0];
        aload(0);
        astore(0);
    }
    __syncthreads();
    const int arow = (64 * wm + (lane & 31)) * kI8Pitch + 16 * (lane >> 5);
    for (int ks = 0; ks < nks; ks++) {
        const bool more = ks + 1 < nks;
        const uint4 bn = bw[(size_t)(more ? ks + 1 : ks) * 64];  // the next step's B, in flight over this one
        if (more) aload(ks + 1);
        if (live) {
            const uint8_t *xb = xs[ks & 1] + arow;
            v4i a[2][2];
#pragma unroll
            for (int rt = 0; rt < 2; rt++)
#pragma unroll
                for (int kk = 0; kk < 2; kk++)
                    a[rt][kk] = *reinterpret_cast<const v4i *>(xb + 32 * rt * kI8Pitch + 32 * kk);
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
        if (more) astore((ks + 1) & 1);
        bq = bn;
        __syncthreads();  // the next tile is written; this one's reads are done
    }
    if (!live) return;

    // Accumulator register r of a 32 x 32 tile: lanes 0-31 hold the 32 columns
    // of row 8 (r / 4) + r % 4, lanes 32-63 those of the row 4 below -- one
    // coalesced row segment per register and half wave, one element per lane
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
                const int m = mw + 32 * rt + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
                if (m >= M) continue;
                float v = scale_bias((float)acc[rt][c2][r], has_rs, has_rs ? rs[m] : 0.0f, has_cs, cn, bn);
                if (PRELU) v = (v > 0) ? v : an * v;  // comp_prelu.h:57-67
                if (epi)  // a fused epilogue (uniform: the launcher's flag; tsg_epilogue.h)
                    epi_store1(Y, yt, ldY, ep, m, n, v);
                else
                    ystore1_any(Y, yt, (size_t)m * (size_t)ldY + n, v);
            }
    }
}

int launch_tcsc_i8mfma(const int8_t *X, const uint32_t *img, int K, const YOut &o)
{
    const int64_t ntiles = (o.N + kI8TileN - 1) / kI8TileN, mtiles = (o.M + kI8TileM - 1) / kI8TileM;
    if (ntiles * mtiles >= (1ll << 31) / kI8Threads) return -2;  // (run_i8 refuses it first)
    const int nks = (K + kI8KStep - 1) / kI8KStep;
    const int xvec = K > 0 && K % 16 == 0 && ((uintptr_t)X & 15) == 0;
    const dim3 grid((unsigned)(ntiles * mtiles)), block(kI8Threads);
    auto *kernel = o.prelu ? tsg_i8mfma_kernel<true> : tsg_i8mfma_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)o.stream, X, reinterpret_cast<const uint4 *>(img), o.b, o.alpha,
                       o.rs, o.cs, o.ep, static_cast<float *>(o.Y), o.ldY, o.kernel_ytype(false), o.M, o.N, K, nks,
                       (int)ntiles, xvec);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace tsg
