// tcsc_kernels.hip -- the compiled-in gfx950 kernels of libternary_spgemm.so
// (the default weight-compiled kernel is a separate code object,
// tsg_jit_kernel.hip + tsg_jit.cpp).
//
// Arithmetic contract (cpp_impl/comp.h:37-63, BaseTCSC<float>): every output
// Y[m,n] is ONE serial fp32 chain  0 + x_p1 + ... + x_pP - x_n1 - ... - x_nQ,
// then + b[n], with the +1 run and the -1 run each in ascending k.  No output
// is ever split across lanes/waves: parallelism is over (m, n) pairs only.
//
// tsg_transpose_kernel / tsg_transpose4_kernel (K % 4 == 0):
//   X [M][K] -> X^T [Kp][Mp], zero padded.  HBM-bound copy (2 * 4 * M * K bytes).
// Every staging pass is a template on X's element type T (float, xf16, xbf16,
// xi8; tsg_xtype.h): it reads T through xload1 / xload4, which widen to fp32,
// and writes the same fp32 layout whatever T is -- so the kernels that consume
// the staged copy never see the type.  The vector forms read one quad (four
// consecutive k of a row) per load: 16 B of fp32, 8 B of a 16-bit type, 4 B of
// int8; they need X aligned to 4 elements and K % 4 == 0 (x_quad_aligned).
// Every staging pass is also a template on Q: an actquant call's pass
// quantises each value it loads, xquant(v, inv[m]) (tsg_actquant.h), with
// inv[m] from tsg_row_absmax_kernel, the row pass that runs before it; a
// normquant call's pass normalises first, xquant(xnorm(v, rn[m], g[k]), inv[m])
// (tsg_norm.h), with rn[m] from the same row pass.  Q is an XStage; kStageNone
// is the pass as it was.
// tsg_tcsc_rx_kernel: the register-X walk, the fallback when a W is too large
//   for one weight-compiled image (> ~300 M nonzeros on one handle) or the
//   generated image cannot be loaded (tsg_capi.cpp create_impl).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "tsg_actquant.h"
#include "tsg_epilogue.h"
#include "tsg_internal.h"
#include "tsg_norm.h"
#include "tsg_scale.h"
#include "tsg_xtype.h"
#include "tsg_ytype.h"

namespace tsg {

// ------------------------------------------------------------------ kernel 1 --
template <typename T, int Q>
__global__ __launch_bounds__(256) void tsg_transpose_kernel(const T *__restrict__ X,
                                                            float *__restrict__ XT, int M, int K,
                                                            int Mp, int Kp, const float *__restrict__ inv,
                                                            const float *__restrict__ rn, const float *__restrict__ g)
{
    __shared__ float tile[64][65];
    const int k0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 64 x 4
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int m = m0 + ty + 4 * i, k = k0 + tx;
        float v = (m < M && k < K) ? xload1(X + (size_t)m * K + k) : 0.0f;
        if (Q && m < M) v = xstage<Q>(v, m, k, K, inv, rn, g);
        tile[ty + 4 * i][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int k = k0 + ty + 4 * i, m = m0 + tx;
        if (k < Kp) XT[(size_t)k * Mp + m] = tile[tx][ty + 4 * i];
    }
}

// Same transpose with a quad per load and 16-byte stores (K % 4 == 0 and X
// aligned to 4 elements): each lane loads 4 consecutive k of one m row and stores 4
// consecutive m of one X^T row -- a quarter of the memory instructions.
template <typename T, int Q>
__global__ __launch_bounds__(256) void tsg_transpose4_kernel(const T *__restrict__ X,
                                                             float *__restrict__ XT, int M, int K,
                                                             int Mp, int Kp, const float *__restrict__ inv,
                                                             const float *__restrict__ rn, const float *__restrict__ g)
{
    __shared__ float tile[64][65];
    const int k0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
    const int c4 = (threadIdx.x & 15) * 4, r = threadIdx.x >> 4;  // 16 x 16
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int ml = r + 16 * i, m = m0 + ml, k = k0 + c4;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (m < M && k < K) {
            v = xload4(X + (size_t)m * K + k);  // K % 4 == 0
            if (Q) v = xstage4<Q>(v, m, k, K, inv, rn, g);
        }
        tile[ml][c4] = v.x;
        tile[ml][c4 + 1] = v.y;
        tile[ml][c4 + 2] = v.z;
        tile[ml][c4 + 3] = v.w;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int kl = r + 16 * i, k = k0 + kl;
        if (k < Kp)
            *reinterpret_cast<float4 *>(XT + (size_t)k * Mp + m0 + c4) =
                make_float4(tile[c4][kl], tile[c4 + 1][kl], tile[c4 + 2][kl], tile[c4 + 3][kl]);
    }
}

// X [M][K] -> the k-pair layout of the jit kernel (tsg_internal.h): for k-row
// pair p and M-row pair mp the 16 bytes at (p * Mp/2 + mp) * 16 hold
// X[2mp][2p], X[2mp+1][2p], X[2mp][2p+1], X[2mp+1][2p+1]; zero outside M x K.
// A 64 (m) x 64 (k) tile goes through LDS: loads along k (16 B per lane when
// VEC: K % 4 == 0 and X aligned to 4 elements), stores 16 B per lane, consecutive
// lanes on consecutive mp (coalesced 512-B runs per pair row).  HBM-bound:
// 8 * M * K bytes.
template <typename T, bool VEC, int Q>
__global__ __launch_bounds__(256) void tsg_transpose_pairs_kernel(const T *__restrict__ X,
                                                                  float *__restrict__ XP, int M, int K,
                                                                  int Mp, int Kp, const float *__restrict__ inv,
                                                                  const float *__restrict__ rn, const float *__restrict__ g)
{
    __shared__ float tile[64][65];  // [m][k]
    const int k0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
    if (VEC) {
        const int c4 = (threadIdx.x & 15) * 4, r = threadIdx.x >> 4;  // 16 x 16
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int ml = r + 16 * i, m = m0 + ml, k = k0 + c4;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (m < M && k < K) {
            v = xload4(X + (size_t)m * K + k);  // K % 4 == 0
            if (Q) v = xstage4<Q>(v, m, k, K, inv, rn, g);
        }
            tile[ml][c4] = v.x;
            tile[ml][c4 + 1] = v.y;
            tile[ml][c4 + 2] = v.z;
            tile[ml][c4 + 3] = v.w;
        }
    } else {
        const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 64 x 4
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int m = m0 + ty + 4 * i, k = k0 + tx;
            float v = (m < M && k < K) ? xload1(X + (size_t)m * K + k) : 0.0f;
            if (Q && m < M) v = xstage<Q>(v, m, k, K, inv, rn, g);
            tile[ty + 4 * i][tx] = v;
        }
    }
    __syncthreads();
    // 32 pairs x 32 M pairs of float4 per tile: 4 per thread
    const int mpl = threadIdx.x & 31, pl0 = threadIdx.x >> 5;  // 32 x 8
    const size_t half_mp = (size_t)Mp / 2;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int pl = pl0 + 8 * i, p = (k0 >> 1) + pl;
        if (2 * p >= Kp) continue;
        const int a = 2 * mpl, kk = 2 * pl;
        *reinterpret_cast<float4 *>(XP + ((size_t)p * half_mp + (size_t)(m0 >> 1) + mpl) * 4) =
            make_float4(tile[a][kk], tile[a + 1][kk], tile[a][kk + 1], tile[a + 1][kk + 1]);
    }
}

// X [M][K] -> the blocked k-quad layout of the 64-row image (tsg_internal.h),
// PR rows per piece (16 or 8) and QP = 64 / PR quads: the 1-KiB piece pr = QP qg
// + rg of (chunk c, M tile t) at ((c * Mt + t) * U + pr) KiB (U = 48 units per
// chunk, 24 for the half ring) holds, in 16-B
// lane slot j, X[64 t + PR rg + j % PR][4 (48 c + QP qg + j / PR) .. +3] -- zero
// past M or K -- so the kernel's DMA pieces are coalesced 1-KiB reads.  Every
// slot is 16 contiguous bytes of a row of X, so this is a gather-copy, not a
// transpose: one wave writes one whole piece (1 KiB, one store per lane) from
// PR row segments of 1024 / PR bytes (the other half of a PR = 16 segment's
// 128-B line is the next piece's, copied by the neighbouring workgroup); no
// LDS, no barrier.  A workgroup copies 4 consecutive pieces of one (chunk, M
// tile).  HBM-bound: 8 * Mp * Kp bytes.
template <typename T, bool VEC, int PR, int Q>
__global__ __launch_bounds__(256) void tsg_transpose_quads_kernel(const T *__restrict__ X,
                                                                  float *__restrict__ XQ, int M, int K,
                                                                  int Mp, int Kp, int units,
                                                                  const float *__restrict__ inv,
                                                                  const float *__restrict__ rn, const float *__restrict__ g)
{
    // units: 1-KiB pieces per (chunk, M tile) -- 48, or 24 for the half ring
    constexpr int QP = 64 / PR;
    const int Mt = Mp >> 6, nch = Kp / (4 * units), groups = units / 4;
    // workgroup order (M tile * nch + chunk) * 12 + piece group: the workgroups
    // in flight read a few M tiles' rows end to end (long runs of each row), not
    // one chunk of every row
    const int blk = blockIdx.x;
    const int tc = blk / groups, pr = (blk % groups) * 4 + (threadIdx.x >> 6);
    const int t = tc / nch, c = tc % nch, j = threadIdx.x & 63;
    const int ct = c * Mt + t;
    const int qg = pr / QP, rg = pr % QP;
    const int m = 64 * t + PR * rg + (j % PR);
    const int k = 4 * (units * c + QP * qg + j / PR);
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (m < M) {
        const T *row = X + (size_t)m * K;
        if (VEC) {
            if (k < K) v = xload4(row + k);  // K % 4 == 0: whole quad inside
        } else {
            if (k < K) v.x = xload1(row + k);
            if (k + 1 < K) v.y = xload1(row + k + 1);
            if (k + 2 < K) v.z = xload1(row + k + 2);
            if (k + 3 < K) v.w = xload1(row + k + 3);
        }
        // (a slot past K holds +0, and xquant(+0) is +0)
        if (Q) v = xstage4<Q>(v, m, k, K, inv, rn, g);
    }
    *reinterpret_cast<float4 *>(XQ + ((size_t)ct * units + pr) * 256 + (size_t)j * 4) = v;
}

// X [M][K] -> the staged copy of the 64-row image's ROW layout
// (tsg_internal.h kJit64RowFlag): (chunk c, M tile t) is 47 KiB at (c * Mt +
// t) * 47 KiB, rows of 47 quads (752 B) -- row r holds X[64 t + r][kb .. kb +
// 187], kb = c * 188 (the last chunk: K - 188 when K >= 188 and K % 4 == 0,
// jit64_row_kbase), zero past M and K.  Each 16-B slot is 16 contiguous bytes
// of a row of X, so this is a gather-copy of row runs (no transpose): reads
// and writes both run along rows.  Four workgroups per (chunk, M tile), 752
// slots each.  HBM-bound: 2 * 4 * Mp * Kp bytes.
template <typename T, bool VEC, int Q>
__global__ __launch_bounds__(256) void tsg_transpose_rows_kernel(const T *__restrict__ X,
                                                                 float *__restrict__ XR, int M, int K, int Mp,
                                                                 int nch, const float *__restrict__ inv,
                                                                 const float *__restrict__ rn, const float *__restrict__ g)
{
    constexpr int kQ = 47, kSlots = 64 * kQ, kPer = kSlots / 4;  // 752 slots per workgroup
    const int Mt = Mp >> 6;
    const int blk = blockIdx.x, part = blk & 3, tc = blk >> 2;
    // workgroup order (M tile * nch + chunk) * 4 + part: the workgroups in
    // flight read a few M tiles' rows end to end
    const int t = tc / nch, c = tc % nch;
    const int kb = (c == nch - 1 && K >= 4 * kQ && (K & 3) == 0) ? K - 4 * kQ : c * 4 * kQ;
    float *dst = XR + ((size_t)c * Mt + t) * (kSlots * 4);
    for (int i = threadIdx.x; i < kPer; i += 256) {
        const int slot = part * kPer + i, r = slot / kQ, q = slot % kQ;
        const int m = 64 * t + r, k = kb + 4 * q;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (m < M) {
            const T *row = X + (size_t)m * K;
            if (VEC) {
                if (k < K) v = xload4(row + k);  // K % 4 == 0: whole quad inside
            } else {
                if (k < K) v.x = xload1(row + k);
                if (k + 1 < K) v.y = xload1(row + k + 1);
                if (k + 2 < K) v.z = xload1(row + k + 2);
                if (k + 3 < K) v.w = xload1(row + k + 3);
            }
            if (Q) v = xstage4<Q>(v, m, k, K, inv, rn, g);
        }
        *reinterpret_cast<float4 *>(dst + (size_t)slot * 4) = v;
    }
}

// The row pass of an actquant call (tsg_actquant.h): one wave per row of X,
// four rows per workgroup.  Each lane keeps fmaxf(fabsf()) of the elements it
// loads (a quad per load when VEC: K % 4 == 0 and X aligned to 4 elements), an
// xor butterfly leaves the row's maximum in every lane (max is exact and
// associative: the reduction's shape does not matter, and a NaN is never the
// larger operand), and lane 0 stores inv[m], deq[m] and, when given, out[m].
// Q8: the call runs a small-M walk, which reads X in place -- every lane then
// reads its elements again (still in cache) and stores q as int8, row-major
// [M][K], four per store when VEC (q8 is aligned to 4 B and K % 4 == 0); the
// walk runs on q8 as an int8-X scaled call.  K = 0: no loads, amax = 0.
// NORM: the row pass of a normquant call (tsg_norm.h).  A sweep in front
// accumulates the row's 256 strided partial sums of squares -- with quad loads
// lane l holds partials 4l .. 4l + 3, with scalar loads partials l + 64 j, j =
// 0..3 -- and reduces them by the contract's tree, neighbours first: the in-lane
// adds are levels 0 and 1 and the xor butterfly over lanes 1, 2, .., 32 levels 2
// to 7 (quads), or the butterfly on each accumulator levels 0 to 5 and (j0 + j1)
// + (j2 + j3) levels 6 and 7 (scalars).  An absent element adds nothing, so
// both give the same bits.  The maximum and q are then taken of xn = xnorm(x,
// rn, g[k]), and lane 0 also stores rn[m].  K = 0: no sum, no division.
template <typename T, bool VEC, bool Q8, bool NORM>
__global__ __launch_bounds__(256) void tsg_row_absmax_kernel(const T *__restrict__ X, int M, int K,
                                                             float *__restrict__ inv, float *__restrict__ deq,
                                                             float *__restrict__ out, int8_t *__restrict__ q8,
                                                             float *__restrict__ rnorm, const float *__restrict__ g,
                                                             float eps)
{
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;  // (whole waves: no barrier follows)
    const T *row = X + (size_t)m * K;
    float rn = 0.0f;
    if (NORM && K > 0) {
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f, ss;
        if (VEC) {
            for (int k = 4 * lane; k < K; k += 256) {
                const float4 v = xload4(row + k);
                s0 = norm_sq_add(s0, v.x);
                s1 = norm_sq_add(s1, v.y);
                s2 = norm_sq_add(s2, v.z);
                s3 = norm_sq_add(s3, v.w);
            }
            ss = (s0 + s1) + (s2 + s3);
#pragma unroll
            for (int d = 1; d <= 32; d <<= 1) ss = ss + __shfl_xor(ss, d, 64);
        } else {
            for (int k = lane; k < K; k += 256) {
                s0 = norm_sq_add(s0, xload1(row + k));
                if (k + 64 < K) s1 = norm_sq_add(s1, xload1(row + k + 64));
                if (k + 128 < K) s2 = norm_sq_add(s2, xload1(row + k + 128));
                if (k + 192 < K) s3 = norm_sq_add(s3, xload1(row + k + 192));
            }
#pragma unroll
            for (int d = 1; d <= 32; d <<= 1) {
                s0 = s0 + __shfl_xor(s0, d, 64);
                s1 = s1 + __shfl_xor(s1, d, 64);
                s2 = s2 + __shfl_xor(s2, d, 64);
                s3 = s3 + __shfl_xor(s3, d, 64);
            }
            ss = (s0 + s1) + (s2 + s3);
        }
        rn = norm_rn(ss, K, eps);
    }
    float amax = 0.0f;
    if (VEC) {
        for (int k = 4 * lane; k < K; k += 256) {
            float4 v = xload4(row + k);
            if (NORM) {
                const float4 gv = gload4(g, k, K);
                v = make_float4(xnorm(v.x, rn, gv.x), xnorm(v.y, rn, gv.y), xnorm(v.z, rn, gv.z), xnorm(v.w, rn, gv.w));
            }
            amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
        }
    } else {
        for (int k = lane; k < K; k += 64) {
            float v = xload1(row + k);
            if (NORM) v = xnorm(v, rn, gload1(g, k, K));
            amax = fmaxf(amax, fabsf(v));
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) amax = fmaxf(amax, __shfl_xor(amax, d, 64));
    float iv, dq;
    actquant_scales(amax, iv, dq);
    if (lane == 0) {
        inv[m] = iv;
        deq[m] = dq;
        if (out) out[m] = dq;
        if (NORM) rnorm[m] = rn;
    }
    if (Q8) {
        int8_t *qrow = q8 + (size_t)m * K;
        if (VEC) {
            for (int k = 4 * lane; k < K; k += 256) {
                float4 v = xload4(row + k);
                if (NORM) {
                    const float4 gv = gload4(g, k, K);
                    v = make_float4(xnormquant(v.x, rn, gv.x, iv), xnormquant(v.y, rn, gv.y, iv),
                                    xnormquant(v.z, rn, gv.z, iv), xnormquant(v.w, rn, gv.w, iv));
                } else {
                    v = xquant4(v, iv);
                }
                const uint32_t w = ((uint32_t)(int)v.x & 0xffu) | (((uint32_t)(int)v.y & 0xffu) << 8) |
                                   (((uint32_t)(int)v.z & 0xffu) << 16) | ((uint32_t)(int)v.w << 24);
                *reinterpret_cast<uint32_t *>(qrow + k) = w;
            }
        } else {
            for (int k = lane; k < K; k += 64) {
                const float v = xload1(row + k);
                qrow[k] = (int8_t)(int)(NORM ? xnormquant(v, rn, gload1(g, k, K), iv) : xquant(v, iv));
            }
        }
    }
}

// One LDS-DMA piece: 64 lanes x 16 B from per-lane global addresses to LDS
// [lds_dst, lds_dst + 1 KiB).  Inline asm on purpose: hipcc cannot prove that
// later ds_reads do not alias an in-flight LDS-DMA and would put
// `s_waitcnt vmcnt(0)` in front of the first one (serialising the prefetch).
// The kernel waits for these itself (vmcnt(0) before each step's barrier);
// M0 is set and restored inside the statement (cdna_hip_programming.md 5.7).
__device__ __forceinline__ void glds16(const void *gsrc, uint32_t lds_dst)
{
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(gsrc), "s"(lds_dst)
        : "memory");
}


// ------------------------------------------------------------ rx kernel --
// Register-X walk (see tsg_internal.h "rx"): the block's X rows live in
// VGPRs and each entry is a SRC1-relative v_pk_add pair; no LDS read per
// entry.  The block loop is generated inline asm (gen_rx_asm.py).
#ifdef TSG_RX_INC
#include TSG_RX_INC  // diagnostic variant of the generated walk
#else
#include "tsg_rx_asm.inc"
#endif
#define TSG_RX_CAT2(a, b) a##b
#define TSG_RX_CAT(a, b) TSG_RX_CAT2(a, b)

typedef float F32x32 __attribute__((ext_vector_type(32)));

template <bool NEG>
__device__ __forceinline__ void rx_walk(F32x32 &a0, F32x32 &a1, F32x32 &a2, F32x32 &a3,
                                        const uint32_t *base, uint32_t &off, uint32_t &hdr,
                                        uint32_t xb)
{
    uint32_t t, nhdr, m0s;
    if constexpr (NEG)
        asm volatile(TSG_RX_CAT(TSG_RX_WALK_NEG_R, TSG_RX_ROWS)
                     : "+{v[112:143]}"(a0), "+{v[144:175]}"(a1), "+{v[176:207]}"(a2),
                       "+{v[208:239]}"(a3), [off] "+s"(off), [hdr] "+s"(hdr), [t] "=&s"(t),
                       [nhdr] "=&s"(nhdr), [m0s] "=&s"(m0s)
                     : [base] "s"(base), [xb] "v"(xb)
                     : TSG_RX_CAT(TSG_RX_CLOBBERS_R, TSG_RX_ROWS));
    else
        asm volatile(TSG_RX_CAT(TSG_RX_WALK_POS_R, TSG_RX_ROWS)
                     : "+{v[112:143]}"(a0), "+{v[144:175]}"(a1), "+{v[176:207]}"(a2),
                       "+{v[208:239]}"(a3), [off] "+s"(off), [hdr] "+s"(hdr), [t] "=&s"(t),
                       [nhdr] "=&s"(nhdr), [m0s] "=&s"(m0s)
                     : [base] "s"(base), [xb] "v"(xb)
                     : TSG_RX_CAT(TSG_RX_CLOBBERS_R, TSG_RX_ROWS));
}

// X^T chunk j (kRxChunk rows x 256 M) -> LDS buffer buf: one 1 KiB row per
// wave-instruction, 8 per wave.
__device__ __forceinline__ void rx_stage(const float *__restrict__ XT, int Mp, int m0, int j, int buf,
                                         int wave, int lane)
{
#pragma unroll
    for (int i = 0; i < kRxChunk / kRxWaves; i++) {
        const int r = wave * (kRxChunk / kRxWaves) + i;
        glds16(XT + (size_t)(j * kRxChunk + r) * Mp + m0 + 4 * lane, (uint32_t)(buf * kRxChunkBytes + r * 1024));
    }
}

template <bool PRELU>
__global__ __launch_bounds__(kRxWaves * 64, 8 / kRxWaves) void tsg_tcsc_rx_kernel(
    const float *__restrict__ XT, int Mp, const uint32_t *__restrict__ wstart,
    const uint32_t *__restrict__ ent, const float *__restrict__ b, const float *__restrict__ alpha,
    float *__restrict__ Y, int64_t ldY, int ytype, int M, int N, int nch, int mtiles, int ntiles,
    const float *__restrict__ rs, const float *__restrict__ cs, Epi ep)
{
    __shared__ __attribute__((aligned(16))) char lds[kRxLdsBytes];
    const int tid = threadIdx.x, lane = tid & 63;
    // LDS is only touched from asm (LDS-DMA, ds_read_b128 at absolute offsets
    // from 0): a never-taken C++ store keeps the allocation in the kernel
    if (M < 0) lds[tid] = 0;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // XCD-aware bijective remap: each XCD gets a contiguous run of workgroups
    const int T = mtiles * ntiles, L = blockIdx.x;
    const int xcd = L & 7, slot = L >> 3, q8 = T >> 3, r8 = T & 7;
    const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
    // n-tile-major: the concurrent workgroups of an XCD share few column
    // tiles, so their entry streams (latency-critical scalar loads) stay in
    // that XCD's L2; X^T chunks arrive by LDS-DMA a whole step ahead.
    const int nt = wg / mtiles, mt = wg - nt * mtiles;
    const int m0 = mt * kRxTileM;
    const int ncol0 = nt * kRxTileCols + wave * kRxNW;

    // the walk addresses its stream as ent + off (bytes; SMEM base + SGPR offset)
    uint32_t off = 4u * __builtin_amdgcn_readfirstlane(wstart[(size_t)nt * kRxWaves + wave]);
    uint32_t hdr = __builtin_amdgcn_readfirstlane(ent[off / 4]);
    rx_stage(XT, Mp, m0, 0, 0, wave, lane);
    F32x32 a0 = {}, a1 = {}, a2 = {}, a3 = {};  // comp.h:41
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // two loops (not one with a branch per step: a uniform if/else between
    // the two walks trips hipcc's SGPR-copy fixup on the asm operands)
    const int steps = 2 * nch;
    for (int q = 0; q < nch; q++) {  // +1 runs, ascending K
        if (q + 1 < steps) rx_stage(XT, Mp, m0, (q + 1) % nch, (q + 1) & 1, wave, lane);
        rx_walk<false>(a0, a1, a2, a3, ent, off, hdr, (uint32_t)(q & 1) * (uint32_t)kRxChunkBytes + (uint32_t)lane * 16u);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    for (int q = nch; q < steps; q++) {  // -1 runs, ascending K
        if (q + 1 < steps) rx_stage(XT, Mp, m0, (q + 1) % nch, (q + 1) & 1, wave, lane);
        rx_walk<true>(a0, a1, a2, a3, ent, off, hdr, (uint32_t)(q & 1) * (uint32_t)kRxChunkBytes + (uint32_t)lane * 16u);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    if (ncol0 >= N) return;
    if (((rs != nullptr) | (cs != nullptr)) && !(ytype & kYEpi)) {
        // a scaled call (uniform; tsg_scale.h): ((chain * rs[m]) * cs[n]) + b[n],
        // three roundings, then the PReLU and the store of any Y type
        // (one with a fused epilogue too goes to that branch, below)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int m = m0 + 4 * lane + r;
            if (m >= M) continue;
            // this branch's own copies, fenced like the 16-bit branch's
            int nc0 = ncol0;
            const float *bs = b, *alphas = alpha, *rss = rs, *css = cs;
            asm volatile("" : "+s"(nc0), "+s"(bs), "+s"(alphas), "+s"(rss), "+s"(css));
            const bool has_rs = rss != nullptr, has_cs = css != nullptr;
            const float rm = has_rs ? rss[m] : 0.0f;
            ystore_seg_any<kRxNW>(Y, ytype, (size_t)m * (size_t)ldY + nc0, N - nc0, [&](int c) {
                const int n = nc0 + c < N ? nc0 + c : N - 1;
                const float acc = c < 8 ? a0[4 * (c & 7) + r] : c < 16 ? a1[4 * (c & 7) + r]
                                 : c < 24 ? a2[4 * (c & 7) + r] : a3[4 * (c & 7) + r];
                float y = scale_bias(acc, has_rs, rm, has_cs, has_cs ? css[n] : 0.0f, bs[n]);
                if (PRELU) y = (y > 0) ? y : alphas[n] * y;  // comp_prelu.h:57-67
                return y;
            });
        }
        return;
    }
    if (ytype != kYF32) {
        if (ytype & kYEpi) {
            // a call with a fused epilogue (uniform: the launcher's flag;
            // tsg_epilogue.h): the scaled value (a missing scale's multiply not
            // performed), the PReLU, then per group of 8 columns the lane's
            // own gate and residual elements, ReLU / ReLU^2, * gate, +
            // residual, and the store of any Y type
            const int yt = ytype & kYTypeMask;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int m = m0 + 4 * lane + r;
                if (m >= M) continue;
                int nc0 = ncol0;
                const float *bs = b, *alphas = alpha, *rss = rs, *css = cs;
                asm volatile("" : "+s"(nc0), "+s"(bs), "+s"(alphas), "+s"(rss), "+s"(css));
                const bool has_rs = rss != nullptr, has_cs = css != nullptr;
                const float rm = has_rs ? rss[m] : 0.0f;
                ystore_seg_epi<kRxNW>(Y, yt, ldY, ep, m, nc0, N - nc0, [&](int c) {
                    const int n = nc0 + c < N ? nc0 + c : N - 1;
                    const float acc = c < 8 ? a0[4 * (c & 7) + r] : c < 16 ? a1[4 * (c & 7) + r]
                                     : c < 24 ? a2[4 * (c & 7) + r] : a3[4 * (c & 7) + r];
                    float y = scale_bias(acc, has_rs, rm, has_cs, has_cs ? css[n] : 0.0f, bs[n]);
                    if (PRELU) y = (y > 0) ? y : alphas[n] * y;  // comp_prelu.h:57-67
                    return y;
                });
            }
            return;
        }
        // a 16-bit Y (uniform): the same fp32 value, rounded once and stored
        // 8 columns at a time (tsg_ytype.h); ldY counts 16-bit elements
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int m = m0 + 4 * lane + r;
            if (m >= M) continue;
            // this branch's own copies of what the fp32 stores below use too
            // (else the compiler computes every column's bias address once for
            // both branches, ahead of them, in scalar registers it must spill)
            int nc0 = ncol0;
            const float *b16 = b, *alpha16 = alpha;
            asm volatile("" : "+s"(nc0), "+s"(b16), "+s"(alpha16));
            ystore_seg<kRxNW>(Y, ytype, (size_t)m * (size_t)ldY + nc0, N - nc0, [&](int c) {
                const int n = nc0 + c < N ? nc0 + c : N - 1;
                const float acc = c < 8 ? a0[4 * (c & 7) + r] : c < 16 ? a1[4 * (c & 7) + r]
                                 : c < 24 ? a2[4 * (c & 7) + r] : a3[4 * (c & 7) + r];
                float y = acc + b16[n];                       // comp.h:63
                if (PRELU) y = (y > 0) ? y : alpha16[n] * y;  // comp_prelu.h:57-67
                return y;
            });
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int m = m0 + 4 * lane + r;
        if (m >= M) continue;
        float *yrow = Y + (size_t)m * (size_t)ldY + ncol0;  // ldY >= N floats per Y row
        float v[kRxNW];
#pragma unroll
        for (int c = 0; c < kRxNW; c++) {
            const int n = ncol0 + c < N ? ncol0 + c : N - 1;
            const float acc = c < 8 ? a0[4 * (c & 7) + r] : c < 16 ? a1[4 * (c & 7) + r]
                             : c < 24 ? a2[4 * (c & 7) + r] : a3[4 * (c & 7) + r];
            float y = acc + b[n];                       // comp.h:63
            if (PRELU) y = (y > 0) ? y : alpha[n] * y;  // comp_prelu.h:57-67
            v[c] = y;
        }
        if (ncol0 + kRxNW <= N && (((uintptr_t)yrow & 15) == 0)) {  // float4 stores need 16-B alignment
#pragma unroll
            for (int c = 0; c < kRxNW; c += 4)
                *reinterpret_cast<float4 *>(yrow + c) = make_float4(v[c], v[c + 1], v[c + 2], v[c + 3]);
        } else {
#pragma unroll
            for (int c = 0; c < kRxNW; c++)
                if (ncol0 + c < N) yrow[c] = v[c];
        }
    }
}

// ---------------------------------------------------------------- launchers --
// Calls launch(x, std::integral_constant<int, Q>) with x = X as its element
// type and Q = what the staging pass does to the values it loads (XStage,
// tsg_norm.h): quantise when inv is given, normalise first when rn is given
// too; 0 when the launch went through.  An int8 X is never quantised (the
// C-ABI refuses it), so those combinations are not instantiated.
template <typename F>
int stage_launch(const XIn &in, F &&launch)
{
    return with_xtype(in.X, in.xtype, [&](auto *x) {
        auto go = [&](auto q) { return launch(x, q), hipGetLastError() == hipSuccess ? 0 : -1; };
        if (!in.inv) return go(std::integral_constant<int, kStageNone>{});
        if constexpr (std::is_same_v<decltype(x), const xi8 *>) return -1;
        else return in.rn ? go(std::integral_constant<int, kStageNorm>{}) : go(std::integral_constant<int, kStageQuant>{});
    });
}

// whether a staging pass may load X a quad at a time
static bool quad_loads(const XIn &in) { return in.K % 4 == 0 && x_quad_aligned(in.X, in.xtype); }

int launch_transpose(const XIn &in, float *XT, int Mp, int Kp, void *stream)
{
    dim3 grid((unsigned)((Kp + 63) / 64), (unsigned)(Mp / 64));
    const bool vec = quad_loads(in);
    return stage_launch(in, [&](auto *x, auto q) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(x)>>;
        constexpr int Q = decltype(q)::value;
        if (vec)
            hipLaunchKernelGGL((tsg_transpose4_kernel<T, Q>), grid, dim3(256), 0, (hipStream_t)stream, x, XT, in.M, in.K,
                               Mp, Kp, in.inv, in.rn, in.g);
        else
            hipLaunchKernelGGL((tsg_transpose_kernel<T, Q>), grid, dim3(256), 0, (hipStream_t)stream, x, XT, in.M, in.K,
                               Mp, Kp, in.inv, in.rn, in.g);
    });
}

int launch_transpose_pairs(const XIn &in, float *XP, int Mp, int Kp, void *stream)
{
    // Mp is a multiple of 128 (the jit M tile) and Kp of 96: the 64 x 64 tiles
    // cover [0, Kp) x [0, Mp) exactly in m and up to 32 pad rows in k
    dim3 grid((unsigned)((Kp + 63) / 64), (unsigned)(Mp / 64));
    const bool vec = quad_loads(in);
    return stage_launch(in, [&](auto *x, auto q) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(x)>>;
        constexpr int Q = decltype(q)::value;
        if (vec)
            hipLaunchKernelGGL((tsg_transpose_pairs_kernel<T, true, Q>), grid, dim3(256), 0, (hipStream_t)stream, x, XP,
                               in.M, in.K, Mp, Kp, in.inv, in.rn, in.g);
        else
            hipLaunchKernelGGL((tsg_transpose_pairs_kernel<T, false, Q>), grid, dim3(256), 0, (hipStream_t)stream, x, XP,
                               in.M, in.K, Mp, Kp, in.inv, in.rn, in.g);
    });
}

int launch_transpose_quads(const XIn &in, float *XQ, int Mp, int Kp, int piece_rows, int chunk, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const bool vec = quad_loads(in);
    if (piece_rows == 0) {  // the row layout: 188-row chunks, 47 KiB per (chunk, M tile)
        if (chunk != 188 || Mp % 64 || Kp % 188) return -1;
        const int nch = Kp / 188;
        const int64_t blocks = (int64_t)nch * (Mp / 64) * 4;
        if (blocks >= ((int64_t)1 << 31)) return -1;
        return stage_launch(in, [&](auto *x, auto q) {
            using T = std::remove_cv_t<std::remove_pointer_t<decltype(x)>>;
            constexpr int Q = decltype(q)::value;
            if (vec) hipLaunchKernelGGL((tsg_transpose_rows_kernel<T, true, Q>), dim3((unsigned)blocks), dim3(256), 0, s, x, XQ, in.M, in.K, Mp, nch, in.inv, in.rn, in.g);
            else hipLaunchKernelGGL((tsg_transpose_rows_kernel<T, false, Q>), dim3((unsigned)blocks), dim3(256), 0, s, x, XQ, in.M, in.K, Mp, nch, in.inv, in.rn, in.g);
        });
    }
    // Mp is a multiple of 64 (the 64-row image's M tile) and Kp of 192 (its
    // chunk): the pieces cover [0, Kp) x [0, Mp) exactly
    if ((chunk != 192 && chunk != 96) || Mp % 64 || Kp % chunk) return -1;
    // chunk / 16 workgroups of 4 pieces per (chunk, M tile)
    const int units = chunk / 4;
    const int64_t blocks = (int64_t)(Kp / chunk) * (Mp / 64) * (units / 4);
    if (blocks >= ((int64_t)1 << 31)) return -1;
    if (piece_rows != 16 && piece_rows != 8) return -1;
    dim3 grid((unsigned)blocks);
    return stage_launch(in, [&](auto *x, auto q) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(x)>>;
        constexpr int Q = decltype(q)::value;
        if (piece_rows == 16) {
            if (vec) hipLaunchKernelGGL((tsg_transpose_quads_kernel<T, true, 16, Q>), grid, dim3(256), 0, s, x, XQ, in.M, in.K, Mp, Kp, units, in.inv, in.rn, in.g);
            else hipLaunchKernelGGL((tsg_transpose_quads_kernel<T, false, 16, Q>), grid, dim3(256), 0, s, x, XQ, in.M, in.K, Mp, Kp, units, in.inv, in.rn, in.g);
        } else {
            if (vec) hipLaunchKernelGGL((tsg_transpose_quads_kernel<T, true, 8, Q>), grid, dim3(256), 0, s, x, XQ, in.M, in.K, Mp, Kp, units, in.inv, in.rn, in.g);
            else hipLaunchKernelGGL((tsg_transpose_quads_kernel<T, false, 8, Q>), grid, dim3(256), 0, s, x, XQ, in.M, in.K, Mp, Kp, units, in.inv, in.rn, in.g);
        }
    });
}

// (tsg_internal.h; an int8 X is refused: -1)
int launch_row_absmax(const XIn &in, float *deq, float *out, int8_t *q8, float eps, void *stream)
{
    if (in.M <= 0) return 0;
    if (in.xtype == kXI8) return -1;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = quad_loads(in);
    const dim3 grid((unsigned)((in.M + 3) / 4));
    return with_xtype(in.X, in.xtype, [&](auto *x) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(x)>>;
        if constexpr (std::is_same_v<T, xi8>) {
            return -1;
        } else {
            auto go = [&](auto v, auto q, auto n) {
                hipLaunchKernelGGL((tsg_row_absmax_kernel<T, decltype(v)::value, decltype(q)::value, decltype(n)::value>),
                                   grid, dim3(256), 0, s, x, in.M, in.K, in.inv, deq, out, q8, in.rn, in.g, eps);
            };
            auto pick_q = [&](auto v, auto n) {
                if (q8) go(v, std::true_type{}, n);
                else go(v, std::false_type{}, n);
            };
            auto pick_v = [&](auto n) {
                if (vec) pick_q(std::true_type{}, n);
                else pick_q(std::false_type{}, n);
            };
            if (in.rn) pick_v(std::true_type{});
            else pick_v(std::false_type{});
            return hipGetLastError() == hipSuccess ? 0 : -1;
        }
    });
}

int launch_tcsc_rx(const float *XT, int Mp, const uint32_t *wstart, const uint32_t *ent, int Npad, int nch,
                   const YOut &o)
{
    hipStream_t s = (hipStream_t)o.stream;
    const int ytype = o.kernel_ytype(false);  // (the kernel tests the two scale pointers)
    const int mtiles = Mp / kRxTileM, ntiles = Npad / kRxTileCols;
    const dim3 grid((unsigned)(mtiles * ntiles)), block(kRxWaves * kLanes);
    auto *kernel = o.prelu ? tsg_tcsc_rx_kernel<true> : tsg_tcsc_rx_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, s, XT, Mp, wstart, ent, o.b, o.alpha, static_cast<float *>(o.Y), o.ldY, ytype,
                       o.M, o.N, nch, mtiles, ntiles, o.rs, o.cs, o.ep);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace tsg
