// tsg_norm.h -- device side of the fused RMSNorm in front of the activation
// quantisation (include/ternary_spgemm.h tcsc_hip_gemm_dev_normquant).  All
// fp32 on the widened X, one rounding per operation, no fma, IEEE division and
// square root:
//     sq[k] = x[m,k] * x[m,k]
//     s[p]  = ((+0 + sq[p]) + sq[p + 256]) + ...      p = 0..255, ascending k
//     ss    = the 256 partials by a balanced binary tree, neighbours first
//     rn[m] = 1.0f / sqrtf(ss / (float)K + eps)
//     xn[m,k] = (x[m,k] * rn[m]) * gamma[k]           (gamma NULL: one multiply)
// and then tsg_actquant.h on xn.  The row pass (tcsc_kernels.hip
// tsg_row_absmax_kernel, NORM) writes rn next to inv and deq; the staging
// passes and the row pass's own sweeps make xn through xnorm, so the two
// cannot drift apart.  A multiply by 1.0f is the identity on every fp32 bit
// pattern, so an absent gamma is carried as 1.0f.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tsg_actquant.h"

namespace tsg {

// What a staging pass does to each value it loads
enum XStage : int {
    kStageNone = 0,   // nothing: the pass as it was
    kStageQuant = 1,  // xquant(v, inv[m])                       (an actquant call)
    kStageNorm = 2,   // xquant(xnorm(v, rn[m], g[k]), inv[m])   (a normquant call)
};

// acc + v * v, two roundings
__device__ __forceinline__ float norm_sq_add(float acc, float v)
{
#pragma clang fp contract(off)
    const float sq = v * v;
    return acc + sq;
}

// rn of a row whose sum of squares is ss (K > 0).  hipcc divides and takes
// square roots of fp32 correctly rounded unless told otherwise.
__device__ __forceinline__ float norm_rn(float ss, int K, float eps)
{
#pragma clang fp contract(off)
    const float ms = ss / (float)K;
    return 1.0f / sqrtf(ms + eps);
}

// One normalised value: two roundings, in this order.
__device__ __forceinline__ float xnorm(float v, float rn, float g)
{
#pragma clang fp contract(off)
    const float t = v * rn;
    return t * g;
}

__device__ __forceinline__ float xnormquant(float v, float rn, float g, float inv)
{
    return xquant(xnorm(v, rn, g), inv);
}

// gamma[k], 1.0f where there is no gamma or no such k
__device__ __forceinline__ float gload1(const float *__restrict__ g, int k, int K)
{
    return (g && k < K) ? g[k] : 1.0f;
}

// gamma[k .. k + 3], k % 4 == 0: one 16-byte load where the quad is whole and
// gamma + k is aligned to it (gamma itself needs only 4-byte alignment)
__device__ __forceinline__ float4 gload4(const float *__restrict__ g, int k, int K)
{
    if (g && k + 3 < K && ((uintptr_t)(g + k) & 15) == 0) return *reinterpret_cast<const float4 *>(g + k);
    return make_float4(gload1(g, k, K), gload1(g, k + 1, K), gload1(g, k + 2, K), gload1(g, k + 3, K));
}

// What a staging pass stores for the value v = X[m, k] it loaded (m < M).  A
// slot past K holds +0 and stays +0.
template <int MODE>
__device__ __forceinline__ float xstage(float v, int m, int k, int K, const float *__restrict__ inv,
                                        const float *__restrict__ rn, const float *__restrict__ g)
{
    if (MODE == kStageNorm) return k < K ? xnormquant(v, rn[m], gload1(g, k, K), inv[m]) : v;
    if (MODE == kStageQuant) return xquant(v, inv[m]);
    return v;
}

// The same for the quad v = X[m, k .. k + 3], k % 4 == 0
template <int MODE>
__device__ __forceinline__ float4 xstage4(float4 v, int m, int k, int K, const float *__restrict__ inv,
                                          const float *__restrict__ rn, const float *__restrict__ g)
{
    if (MODE == kStageNorm) {
        const float r = rn[m], iv = inv[m];
        const float4 gv = gload4(g, k, K);
        return make_float4(k < K ? xnormquant(v.x, r, gv.x, iv) : v.x, k + 1 < K ? xnormquant(v.y, r, gv.y, iv) : v.y,
                           k + 2 < K ? xnormquant(v.z, r, gv.z, iv) : v.z,
                           k + 3 < K ? xnormquant(v.w, r, gv.w, iv) : v.w);
    }
    if (MODE == kStageQuant) return xquant4(v, inv[m]);
    return v;
}

}  // namespace tsg
