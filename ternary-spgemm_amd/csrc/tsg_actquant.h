// tsg_actquant.h -- device side of the fused per-row int8 activation
// quantisation (include/ternary_spgemm.h tcsc_hip_gemm_dev_actquant).  All fp32
// on the widened X, one rounding per operation, IEEE divisions:
//     a = max(max_k |x[m,k]|, 1e-5f);  inv[m] = 127.0f / a;  deq[m] = a / 127.0f
//     q[m,k] = min(max(rintf(x[m,k] * inv[m]), -127.0f), 127.0f)
// The row pass (tcsc_kernels.hip tsg_row_absmax_kernel) writes inv and deq; the
// staging passes quantise every value they load with xquant, so the staged
// copy holds integer-valued fp32 and the kernels that read it run the chain of
// an int8 X; deq is their per-row scale (tsg_scale.h).
#pragma once

#include <hip/hip_runtime.h>

namespace tsg {

constexpr float kActQuantEps = 1e-5f;  // floor of a row's maximum (a zero row: q = 0, deq = eps / 127)
constexpr float kActQuantMax = 127.0f;

// inv and deq of a row whose max |x| is amax.  hipcc divides fp32 correctly
// rounded (v_div_scale / v_div_fmas / v_div_fixup) unless told otherwise.
__device__ __forceinline__ void actquant_scales(float amax, float &inv, float &deq)
{
    const float a = fmaxf(amax, kActQuantEps);
    inv = kActQuantMax / a;
    deq = a / kActQuantMax;
}

// One value.  Like scale_bias: the pragma keeps the multiply a rounding of its
// own wherever this is inlined.  rintf rounds ties to even (v_rndne_f32); a
// NaN comes out as -127 (fmaxf returns the number), an infinity as +-127, so
// the result is always an integer in [-127, 127] (or -0).
__device__ __forceinline__ float xquant(float v, float inv)
{
#pragma clang fp contract(off)
    const float t = rintf(v * inv);
    return fminf(fmaxf(t, -kActQuantMax), kActQuantMax);
}

__device__ __forceinline__ float4 xquant4(float4 v, float inv)
{
    return make_float4(xquant(v.x, inv), xquant(v.y, inv), xquant(v.z, inv), xquant(v.w, inv));
}

}  // namespace tsg
