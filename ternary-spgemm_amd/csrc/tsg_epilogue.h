// tsg_epilogue.h -- device side of the fused epilogue (include/ternary_spgemm.h
// tcsc_hip_gemm_dev_ex): after + b[n] and the PReLU, still in fp32 and before
// the one rounding to the Y type,
//   a = ReLU(y) or ReLU(y)^2      (act; the PReLU stays the kernels' own)
//   a = a * widen(mul[m, n])      (the gate of a gated FFN)
//   a = a + widen(add[m, n])      (the residual)
// each rounded once, a missing step not performed.  Every kernel that stores Y
// branches once, on the kYEpi flag its launcher sets in the ytype argument
// (tsg_internal.h; wave-uniform), and comes here only then; a call without an
// epilogue runs the code it ran before.  The operands are [M, N] of fp32, fp16
// or bf16 (YType values) with a row stride of their own.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tsg_internal.h"
#include "tsg_ytype.h"

namespace tsg {

// The three steps on one finished fp32 value y.  g, r: the widened operand
// elements (ignored without has_mul / has_add).  As in scale_bias (tsg_scale.h)
// the pragma takes the `contract` flag off these operations wherever they are
// inlined: a * g + r is never one fma.
//   RELU   y > 0 ? y : (y != y ? y : +0)   -0 -> +0, a NaN stays a NaN
//   RELU2  the same, squared (rounded once; may overflow to +inf)
__device__ __forceinline__ float epi_apply(float y, int act, bool has_mul, float g, bool has_add, float r)
{
#pragma clang fp contract(off)
    float a = y;
    if (act >= kEpiRelu) {
        a = y > 0 ? y : (y != y ? y : 0.0f);
        if (act == kEpiRelu2) a = a * a;
    }
    if (has_mul) a = a * g;
    if (has_add) a = a + r;
    return a;
}

// widening a 16-bit element to fp32 (exact)
__device__ __forceinline__ float epi_widen16(uint16_t u, bool bf16)
{
    return bf16 ? __builtin_bit_cast(float, (uint32_t)u << 16) : (float)__builtin_bit_cast(_Float16, u);
}

// The operand pointer a kernel loads through: the caller's, or -- for an
// operand that IS Y (the launcher's alias bit) -- the kernel's own Y pointer,
// so that the load and the store of an element go through one pointer
__device__ __forceinline__ const char *epi_base(const void *op, bool is_y, const void *Y)
{
    return static_cast<const char *>(is_y ? Y : op);
}

// One element (the walks: a lane holds one column of a row)
__device__ __forceinline__ float epi_load1(const char *base, int t, size_t i)
{
    if (t == kYF32) return reinterpret_cast<const float *>(base)[i];
    return epi_widen16(reinterpret_cast<const uint16_t *>(base)[i], t == kYBF16);
}

// Eight consecutive values, columns c .. c + 7 of a lane's row segment that
// starts at seg (nvalid of its columns lie inside N, >= 1).  The load rule is
// the store rule of ystore_seg_any: a full-width segment that starts 16-byte
// aligned (vec, per operand and per lane) is loaded with 16-byte loads,
// anything else element by element; a column past nvalid reads the segment's
// last valid element (its value is never stored).  The same bits either way.
__device__ __forceinline__ void epi_load8(const char *seg, int t, bool vec, int c, int nvalid, float (&o)[8])
{
    if (t == kYF32) {
        const float *p = reinterpret_cast<const float *>(seg);
        if (vec) {
            const float4 lo = *reinterpret_cast<const float4 *>(p + c), hi = *reinterpret_cast<const float4 *>(p + c + 4);
            o[0] = lo.x, o[1] = lo.y, o[2] = lo.z, o[3] = lo.w;
            o[4] = hi.x, o[5] = hi.y, o[6] = hi.z, o[7] = hi.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) o[j] = p[c + j < nvalid ? c + j : nvalid - 1];
        }
        return;
    }
    const uint16_t *p = reinterpret_cast<const uint16_t *>(seg);
    const bool bf16 = t == kYBF16;
    if (vec) {
        const uint4 q = *reinterpret_cast<const uint4 *>(p + c);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] = epi_widen16((uint16_t)(w[j >> 1] >> (16 * (j & 1))), bf16);
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] = epi_widen16(p[c + j < nvalid ? c + j : nvalid - 1], bf16);
    }
}

// The walks' store: one element of any Y type
__device__ __forceinline__ void ystore1_any(void *Y, int yt, size_t i, float v)
{
    if (yt != kYF32)
        ystore1(Y, yt, i, v);
    else
        static_cast<float *>(Y)[i] = v;
}

// One element through the epilogue (the ELL walks): y is the finished fp32
// value (+ b[n], PReLU); m, n its row and column.  The element of an operand
// that is Y itself is read here, by the lane that stores it, before the store.
__device__ __forceinline__ void epi_store1(void *Y, int yt, int64_t ldY, const Epi &ep, int m, int n, float y)
{
    const bool has_mul = ep.mul != nullptr, has_add = ep.add != nullptr;
    float g = 0.0f, r = 0.0f;
    if (has_mul)
        g = epi_load1(epi_base(ep.mul, ep.bits & kEpiMulIsY, Y), (ep.bits >> kEpiMulShift) & 3,
                      (size_t)m * (size_t)ep.ldmul + n);
    if (has_add)
        r = epi_load1(epi_base(ep.add, ep.bits & kEpiAddIsY, Y), (ep.bits >> kEpiAddShift) & 3,
                      (size_t)m * (size_t)ep.ldadd + n);
    ystore1_any(Y, yt, (size_t)m * (size_t)ldY + n, epi_apply(y, ep.bits & kEpiActMask, has_mul, g, has_add, r));
}

// NW consecutive values of a lane's row segment through the epilogue (the
// dispatchers and rx): ystore_seg_any with the operand loads in its loop.  m:
// the row; nc0: the segment's first column; nvalid = N - nc0; val(c): the
// finished fp32 value of column c before the epilogue (+ b[n], PReLU), safe to
// evaluate for every c < NW.  Per group of 8 columns the lane loads its 8 gate
// and 8 residual elements, applies the three steps, converts and stores: the
// accumulators stay where they are and nothing wider than a group is held.
// An operand that is Y itself: group c's elements are loaded before group c is
// stored, by the lane that stores them, and no other lane touches them.
template <int NW, typename F>
__device__ __forceinline__ void ystore_seg_epi(void *Y, int yt, int64_t ldY, const Epi &ep, int m, int nc0, int nvalid,
                                               F &&val)
{
    static_assert(NW % 8 == 0, "groups of 8 elements");
    const int act = ep.bits & kEpiActMask, mt = (ep.bits >> kEpiMulShift) & 3, at = (ep.bits >> kEpiAddShift) & 3;
    const bool has_mul = ep.mul != nullptr, has_add = ep.add != nullptr;
    const bool f32 = yt == kYF32, bf16 = yt == kYBF16;
    char *yrow = static_cast<char *>(Y) + ((size_t)m * (size_t)ldY + nc0) * (f32 ? 4u : 2u);
    float *yrow32 = reinterpret_cast<float *>(yrow);
    uint16_t *yrow16 = reinterpret_cast<uint16_t *>(yrow);
    const bool vec = nvalid >= NW && (((uintptr_t)yrow & 15) == 0);
    // the operands' segments (a missing operand: Y's own, never loaded)
    const char *mseg = has_mul ? epi_base(ep.mul, ep.bits & kEpiMulIsY, Y) +
                                     ((size_t)m * (size_t)ep.ldmul + nc0) * (mt == kYF32 ? 4u : 2u)
                               : yrow;
    const char *aseg = has_add ? epi_base(ep.add, ep.bits & kEpiAddIsY, Y) +
                                     ((size_t)m * (size_t)ep.ldadd + nc0) * (at == kYF32 ? 4u : 2u)
                               : yrow;
    const bool mvec = nvalid >= NW && (((uintptr_t)mseg & 15) == 0);
    const bool avec = nvalid >= NW && (((uintptr_t)aseg & 15) == 0);
#pragma unroll
    for (int c = 0; c < NW; c += 8) {
        float g[8] = {}, r[8] = {};
        if (has_mul) epi_load8(mseg, mt, mvec, c, nvalid, g);
        if (has_add) epi_load8(aseg, at, avec, c, nvalid, r);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = epi_apply(val(c + j), act, has_mul, g[j], has_add, r[j]);
        if (f32) {
            if (vec) {
                *reinterpret_cast<float4 *>(yrow32 + c) = make_float4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<float4 *>(yrow32 + c + 4) = make_float4(v[4], v[5], v[6], v[7]);
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++)
                    if (c + j < nvalid) yrow32[c + j] = v[j];
            }
            continue;
        }
        uint32_t w[4];
        if (bf16) {
#pragma unroll
            for (int j = 0; j < 4; j++) w[j] = ypack2<true>(v[2 * j], v[2 * j + 1]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) w[j] = ypack2<false>(v[2 * j], v[2 * j + 1]);
        }
        if (vec) {
            *reinterpret_cast<uint4 *>(yrow16 + c) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (c + j < nvalid) yrow16[c + j] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
        }
    }
}

}  // namespace tsg
