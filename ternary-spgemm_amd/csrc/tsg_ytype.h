// tsg_ytype.h -- device side of the Y element types (include/ternary_spgemm.h
// tsg_ytype; the host side, YType and ytype_size, is in tsg_internal.h).
// Every kernel that stores Y holds the finished fp32 value -- chain, + b[n],
// PReLU, all in fp32 as ever -- in a register right before the store.  For a
// 16-bit Y that value is rounded ONCE, to nearest even, here, and nothing is
// computed after it: the result is the element-wise cast of the fp32 call's Y.
// The fp32 stores stay in the kernels as they were; a kernel branches on the
// (wave-uniform) ytype once and comes here only for the 16-bit types.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tsg_internal.h"

namespace tsg {

typedef float yf32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 yf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 ybf16x2 __attribute__((ext_vector_type(2)));

// The two conversions, both round-to-nearest-even under the mode the kernels
// run in (hipcc's default: RNE, subnormals kept): beyond the largest finite
// value -> +-inf, fp16 subnormals kept, -0 stays -0, NaN stays a (quiet) NaN.
// fp16: v_cvt_f16_f32.  bf16: the fptrunc is gfx950's v_cvt_pk_bf16_f32 (two
// values per instruction in ypack2).
template <bool BF16>
__device__ __forceinline__ uint16_t ycvt1(float y)
{
    if constexpr (BF16)
        return __builtin_bit_cast(uint16_t, (__bf16)y);
    else
        return __builtin_bit_cast(uint16_t, (_Float16)y);
}
// two neighbours in one dword (lo at the lower address)
template <bool BF16>
__device__ __forceinline__ uint32_t ypack2(float lo, float hi)
{
    const yf32x2 v = {lo, hi};
    if constexpr (BF16)
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, ybf16x2));
    else
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, yf16x2));
}

// One element (the walks: a lane holds one column of a row)
__device__ __forceinline__ void ystore1(void *Y, int ytype, size_t i, float y)
{
    uint16_t *p = static_cast<uint16_t *>(Y) + i;
    *p = ytype == kYBF16 ? ycvt1<true>(y) : ycvt1<false>(y);
}

// NW consecutive values of a lane's row segment (the dispatchers and rx; NW a
// multiple of 8).  yrow: the segment's first element; nvalid: how many of its
// columns lie inside N (>= 1); val(c): the finished fp32 value of column c
// (called for every c < NW: past nvalid it must still be safe to evaluate).
// A full segment that starts 16-byte aligned goes out as 16-byte stores of 8
// elements; anything else -- the ragged last column tile, a misaligned row --
// element by element with 2-byte stores, so that nothing but the segment's own
// valid elements is written, not even the neighbour that shares a dword with
// its first or last one.  Eight values are converted and stored at a time:
// the accumulators stay where they are, nothing wider is held.
// The code holds val(c) once per column: a copy per type and per store width
// of a 128-column segment makes the compiler hoist what the copies share (a
// bias address and a guard per column) ahead of all of them, into more scalar
// registers than there are.  So the (uniform) type picks the conversion per
// group of 8 and the (per-lane) alignment picks the store per group of 8.
template <int NW, typename F>
__device__ __forceinline__ void ystore_seg(void *Y, int ytype, size_t first, int nvalid, F &&val)
{
    static_assert(NW % 8 == 0, "16-byte stores of 8 elements");
    uint16_t *yrow = static_cast<uint16_t *>(Y) + first;
    const bool vec = nvalid >= NW && (((uintptr_t)yrow & 15) == 0);
    const bool bf16 = ytype == kYBF16;
#pragma unroll
    for (int c = 0; c < NW; c += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = val(c + j);
        uint32_t w[4];
        if (bf16) {
#pragma unroll
            for (int j = 0; j < 4; j++) w[j] = ypack2<true>(v[2 * j], v[2 * j + 1]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) w[j] = ypack2<false>(v[2 * j], v[2 * j + 1]);
        }
        if (vec) {
            *reinterpret_cast<uint4 *>(yrow + c) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (c + j < nvalid) yrow[c + j] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
        }
    }
}

// The same for a segment of any Y type, fp32 included (the scaled epilogues,
// tsg_scale.h: one out-of-line copy of the epilogue serves all three types).
// fp32: a full segment whose first element is 16-byte aligned goes out as
// float4 stores, anything else as 4-byte stores of the valid elements -- the
// rule of the kernels' own fp32 stores.  Again val(c) is held once per column
// and the (uniform) type is looked at per group of 8.
// (tsg_epilogue.h ystore_seg_epi is this body again with the operand loads in
// the loop, and the kernels' epilogue branches repeat the scaled branch's
// lambda: a change to the store rule here is made there too.)
template <int NW, typename F>
__device__ __forceinline__ void ystore_seg_any(void *Y, int ytype, size_t first, int nvalid, F &&val)
{
    static_assert(NW % 8 == 0, "groups of 8 elements");
    const bool f32 = ytype == kYF32, bf16 = ytype == kYBF16;
    // one pointer for both element sizes (a lane holds nothing per type)
    char *yrow = static_cast<char *>(Y) + first * (f32 ? 4u : 2u);
    float *yrow32 = reinterpret_cast<float *>(yrow);
    uint16_t *yrow16 = reinterpret_cast<uint16_t *>(yrow);
    const bool vec = nvalid >= NW && (((uintptr_t)yrow & 15) == 0);
#pragma unroll
    for (int c = 0; c < NW; c += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = val(c + j);
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
