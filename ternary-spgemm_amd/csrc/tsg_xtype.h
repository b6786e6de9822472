// tsg_xtype.h -- device side of the X element types (include/ternary_spgemm.h
// tsg_xtype; the host side, XType and xtype_size, is in tsg_internal.h).
// Every kernel that reads the caller's X does it through xload1 / xload4:
// the value is widened to fp32 right after the load, exactly (fp16 -> fp32,
// bf16 -> fp32 and int8 -> fp32 lose nothing), so everything downstream -- the
// staged layouts, LDS, the chains -- holds the fp32 an fp32 call on the widened
// X would have held.  The float overloads are the plain loads.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tsg_internal.h"

namespace tsg {

// 16-bit elements are carried as their bits (no arithmetic on them here)
struct xf16 { uint16_t bits; };
struct xbf16 { uint16_t bits; };
typedef int8_t xi8;

// fp16: the hardware convert (v_cvt_f32_f16; subnormals are exact fp32 normals)
__device__ __forceinline__ float xwiden_f16(uint32_t bits16)
{
    return (float)__builtin_bit_cast(_Float16, (uint16_t)bits16);
}
// bf16 is the upper half of an fp32
__device__ __forceinline__ float xwiden_bf16(uint32_t bits16) { return __uint_as_float(bits16 << 16); }

// one element
__device__ __forceinline__ float xload1(const float *p) { return *p; }
__device__ __forceinline__ float xload1(const xf16 *p) { return xwiden_f16(p->bits); }
__device__ __forceinline__ float xload1(const xbf16 *p) { return xwiden_bf16(p->bits); }
__device__ __forceinline__ float xload1(const xi8 *p) { return (float)(int)*p; }

// four consecutive elements in ONE load: p is aligned to 4 elements (16 B for
// fp32, 8 B for the 16-bit types, 4 B for int8; x_vec_ok)
__device__ __forceinline__ float4 xload4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 xload4(const xf16 *p)
{
    const uint2 w = *reinterpret_cast<const uint2 *>(p);
    return make_float4(xwiden_f16(w.x & 0xffffu), xwiden_f16(w.x >> 16), xwiden_f16(w.y & 0xffffu),
                       xwiden_f16(w.y >> 16));
}
__device__ __forceinline__ float4 xload4(const xbf16 *p)
{
    const uint2 w = *reinterpret_cast<const uint2 *>(p);
    return make_float4(__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16),
                       __uint_as_float(w.y & 0xffff0000u));
}
__device__ __forceinline__ float4 xload4(const xi8 *p)
{
    const int w = *reinterpret_cast<const int *>(p);
    return make_float4((float)((w << 24) >> 24), (float)((w << 16) >> 24), (float)((w << 8) >> 24),
                       (float)(w >> 24));
}

// Calls f with X as a pointer to its element type; -1 for an unknown type
// (the C-ABI refuses those before any launcher runs).
template <typename F>
int with_xtype(const void *X, int xtype, F &&f)
{
    switch (xtype) {
    case kXF32: return f(static_cast<const float *>(X));
    case kXF16: return f(static_cast<const xf16 *>(X));
    case kXBF16: return f(static_cast<const xbf16 *>(X));
    case kXI8: return f(static_cast<const xi8 *>(X));
    default: return -1;
    }
}

}  // namespace tsg
