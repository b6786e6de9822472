// tsg_i8frag.h -- what the integer matrix-core kernels (tsg_i8mfma.hip,
// tsg_i8gemv.hip) share on the device: the operand types of
// v_mfma_i32_32x32x32_i8 and the unpacking of a packed image dword
// (tsg_internal.h I8Geom) to a B fragment.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace tsg {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// One packed dword -> the 16 int8 entries of a B fragment (tsg_internal.h).
// v_perm_b32 picks each result byte from its two sources by a selector byte:
// 0-7 a source byte, 8-11 the sign of one replicated, 12 the constant 0x00.
// Both sources are 0x80808001 -- byte 0 is 0x01 in either, every other sign is
// set -- so the code at bits 2-3 of a byte selects 0x01 (0), 0xff (8) or 0x00
// (12) whichever way the sources and the sign selectors are numbered.
__device__ __forceinline__ v4i i8_unpack(uint32_t w)
{
    constexpr uint32_t src = 0x80808001u, m = 0x0c0c0c0cu;
    v4i r;
    r.x = (int)__builtin_amdgcn_perm(src, src, (w << 2) & m);
    r.y = (int)__builtin_amdgcn_perm(src, src, w & m);
    r.z = (int)__builtin_amdgcn_perm(src, src, (w >> 2) & m);
    r.w = (int)__builtin_amdgcn_perm(src, src, (w >> 4) & m);
    return r;
}

}  // namespace tsg
