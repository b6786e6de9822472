// tsg_i8frag.h -- what the matrix-core kernels share on the device, over the
// one packed image (tsg_internal.h I8Geom):
//   every kernel (tsg_i8mfma, tsg_i8gemv, tsg_i8glu, tsg_x16mfma .hip)
//     mfma_row / mfma_row0   accumulator register -> row of a 32 x 32 tile
//   the four int8 kernels
//     v4i, v16i, i8_unpack   operands of v_mfma_i32_32x32x32_i8; an image dword -> a B fragment
//     i8_arow, i8_apiece     16 bytes of the int8 X: the one statement of the read rule
//   the two tile kernels (tsg_i8mfma_kernel, tsg_i8glu_kernel)
//     i8_atile_store, i8_afrag_offset, i8_afrags   the 128 x 64-byte A tile through LDS
//   the two split-K kernels (tsg_i8gemv_kernel, tsg_i8glu_gemv_kernel)
//     i8_splitk_tile, i8_wave_steps, i8_afrag_pair, i8_afrag_zero
// The B streams and the matrix-instruction loops stay with each kernel: they
// differ (one image or two, 8 or 16 bytes per lane and step).  The per-element
// finish they share is finish_store1 (tsg_epilogue.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tsg_internal.h"

namespace tsg {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// Accumulator register r of a 32 x 32 tile (v_mfma_*_32x32x*): lanes 0-31 hold
// the 32 columns of row 8 (r / 4) + r % 4 (mfma_row0: the first row of the
// register), lanes 32-63 those of the row 4 below -- one coalesced row segment
// per register and half wave, one element per lane.
__device__ __forceinline__ int mfma_row0(int r) { return 8 * (r >> 2) + (r & 3); }
__device__ __forceinline__ int mfma_row(int r, int lane) { return mfma_row0(r) + 4 * (lane >> 5); }

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

// The 16 bytes X[m][k .. k + 15] of an int8 X, M x K row-major, through the
// row's pointer xr = i8_arow(X, m, M, K) and row_in = m < M.  xvec (the
// launchers' x_vec_ok: K % 16 == 0 and X 16-byte aligned): a piece is inside a
// row or past its end, one 16-byte load; else byte by byte.  Rows >= M and
// k >= K are zero, and nothing outside [X, X + M K) is read: a row past M
// points at row 0 and is never read byte-wise.  (The row pointer is the
// caller's, computed once before its K loop: with m and M here the compiler no
// longer strength-reduces the addresses -- four more vector instructions per
// step of the tile kernels, ten more registers in the split-K kernels.)
__device__ __forceinline__ const int8_t *i8_arow(const int8_t *X, int m, int M, int K)
{
    return X + (size_t)(m < M ? m : 0) * K;
}
__device__ __forceinline__ uint4 i8_apiece(const int8_t *xr, bool row_in, int k, int K, int xvec)
{
    if (xvec) {
        const bool in = row_in && k < K;
        const uint4 v = *reinterpret_cast<const uint4 *>(xr + (in ? k : 0));
        return in ? v : make_uint4(0, 0, 0, 0);
    }
    uint32_t w[4] = {0, 0, 0, 0};
    if (row_in)
        for (int e = 0; e < 16 && k + e < K; e++) w[e >> 2] |= (uint32_t)(uint8_t)xr[k + e] << (8 * (e & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// ---------------------------------------------------------------------------
// The A tile of the tile kernels: a step's 128 rows x 64 bytes, loaded by the
// whole workgroup of kI8Threads -- thread t the 16-byte pieces t and t + 256,
// piece p = (row p / 4, k quarter p % 4), so four neighbouring lanes read one
// row's 64 contiguous bytes -- one step ahead, into registers, and stored to
// the other half of a double-buffered LDS tile after the step's matrix
// instructions (i8_atile_store): one barrier per step.  Piece j of a thread is
// the k quarter tid % 4 of tile row (tid + 256 j) / 4.
//
// LDS row pitch 80 B = 64 + 16.  A fragment read is a ds_read_b128 of lane l
// at (row0 + l % 32) * 80 + 32 kk + 16 (l / 32) (i8_afrag_offset, i8_afrags);
// the LDS serves a b128 read 16 lanes at a time (64 banks x 4 B = 16 slots of
// 16 B), and the 16 lanes of a group are 16 consecutive rows at one k offset,
// slot (5 row + c) mod 16: 5 is odd, so they fall on 16 distinct slots --
// conflict-free.  (The stores, rows r .. r + 3 x 4 quarters per group, collide
// two ways on 3 of 16 slots; there are 2 per thread and step against 4
// fragment reads.)
constexpr int kI8Pitch = kI8KStep + 16;

// the thread's two pieces, registers -> the LDS buffer xs
__device__ __forceinline__ void i8_atile_store(uint8_t *xs, const uint4 (&areg)[2])
{
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int p = (int)threadIdx.x + kI8Threads * j;
        *reinterpret_cast<uint4 *>(&xs[(p >> 2) * kI8Pitch + 16 * (p & 3)]) = areg[j];
    }
}

// where a lane's fragments of the 64 tile rows from row0 start in an LDS buffer ...
__device__ __forceinline__ int i8_afrag_offset(int row0, int lane)
{
    return (row0 + (lane & 31)) * kI8Pitch + 16 * (lane >> 5);
}
// ... and its four fragments from there: a[row tile][k half]
__device__ __forceinline__ void i8_afrags(const uint8_t *xb, v4i (&a)[2][2])
{
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int kk = 0; kk < 2; kk++) a[rt][kk] = *reinterpret_cast<const v4i *>(xb + 32 * rt * kI8Pitch + 32 * kk);
}

// ---------------------------------------------------------------------------
// Split-K (M <= 32: one row tile, the k-steps dealt to the S waves of a
// workgroup, wave w taking w, w + S, ...).
//
// The grid of 32-column workgroups: the two halves of a 64-column granule read
// alternate 8 bytes of the same lines, so they are numbered onto one XCD and
// its L2 (ids b and b + 8: workgroups go round the 8 XCDs by id,
// tsg_jit_map.h); the launchers pad the granules to a multiple of 8, and a
// workgroup of the padding (its first column >= N) returns at once.
struct I8SplitKTile {
    int ct, half;  // granule of 64 columns, and of it the column half
};
__device__ __forceinline__ I8SplitKTile i8_splitk_tile(int block)
{
    const int idx = block >> 3;
    return {(idx >> 1) * 8 + (block & 7), idx & 1};
}

// the steps of wave w of S
__device__ __forceinline__ int i8_wave_steps(int nks, int w, int S) { return nks > w ? (nks - w + S - 1) / S : 0; }

// A is not staged -- no wave reads a k range another wave of its workgroup
// reads: a lane's two fragments of step ks, k half kk at k = 64 ks + 32 kk + kl
// (xr, row_in: the row lane % 32; kl = 16 (lane / 32)), straight from global memory
__device__ __forceinline__ void i8_afrag_pair(const int8_t *xr, bool row_in, int kl, int ks, int K, int xvec,
                                              v4i (&a)[2])
{
#pragma unroll
    for (int kk = 0; kk < 2; kk++)
        a[kk] = __builtin_bit_cast(v4i, i8_apiece(xr, row_in, ks * kI8KStep + 32 * kk + kl, K, xvec));
}
// A slot past the wave's last step: its matrix instructions add 0 whatever its
// B holds, so the K loop has no branch around them
__device__ __forceinline__ void i8_afrag_zero(v4i (&a)[2])
{
#pragma unroll
    for (int kk = 0; kk < 2; kk++) a[kk] = v4i{0, 0, 0, 0};
}

}  // namespace tsg
