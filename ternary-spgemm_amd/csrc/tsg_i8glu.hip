// tsg_i8glu.hip -- the fused gate/up projection of a gated FFN on the integer
// matrix cores (tcsc_hip_gemm_dev_glu): Y = act(gate(x)) * up(x), one launch
// over the packed images (tsg_internal.h I8Geom) of two handles of one shape.
// tsg_i8glu_kernel serves M > 32, tsg_i8glu_gemv_kernel 1 <= M <= 32.
//
// Why it stores the bits of the two-call sequence.  Both chains are the exact
// integers of tsg_i8mfma.hip's argument (|x| <= 128, W ternary, |sum| <= 128 K
// <= 2^24: int32 accumulators, v_cvt_f32_i32 exact, any order of the terms),
// so u = scale_bias(chain_up) is the fp32 value an up call stores into an fp32
// U, y = scale_bias(chain_gate) what the gate call hands its epilogue, and
// a = act(y) * u the product that epilogue forms with dmul = U: one fp32
// multiply, rounded once, never contracted (glu_store1).  What follows -- the
// caller's own dmul, dadd, the one rounding to the Y type -- is epi_store1 /
// ystore1_any, one element per lane, with the activation already applied.
//
// Tile variant.  Workgroup: 256 threads = 4 waves as 2 x 2 on 128 rows x 64
// columns, one granule of either image.  Wave (wm, wn) owns rows 64 wm .. + 63
// and the 32 columns of column half wn, for BOTH matrices: acc[row tile][matrix]
// is 64 accumulator registers, tsg_i8mfma_kernel's budget, so two workgroups
// still share a CU.  A: the double-buffered LDS tile both tile kernels take
// from tsg_i8frag.h (loaded through i8_apiece), one barrier per step.  B: per
// step a lane loads its contiguous 8 bytes of column half wn (dwords 2 wn and
// 2 wn + 1) from each image, one step ahead, registers only.  Per step a wave
// issues 4 ds_read_b128, 4 unpacks and 8 matrix instructions: an A fragment
// feeds both matrices, a B fragment both row tiles -- tsg_i8mfma_kernel's
// ratio.  Grid: one workgroup per (M tile, granule), the granule fastest:
// twice tsg_i8mfma_kernel's workgroups per call.
//
// Split-K variant.  One workgroup per 32 output columns, S waves (1, 2, 4, 8:
// tsg_internal.h i8glu_pick) taking the k-steps w, w + S, ...; a wave holds
// acc[matrix][k half] = 64 registers and loads per step 8 bytes of each image
// and its two A fragments straight from global memory (tsg_i8frag.h
// i8_afrag_pair), kGluDepth steps in flight in registers with a zero A past the
// wave's last step: no LDS and no barrier in the K loop.  The grid is the
// split-K numbering of tsg_i8frag.h (i8_splitk_tile: the two halves of a
// granule on one XCD).  Reduce: registers 0-15 are gate, 16-31 up, [S][32][64]
// ints of LDS (8 KiB S); after the one barrier wave w takes r = w, w + S, ...
// of 16 and sums the S partials of registers r AND 16 + r, so y and u of an
// element meet in one lane (tsg_i8frag.h mfma_row).  Registers whose rows are
// all >= M are neither written nor read.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tsg_epilogue.h"
#include "tsg_i8frag.h"
#include "tsg_internal.h"
#include "tsg_ytype.h"

namespace tsg {

namespace {

constexpr int kGluDepth = 2;  // steps in flight per wave of the split-K variant (tsg_i8gemv.hip: the measurement)

// What both variants hand their epilogue; by value, one kernel argument
struct GluOut {
    const float *b, *alpha, *cs, *b_up, *cs_up, *rs;
    Epi ep;     // the caller's dmul / dadd; its activation bits are cleared (act below)
    int act;    // kEpiRelu, kEpiRelu2 or 0 (the PReLU is the template flag)
    int ytype;  // YOut::kernel_ytype: the type, and kYEpi when ep has an operand
    int64_t ldY;
};

// A lane's column: what its elements take of the six per-column arrays, loaded once
struct GluCol {
    float b, cs, b_up, cs_up, alpha;
};
template <bool PRELU>
__device__ __forceinline__ GluCol glu_col(const GluOut &o, int n)
{
    GluCol c;
    c.b = o.b[n], c.b_up = o.b_up[n];
    c.cs = o.cs ? o.cs[n] : 0.0f, c.cs_up = o.cs_up ? o.cs_up[n] : 0.0f;
    c.alpha = PRELU ? o.alpha[n] : 0.0f;
    return c;
}

// One element: y and u from the two chains, a = act(y) * u, then the caller's
// operands and the store.  The pragma keeps a * u apart from the add that may
// follow it inside epi_store1.
template <bool PRELU>
__device__ __forceinline__ void glu_store1(float *Y, const GluOut &o, const GluCol &c, int cg, int cu, int m, int n)
{
#pragma clang fp contract(off)
    const bool has_rs = o.rs != nullptr;
    const float r = has_rs ? o.rs[m] : 0.0f;
    const float u = scale_bias((float)cu, has_rs, r, o.cs_up != nullptr, c.cs_up, c.b_up);
    const float y = scale_bias((float)cg, has_rs, r, o.cs != nullptr, c.cs, c.b);
    float a = y;
    if (PRELU) {
        a = (y > 0) ? y : c.alpha * y;  // comp_prelu.h:57-67
    } else if (o.act >= kEpiRelu) {
        a = y > 0 ? y : (y != y ? y : 0.0f);
        if (o.act == kEpiRelu2) a = a * a;
    }
    a = a * u;
    store1(Y, o.ytype & kYTypeMask, (o.ytype & kYEpi) != 0, o.ldY, o.ep, m, n, a);  // the caller's dmul / dadd
}

}  // namespace

template <bool PRELU>
__global__ __launch_bounds__(kI8Threads, 2) void tsg_i8glu_kernel(const int8_t *__restrict__ X,
                                                                   const uint32_t *__restrict__ img_g,
                                                                   const uint32_t *__restrict__ img_u, GluOut o,
                                                                   float *__restrict__ Y, int M, int N, int K, int nks,
                                                                   int granules, int xvec)
{
    __shared__ __attribute__((aligned(16))) uint8_t xs[2][kI8TileM * kI8Pitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int ct = blockIdx.x % granules, mt = blockIdx.x / granules;
    const int m0 = mt * kI8TileM;
    const int mw = m0 + 64 * wm, nw = kI8WaveN * ct + 32 * wn;  // the wave's tile
    const bool live = mw < M && nw < N;                          // (uniform) it holds an element of Y
    // the wave's two B streams: step ks at + 256 ks dwords
    const size_t boff = ((size_t)ct * nks * 64 + lane) * 4 + 2 * wn;
    const uint32_t *bg = img_g + boff, *bu = img_u + boff;

    v16i acc[2][2];  // [row tile][matrix: 0 gate, 1 up]
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int mx = 0; mx < 2; mx++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[rt][mx][r] = 0;

    // the thread's two pieces of a step's A tile, global -> registers: i8_apiece's
    // rule (tsg_i8frag.h) written out -- through the helper this kernel's M = 64
    // cells ran 1.0-1.3 % slower, past their spread (profiles/mfma_shared_ab.jsonl)
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
    uint2 qg = make_uint2(0, 0), qu = make_uint2(0, 0);
    if (nks > 0) {
        qg = *reinterpret_cast<const uint2 *>(bg);
        qu = *reinterpret_cast<const uint2 *>(bu);
        aload(0);
        i8_atile_store(xs[0], areg);
    }
    __syncthreads();
    const int arow = i8_afrag_offset(64 * wm, lane);
    for (int ks = 0; ks < nks; ks++) {
        const bool more = ks + 1 < nks;
        const size_t nxt = (size_t)(more ? ks + 1 : ks) * 256;  // the next step's B, in flight over this one
        const uint2 ng = *reinterpret_cast<const uint2 *>(bg + nxt), nu = *reinterpret_cast<const uint2 *>(bu + nxt);
        if (more) aload(ks + 1);
        if (live) {
            v4i a[2][2];
            i8_afrags(xs[ks & 1] + arow, a);
            const uint32_t bword[2][2] = {{qg.x, qg.y}, {qu.x, qu.y}};
#pragma unroll
            for (int mx = 0; mx < 2; mx++)
#pragma unroll
                for (int kk = 0; kk < 2; kk++) {
                    const v4i bf = i8_unpack(bword[mx][kk]);
#pragma unroll
                    for (int rt = 0; rt < 2; rt++)
                        acc[rt][mx] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[rt][kk], bf, acc[rt][mx], 0, 0, 0);
                }
        }
        if (more) i8_atile_store(xs[(ks + 1) & 1], areg);
        qg = ng, qu = nu;
        __syncthreads();  // the next tile is written; this one's reads are done
    }
    if (!live) return;

    const int n = nw + (lane & 31);
    if (n >= N) return;
    const GluCol c = glu_col<PRELU>(o, n);
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int m = mw + 32 * rt + mfma_row(r, lane);
            if (m < M) glu_store1<PRELU>(Y, o, c, acc[rt][0][r], acc[rt][1][r], m, n);
        }
}

template <bool PRELU>
__global__ __launch_bounds__(64 * kI8GluWaves) void tsg_i8glu_gemv_kernel(const int8_t *__restrict__ X,
                                                                          const uint32_t *__restrict__ img_g,
                                                                          const uint32_t *__restrict__ img_u, GluOut o,
                                                                          float *__restrict__ Y, int M, int N, int K,
                                                                          int nks, int xvec)
{
    extern __shared__ int red[];  // [S][32][64]
    constexpr int NR = 32, D = kGluDepth;
    const int lane = threadIdx.x & 63, S = (int)(blockDim.x >> 6);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // the workgroup's tile: column half `half` of granule ct
    const I8SplitKTile t = i8_splitk_tile((int)blockIdx.x);
    const int ct = t.ct, half = t.half, n0 = kI8WaveN * ct + 32 * half;
    if (n0 >= N) return;  // (uniform) a workgroup of the grid's padding to 16

    const size_t boff = ((size_t)ct * nks * 64 + lane) * 4 + 2 * half;  // step ks at + 256 ks
    const uint32_t *bg = img_g + boff, *bu = img_u + boff;
    const int row = lane & 31, kl = 16 * (lane >> 5);
    const int8_t *xr = i8_arow(X, row, M, K);
    const int cnt = i8_wave_steps(nks, w, S);

    uint32_t bq[D][2][2];  // [slot][matrix][k half]
    v4i a[D][2];
    // the wave's j-th step into slot d (past its last step: a zero A)
    auto load = [&](int d, int j) {
        if (j < cnt) {
            const int ks = w + j * S;
            const uint2 vg = *reinterpret_cast<const uint2 *>(bg + (size_t)ks * 256);
            const uint2 vu = *reinterpret_cast<const uint2 *>(bu + (size_t)ks * 256);
            bq[d][0][0] = vg.x, bq[d][0][1] = vg.y, bq[d][1][0] = vu.x, bq[d][1][1] = vu.y;
            i8_afrag_pair(xr, row < M, kl, ks, K, xvec, a[d]);
        } else {
            i8_afrag_zero(a[d]);
        }
    };

    v16i acc[2][2];  // [matrix][k half]
#pragma unroll
    for (int mx = 0; mx < 2; mx++)
#pragma unroll
        for (int kk = 0; kk < 2; kk++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[mx][kk][r] = 0;
#pragma unroll
    for (int d = 0; d < D; d++) {
#pragma unroll
        for (int f = 0; f < 4; f++) bq[d][f >> 1][f & 1] = 0;
        load(d, d);
    }
    for (int i = 0; i < cnt; i += D) {
#pragma unroll
        for (int d = 0; d < D; d++) {
#pragma unroll
            for (int mx = 0; mx < 2; mx++)
#pragma unroll
                for (int kk = 0; kk < 2; kk++)
                    acc[mx][kk] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[d][kk], i8_unpack(bq[d][mx][kk]), acc[mx][kk],
                                                                        0, 0, 0);
            load(d, i + d + D);
        }
    }

    // register j = 16 matrix + r of the wave -> red[(w NR + j) 64 + lane]
#pragma unroll
    for (int mx = 0; mx < 2; mx++)
#pragma unroll
        for (int r = 0; r < 16; r++)
            if (mfma_row0(r) < M) red[(w * NR + 16 * mx + r) * 64 + lane] = acc[mx][0][r] + acc[mx][1][r];
    __syncthreads();

    const int n = n0 + (lane & 31);
    const GluCol c = glu_col<PRELU>(o, n < N ? n : n0);
    for (int r = w; r < 16; r += S) {
        if (mfma_row0(r) >= M) continue;  // (uniform) a register of padding rows
        int sg = 0, su = 0;
        for (int s = 0; s < S; s++) {
            sg += red[(s * NR + r) * 64 + lane];
            su += red[(s * NR + 16 + r) * 64 + lane];
        }
        const int m = mfma_row(r, lane);
        if (m < M && n < N) glu_store1<PRELU>(Y, o, c, sg, su, m, n);
    }
}

// o: the gate call's output block with the up side filled in (img_up, b_up,
// cs_up); X: int8 [M][K]; img: the gate handle's image.  M <= kI8GemvMaxM and
// !tile: the split-K variant.
int launch_tcsc_i8glu(const int8_t *X, const uint32_t *img, int K, const YOut &o, bool tile)
{
    if (o.M < 1 || !o.img_up || !o.b_up) return -2;  // (run_mfma sends no other call here)
    GluOut g;
    g.b = o.b, g.alpha = o.alpha, g.cs = o.cs, g.b_up = o.b_up, g.cs_up = o.cs_up, g.rs = o.rs;
    g.ep = o.ep;
    g.act = o.ep.bits & kEpiActMask;
    g.ep.bits &= ~kEpiActMask;  // applied before the multiply by u, not by epi_store1
    g.ytype = o.ytype | (g.ep.on() ? kYEpi : 0);
    g.ldY = o.ldY;
    const int nks = i8_nks(K), xvec = x_vec_ok(X, K, 16);
    const int64_t granules = ((int64_t)o.N + kI8WaveN - 1) / kI8WaveN;
    float *Y = static_cast<float *>(o.Y);
    if (!tile && o.M <= kI8GemvMaxM) {
        const int S = i8glu_pick(K);
        const dim3 grid((unsigned)((granules + 7) / 8 * 16)), block(64 * S);
        const size_t lds = (size_t)S * 32 * 64 * sizeof(int);
        auto *kernel = o.prelu ? tsg_i8glu_gemv_kernel<true> : tsg_i8glu_gemv_kernel<false>;
        hipLaunchKernelGGL(kernel, grid, block, lds, (hipStream_t)o.stream, X, img, o.img_up, g, Y, o.M, o.N, K, nks,
                           xvec);
    } else {
        const int64_t mtiles = ((int64_t)o.M + kI8TileM - 1) / kI8TileM;
        // (run_mfma refuses it first; two workgroups per 128 x 128 tile: the grid stays under 2^32 threads)
        if (!mfma_grid_ok(o.M, o.N, kI8TileM, kI8TileN, kI8Threads)) return -2;
        const dim3 grid((unsigned)(granules * mtiles)), block(kI8Threads);
        auto *kernel = o.prelu ? tsg_i8glu_kernel<true> : tsg_i8glu_kernel<false>;
        hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)o.stream, X, img, o.img_up, g, Y, o.M, o.N, K, nks,
                           (int)granules, xvec);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace tsg
