/*
 * ternary_spgemm.h -- C-ABI of the MI355X-native ternary TCSC spGEMM.
 *
 *     Y[m,n] = ( sum_{k in P(n)} X[m,k]  -  sum_{k in N(n)} X[m,k] ) + b[n]
 *
 * with W in {-1,0,+1}^{K x N} given in the reference's TCSC layout
 * (col_start_pos/neg: N+1 ints; row_index_pos/neg: ascending k per column).
 * Results are bit-identical to the reference CPU kernel BaseTCSC<float>
 * (cpp_impl/comp.h:25-69): every output is ONE serial fp32 chain
 * 0 + x_p1 + ... + x_pP - x_n1 - ... - x_nQ, then + b[n].
 *
 * This header is the drop-in surface (registration, the comp_func calls,
 * introspection, host helpers).  Tuning and test hooks of the same library
 * (stream widths, kernel and image choices, the generated code for CPU
 * emulation) are declared in ternary_spgemm_test.h.
 *
 * Plain pointers and sizes only; no torch or HIP types.  Every function
 * returns TSG_OK (0) or a TSG_ERR_* code; tcsc_hip_last_error() gives text.
 * Reference interfaces each entry point replaces are cited as
 * path:line relative to alessiomelone/Ternary-spGEMM.
 */
#ifndef TERNARY_SPGEMM_H
#define TERNARY_SPGEMM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSG_ABI_VERSION 2

enum tsg_status {
    TSG_OK = 0,
    TSG_ERR_ARG = 1,     /* bad argument: null pointer, shape mismatch, malformed TCSC */
    TSG_ERR_HIP = 2,     /* HIP runtime / launch failure */
    TSG_ERR_NOMEM = 3,   /* device or host allocation failed */
    TSG_ERR_NODEV = 4,   /* no usable gfx950 device */
    TSG_ERR_RANGE = 5    /* size exceeds a supported limit */
};

/* Opaque handle: one TCSC weight matrix resident on one device (the device
 * image built from the TCSC arrays at registration, plus a work buffer). */
typedef struct tsg_tcsc tsg_tcsc;

/* ---- registration ---------------------------------------------------------
 * Replaces `std::make_shared<TCSC>(W_raw, K, N)` + capture in the
 * add_function lambda (cpp_impl/main.cpp:63,76-81; TCSC.h:13-41): the format
 * is built/uploaded ONCE, before any call.  Arrays are copied; the caller
 * keeps ownership.  device < 0 selects the current HIP device.
 * On failure *out is NULL and the status says why. */
int tcsc_hip_create(const int32_t *col_start_pos, const int32_t *col_start_neg,
                    const int32_t *row_index_pos, const int32_t *row_index_neg,
                    int K, int N, int device, tsg_tcsc **out);

/* Same, from a dense row-major K x N ternary matrix (TCSC ctor semantics,
 * TCSC.h:13-41; any value other than +1/-1 is treated as 0, as there). */
int tcsc_hip_create_dense(const int32_t *W, int K, int N, int device, tsg_tcsc **out);

/* GPU-side TCSC encoder (the TCSC ctor, TCSC.h:13-41, on the device): dW is a
 * dense row-major K x N int32 ternary matrix in device memory; d_csp / d_csn
 * (int32[N+1], caller-allocated device arrays) receive the column starts and
 * *nnz_pos / *nnz_neg the entry counts (the call synchronises `stream` to
 * return them).  When d_rip and d_rin are non-NULL (device arrays of at least
 * rip_cap >= nnz_pos and rin_cap >= nnz_neg int32s) the row indices are filled
 * too; call first with NULLs to size them.  Same arrays as tcsc_hip_create_dense
 * builds on the host, bit for bit. */
int tcsc_hip_encode_dense_dev(const int32_t *dW, int K, int N, int32_t *d_csp, int32_t *d_csn,
                              int32_t *d_rip, int64_t rip_cap, int32_t *d_rin, int64_t rin_cap,
                              int64_t *nnz_pos, int64_t *nnz_neg, void *stream);

/* Same, from "CSC with compressed values vector (1s and -1s, 8 bits for 5
 * values)" (readme.md:111, the reference's optimisation idea 2): col_ptr
 * int32[N+1], row_idx int32[nnz] (ascending k per column), values base-3
 * packed 5 per byte in CSC order, digit = v + 1.  Results are the same
 * BaseTCSC chains (+1 entries, then -1 entries, each ascending). */
int tcsc_hip_create_csc_packed(const int32_t *col_ptr, const int32_t *row_idx,
                               const uint8_t *packed, int K, int N, int device, tsg_tcsc **out);

/* BlockedTCSC<B> registration (data_structures/BlockedTCSC.h:5-49; the
 * reference's main.cpp:69 builds it with B = BLOCK_SIZE = 512): col_start_pos /
 * col_start_neg have (K/B)*N + 1 entries, slot kb*N + n listing column n's
 * +1 / -1 rows of block kb ([kb*B, kb*B + B), ascending); rows past (K/B)*B
 * are not part of the format.  Calls through the handle then compute
 * BaseBlockedTCSC<float> (comp.h:607-658): per block y = 0 + pos - neg, Y += y
 * block by block, then + b -- bit for bit, in that order.  Runs on the
 * weight-compiled kernel only (TSG_KERNEL must be unset or "jit"). */
int tcsc_hip_create_blocked(const int32_t *col_start_pos, const int32_t *col_start_neg,
                            const int32_t *row_index_pos, const int32_t *row_index_neg,
                            int K, int N, int B, int device, tsg_tcsc **out);

/* Releases every device/host resource of the handle (NULL is a no-op). */
void tcsc_hip_destroy(tsg_tcsc *h);

/* ---- compute --------------------------------------------------------------
 * Replaces one call of the registered comp_func
 *   using comp_func = std::function<void(float*X, float*B, float*Y, int M, int N, int K)>
 * (cpp_impl/common.h:12) bound to BaseTCSC<float> (comp.h:25-69).
 * Argument order M, N, K as there.  HOST pointers: X is M x K row-major,
 * b has N floats, Y is M x N row-major and is fully overwritten.
 * Synchronous: Y is valid on return (main.cpp:214-216, perf.cpp:62-66).
 * Host threads sharing a handle run their host-pointer calls one at a time
 * (the handle's staging buffers and streams).
 * A large call is pipelined by M chunks (tcsc_hip_host_chunk_rows): X chunk
 * i+1 travels in while chunk i computes and chunk i-1's Y travels out, on
 * three streams of the handle plus one helper thread for the Y copies; the
 * result is the unchunked one bit for bit (rows are independent). */
int tcsc_hip_gemm(tsg_tcsc *h, const float *X, const float *b, float *Y, int M, int N, int K);

/* Optional page-locking of a host buffer the caller passes to repeated
 * host-pointer calls (e.g. the X and Y of a benchmark loop, perf.cpp:37-71):
 * the call's copies then DMA directly instead of through the runtime's
 * pin-on-the-fly staging.  The buffer must stay allocated until
 * tcsc_hip_host_unregister.  Unregistered (pageable) buffers keep working.
 * Extension: no reference counterpart. */
int tcsc_hip_host_register(void *p, size_t bytes);
int tcsc_hip_host_unregister(void *p);

/* DEVICE pointers (on the handle's device), enqueued on `stream`
 * (a hipStream_t; NULL = legacy default stream); returns without waiting.
 * Streams: calls on one handle are serialised on the host (a mutex) and share
 * the handle's X^T work buffer; a call on a different stream than the
 * previous call waits (hipStreamWaitEvent) for the previous call's kernel
 * before it overwrites that buffer, so calls from several streams / threads
 * on one handle are safe (and run one after the other on the device).
 * The first call whose M picks a code image or work-buffer size the handle
 * has not prepared yet compiles / allocates it and synchronises `stream`
 * (the image's probe launch); tcsc_hip_reserve(h, max_M) is the place to do
 * that ahead of time.
 * Graph capture: after tcsc_hip_reserve(h, max_M), calls with M <= max_M
 * allocate, compile and synchronise nothing and can be captured; a captured
 * call reuses the work buffer when replayed, so a replay must not overlap
 * other calls on the same handle issued on other streams (a capture does not
 * change what uncaptured calls on other streams wait for). */
int tcsc_hip_gemm_dev(tsg_tcsc *h, const float *dX, const float *db, float *dY,
                      int M, int N, int K, void *stream);

/* PReLU twin: comp_func_prelu (common.h:13) bound to BaseTCSC_PreLU<float>
 * (comp_prelu.h:12-70): y = chain + b[n]; Y = y > 0 ? y : alpha[n]*y. */
int tcsc_hip_gemm_prelu(tsg_tcsc *h, const float *X, const float *b, const float *alpha,
                        float *Y, int M, int N, int K);
int tcsc_hip_gemm_prelu_dev(tsg_tcsc *h, const float *dX, const float *db, const float *dalpha,
                            float *dY, int M, int N, int K, void *stream);

/* The same two calls with an output row stride: row m of the result starts at
 * dY + m * ldY (ldY in floats, 64-bit), so an [M, N] block lands in its own
 * columns of a wider row-major buffer -- several handles fed by one X writing
 * side by side, or one column shard of a larger Y -- without a second pass.
 * ldY >= N is required: a smaller value returns TSG_ERR_ARG with a message and
 * enqueues nothing.  Floats outside [m * ldY, m * ldY + N) are never written.
 * Rows whose start is not 16-byte aligned (an odd ldY, a misaligned dY) are
 * stored float by float, the others with 16-byte stores; the result is the
 * same bit for bit.  Everything else -- stream semantics, reserve and graph
 * capture, the kernel an M picks -- is as tcsc_hip_gemm_dev, which is the
 * ldY = N case of this call.  Extension: no reference counterpart.
 *
 * Inputs of every device-pointer call: dX, db and dalpha need only 4-byte
 * alignment, so they may be slices of larger buffers.  A 16-byte aligned dX
 * with K % 4 == 0 selects the vector staging passes and the direct-X path of
 * the 64-row image (one launch); any other dX takes the scalar passes and the
 * staged copy -- the result is the same bit for bit.  No result depends on
 * memory outside [dX, dX + M*K), [db, db + N) and [dalpha, dalpha + N), nor on
 * a previous call on the handle (its X^T work buffer, its device copies of
 * host operands, LDS); the inputs are never written.  Pinned by
 * tests/test_gpu_isolation.py (operands inside NaN-filled buffers, an all-NaN
 * call before the checked one): no value from outside those ranges reaches Y.
 * That no address outside them is ever loaded is not claimed. */
int tcsc_hip_gemm_dev_ld(tsg_tcsc *h, const float *dX, const float *db, float *dY, int64_t ldY,
                         int M, int N, int K, void *stream);
int tcsc_hip_gemm_prelu_dev_ld(tsg_tcsc *h, const float *dX, const float *db, const float *dalpha,
                               float *dY, int64_t ldY, int M, int N, int K, void *stream);

/* The same two calls with X in a narrower element type: activations held in
 * 16 or 8 bits go in as they are, without an fp32 copy of X.  dX is M x K
 * row-major of the type xtype names, aligned to its element size only (it may
 * be a slice of a larger buffer); b, alpha and Y stay fp32, and ldY, the
 * stream semantics, tcsc_hip_reserve and graph capture are as on
 * tcsc_hip_gemm_dev_ld.  The library widens X to fp32 inside the pass that
 * reads it (its X^T staging pass, or the small-M walks' load of X), and
 *
 *   Y equals, bit for bit, what tcsc_hip_gemm_dev_ld gives on the element-wise
 *   widened X.
 *
 * fp16 -> fp32, bf16 -> fp32 and int8 -> fp32 are exact: fp16 subnormals widen
 * to their exact fp32 values, +-inf and -0 are kept, a NaN stays a NaN (its
 * payload is not promised, as elsewhere in this library).  With int8 X every
 * partial sum of a chain is an integer of magnitude at most 128 K, so the chains
 * are integer-exact while K * 128 <= 2^24 (K * 127 < 2^24 without -128).
 * TSG_X_F32 is tcsc_hip_gemm_dev_ld itself (the same path, direct X included).
 * Any other xtype value returns TSG_ERR_ARG with a message and enqueues
 * nothing.  A dX aligned to 4 elements with K % 4 == 0 selects the vector
 * staging passes (one 8-byte load per four 16-bit elements, one 4-byte load
 * per four int8), any other dX the scalar ones -- same result.  A 16- or
 * 8-bit X is always staged (the weight-compiled images read fp32), so such a
 * call uses the work buffer at every M that runs an image;
 * tcsc_hip_reserve(h, max_M) sizes it for that.  The isolation paragraph above
 * holds with [dX, dX + M*K) counted in elements of the type.  The kernel and
 * image an M picks do not depend on the type.  Extension: no reference
 * counterpart. */
enum tsg_xtype { TSG_X_F32 = 0, TSG_X_F16 = 1, TSG_X_BF16 = 2, TSG_X_I8 = 3 };

int tcsc_hip_gemm_dev_x(tsg_tcsc *h, const void *dX, int xtype, const float *db, float *dY,
                        int64_t ldY, int M, int N, int K, void *stream);
int tcsc_hip_gemm_prelu_dev_x(tsg_tcsc *h, const void *dX, int xtype, const float *db,
                              const float *dalpha, float *dY, int64_t ldY, int M, int N, int K,
                              void *stream);

/* The same two calls again with Y in a narrower element type as well: a layer
 * that keeps its activations in 16 bits gets them back in 16 bits from the one
 * call, without a cast pass over an fp32 Y.  dY is M rows of the type ytype
 * names; b and alpha stay fp32; xtype and ytype are independent.  The chain,
 * + b[n] and the PReLU run in fp32 exactly as on tcsc_hip_gemm_dev_x, and the
 * rounding is the last step before the store, so
 *
 *   Y[m, n] is the value tcsc_hip_gemm_dev_x / _prelu_dev_x would have stored,
 *   rounded ONCE, to nearest even, to the type: bit for bit the element-wise
 *   round-to-nearest-even cast of the fp32 call's Y.
 *
 * Values beyond the type's largest finite value round to +-inf (fp16: from
 * 65520), fp16 subnormal results are kept, not flushed, -0 stays -0, and a NaN
 * stays a NaN (its payload is not promised, as elsewhere in this library).
 * ldY counts ELEMENTS OF THE Y TYPE and must be >= N (else TSG_ERR_ARG, nothing
 * enqueued).  dY needs only element alignment (2 bytes for the 16-bit types),
 * so it may be any slice of a wider buffer.  Only the elements
 * [m * ldY, m * ldY + N) of each row are written -- and that holds for the
 * 16-bit neighbour that shares a dword with a row's first or last element too:
 * it is never written, not even with its own value.  A row segment that starts
 * 16-byte aligned and is full width (a lane's 8 to 128 columns inside N) is
 * stored with 16-byte stores of 8 elements; anything else -- the ragged last
 * column tile, rows of an odd ldY or a misaligned dY -- element by element
 * with 2-byte stores; the result is the same bit for bit.
 * TSG_Y_F32 is tcsc_hip_gemm_dev_x itself (the same path, ldY in floats).  Any
 * other ytype value returns TSG_ERR_ARG with a message naming tsg_ytype and
 * enqueues nothing.  Stream semantics, tcsc_hip_reserve and graph capture, the
 * kernel and image an M picks, the direct-X path of the 64-row image and the
 * work buffer are as on tcsc_hip_gemm_dev_x: the Y type adds no allocation and
 * no launch.  The host-pointer calls stay fp32.  Extension: no reference
 * counterpart. */
enum tsg_ytype { TSG_Y_F32 = 0, TSG_Y_F16 = 1, TSG_Y_BF16 = 2 };

int tcsc_hip_gemm_dev_xy(tsg_tcsc *h, const void *dX, int xtype, const float *db, void *dY,
                         int ytype, int64_t ldY, int M, int N, int K, void *stream);
int tcsc_hip_gemm_prelu_dev_xy(tsg_tcsc *h, const void *dX, int xtype, const float *db,
                               const float *dalpha, void *dY, int ytype, int64_t ldY, int M, int N,
                               int K, void *stream);

/* The same two calls once more with a per-row and a per-column scale in the
 * epilogue.  A ternary W comes with a weight scale (W ~ gamma * T, per tensor
 * or per output column) and int8 activations with a per-row (per-token)
 * dequantisation scale; the layer needs
 *
 *   Y[m, n] = chain(m, n) * drow_scale[m] * dcol_scale[n] + db[n]
 *
 * from the one call, without a zero b, an fp32 Y and a second pass over Y --
 * and with int8 X the unscaled chains (integers up to 127 * nnz(column)) would
 * overflow an fp16 Y from 65520 on.  drow_scale is float[M], dcol_scale is
 * float[N], both device memory that needs only 4-byte alignment (slices are
 * fine); either may be NULL.
 *
 * Order and rounding.  All arithmetic is fp32, one rounding per operation, no
 * fused multiply-add anywhere:
 *
 *   t = chain                  exactly the value tcsc_hip_gemm_dev_x adds b to
 *                              (a blocked handle: after its last block)
 *   if (drow_scale) t = t * drow_scale[m]        rounded
 *   if (dcol_scale) t = t * dcol_scale[n]        rounded
 *   y = t + db[n]                                rounded, never contracted with
 *                                                the multiply before it
 *   PReLU as on the other calls, then the one rounding to ytype as on _xy.
 *
 * Special values.  A scale may be any fp32 value -- 0, negative, subnormal,
 * inf, NaN: Y is the IEEE result of the operations above (a NaN's payload is
 * not promised, as elsewhere in this library).
 * NULL scales.  A NULL scale means its multiply is not performed (not a
 * multiply by 1).  With both NULL the call is tcsc_hip_gemm_dev_xy itself: the
 * same path, bit for bit.
 * As on _xy: the meaning of ldY (elements of the Y type, >= N), dY's alignment
 * and the guarantee that only [m * ldY, m * ldY + N) of each row is written,
 * the 16-bit neighbour in a shared dword included; stream semantics,
 * tcsc_hip_reserve and graph capture; the kernel and image an M picks and the
 * direct-X path of the 64-row image; the work buffer.  The scales add no
 * launch, no allocation and no synchronisation: they are two more pointers of
 * the kernel that stores Y.
 * Isolation.  The isolation paragraph above extends to the scales: no result
 * depends on memory outside [drow_scale, drow_scale + M) and [dcol_scale,
 * dcol_scale + N), and the scales are never written.
 * Errors.  A bad xtype, ytype or ldY and a null handle are TSG_ERR_ARG with a
 * message, nothing enqueued, as on _xy.
 * Out of scope: a NULL db (pass zeros); the host-pointer calls, which stay
 * fp32 and unscaled; the plugin header (tcsc_hip_plugin.hpp).  Extension: no
 * reference counterpart. */
int tcsc_hip_gemm_dev_scaled(tsg_tcsc *h, const void *dX, int xtype, const float *drow_scale,
                             const float *dcol_scale, const float *db, void *dY, int ytype, int64_t ldY,
                             int M, int N, int K, void *stream);
int tcsc_hip_gemm_prelu_dev_scaled(tsg_tcsc *h, const void *dX, int xtype, const float *drow_scale,
                                   const float *dcol_scale, const float *db, const float *dalpha, void *dY,
                                   int ytype, int64_t ldY, int M, int N, int K, void *stream);

/* The _scaled calls with the int8 activations and their per-row scale made
 * inside the call: per-row (per-token) symmetric int8 quantisation of an fp32,
 * fp16 or bf16 X, fused into the pass that stages X.  With the int8 X and the
 * row scale of the _scaled calls this is a W1.58A8 linear layer from
 * activations in their own type, one call, no int8 copy of X in memory.
 *
 * Contract.  All arithmetic is fp32 on the widened X (the widening is exact),
 * one rounding per operation, both divisions IEEE correctly rounded:
 *
 *   amax[m] = max_k |x[m, k]|                     (0 for K = 0)
 *   a       = max(amax[m], 1e-5f)
 *   inv     = 127.0f / a
 *   deq[m]  = a / 127.0f
 *   q[m, k] = min(max(rintf(x[m, k] * inv), -127.0f), 127.0f)   ties to even
 *   Y       = what tcsc_hip_gemm_[prelu_]dev_scaled stores for the int8 X = q,
 *             drow_scale = deq and the same dcol_scale, db, dalpha, ytype and
 *             ldY -- bit for bit.
 *
 * xtype is TSG_X_F32, TSG_X_F16 or TSG_X_BF16; TSG_X_I8 is TSG_ERR_ARG with a
 * message, nothing enqueued (an int8 X has its scale already: _scaled).
 * drow_scale_out may be NULL; otherwise deq is stored to it, float[M] of device
 * memory that needs only 4-byte alignment, and only [0, M) is written.
 * dcol_scale may be NULL: its multiply is then not performed, as on _scaled.
 * A zero row gives q = 0 and Y[m, n] = db[n] (after the PReLU and the cast).
 * A row that holds an inf or a NaN: its own Y row and deq[m] are unspecified;
 * nothing faults, and every other row is bit for bit what it is without it.
 * (rintf(x * inv) can be -0 where an int8 holds 0; a chain starts at +0 and is
 * never -0, so both give the same bits.)
 * How it runs.  A row pass (one wave per row) finds amax and writes inv and
 * deq to a per-handle scratch; the staging pass of the kernel an M picks then
 * quantises each value it loads, so the staged copy holds integer-valued fp32
 * and the kernel runs the chains of an int8 X with the scratch's deq as its
 * row scale.  Such a call is always staged (never the direct-X path).  A
 * small-M walk reads X in place: for it the row pass also writes q as int8 to
 * the scratch and the walk runs on that.  Two launches more than _scaled at
 * most, no synchronisation.
 * As on _scaled: ldY, dY's alignment and the written-range guarantee, the
 * 16-bit neighbour in a shared dword included; stream semantics; isolation
 * from memory outside the operands and from earlier calls; the kernel and
 * image an M picks.  The scratch (three floats per row, and M * K bytes for a
 * walk) is the handle's, grow-only and shared by every stream exactly like the
 * work buffer: tcsc_hip_reserve(h, max_M) sizes it, and a call that would grow
 * it during stream capture is TSG_ERR_ARG naming tcsc_hip_reserve.
 * Out of scope: asymmetric or int4 quantisation, a caller's clip value, the
 * host-pointer calls, the plugin header.  Extension: no reference counterpart. */
int tcsc_hip_gemm_dev_actquant(tsg_tcsc *h, const void *dX, int xtype, float *drow_scale_out,
                               const float *dcol_scale, const float *db, void *dY, int ytype, int64_t ldY,
                               int M, int N, int K, void *stream);
int tcsc_hip_gemm_prelu_dev_actquant(tsg_tcsc *h, const void *dX, int xtype, float *drow_scale_out,
                                     const float *dcol_scale, const float *db, const float *dalpha, void *dY,
                                     int ytype, int64_t ldY, int M, int N, int K, void *stream);

/* The _actquant calls with the RMSNorm that stands in front of the activation
 * quantisation of a BitNet-style layer made inside the call too:
 * x -> x * rsqrt(mean(x^2) + eps) * gamma, then the per-row int8 quantisation,
 * both fused into the passes that read X -- no normalised copy of X in memory.
 *
 * Contract.  All arithmetic is fp32 on the widened X (the widening is exact),
 * every operation rounded once, no fma and no contraction anywhere, the
 * division and the square root IEEE correctly rounded (no reciprocal-square-
 * root shortcut):
 *
 *   sq[k]   = x[m, k] * x[m, k]
 *   s[p]    = ((+0 + sq[p]) + sq[p + 256]) + sq[p + 512] ...   p = 0..255: 256
 *             strided partial sums, each serial in ascending k
 *   ss      = the 256 partials summed by a balanced binary tree, neighbours
 *             first: eight times  s'[p] = s[2p] + s[2p + 1]
 *   ms      = ss / (float)K
 *   rn[m]   = 1.0f / sqrtf(ms + eps)
 *   xn[m,k] = (x[m, k] * rn[m]) * gamma[k]      two roundings, in this order;
 *             dgamma NULL: the second multiply is not performed
 *   Y, deq  = what tcsc_hip_gemm_[prelu_]dev_actquant gives on the fp32 X = xn
 *             with the same other arguments -- bit for bit.
 *
 * The shape of the sum is part of the contract because a sum of squares is not
 * associative; an absent element adds nothing (the same as adding +0), and an
 * aligned and a misaligned X give the same bits.
 * eps must be finite and > 0: anything else is TSG_ERR_ARG with a message that
 * names eps, nothing enqueued.  xtype is TSG_X_F32, TSG_X_F16 or TSG_X_BF16;
 * TSG_X_I8 is refused as on _actquant.
 * dgamma is float[K] of device memory that needs only 4-byte alignment (it may
 * be a slice); it is never written, and nothing outside [dgamma, dgamma + K)
 * reaches Y.
 * K = 0: no sum and no division happen; the call is _actquant at K = 0 (Y = b,
 * deq = 1e-5f / 127).  An all-zero row: rn = 1 / sqrtf(eps), xn = 0, q = 0,
 * Y[m, :] = b.  A row that holds an inf or a NaN, or whose ss overflows: its
 * own Y row and deq[m] are unspecified; nothing faults, and every other row is
 * bit for bit what it is without it.
 * How it runs.  The row pass of _actquant gains a sweep in front that
 * accumulates the 256 partials, reduces them and computes rn; its maximum and,
 * for a small-M walk, its int8 q are taken of xn; it stores rn next to inv and
 * deq in the scratch (three floats per row).  The staging pass then stores
 * q(xn) for each value it loads.  Always staged, no launch and no
 * synchronisation over _actquant.
 * drow_scale_out, dcol_scale, db, dalpha, ytype, ldY, the written-range
 * guarantee, stream semantics, the kernel an M picks, isolation from earlier
 * calls, the scratch's grow-only / tcsc_hip_reserve / capture rules: as on
 * _actquant.
 * Out of scope: a norm without the quantisation, LayerNorm (a mean), a 16-bit
 * gamma, an rn output, the host-pointer calls, the plugin header.  Extension:
 * no reference counterpart. */
int tcsc_hip_gemm_dev_normquant(tsg_tcsc *h, const void *dX, int xtype, const float *dgamma, float eps,
                                float *drow_scale_out, const float *dcol_scale, const float *db, void *dY,
                                int ytype, int64_t ldY, int M, int N, int K, void *stream);
int tcsc_hip_gemm_prelu_dev_normquant(tsg_tcsc *h, const void *dX, int xtype, const float *dgamma, float eps,
                                      float *drow_scale_out, const float *dcol_scale, const float *db,
                                      const float *dalpha, void *dY, int ytype, int64_t ldY, int M, int N, int K,
                                      void *stream);

/* One descriptor call for all of the device calls above, with a fused epilogue
 * after the projection: ReLU or ReLU^2, a gate multiply and a residual add on
 * the finished fp32 value, before the one rounding to the Y type.  A gated FFN
 * computes down(act(gate(x)) * up(x)) and every attention output and FFN down
 * projection is followed by h = h + proj(x); with these three steps in the
 * kernel that stores Y the caller runs no elementwise pass over an [M, N]
 * tensor.  The descriptor maps one to one onto what a device call carries
 * internally, so later features extend this struct and not the list of entry
 * points; the calls above stay as they are.
 *
 * in_mode picks the call the descriptor restates: TSG_IN_PLAIN is _scaled (and
 * with both scales NULL _xy), TSG_IN_ACTQUANT is _actquant, TSG_IN_NORMQUANT is
 * _normquant; act = TSG_ACT_PRELU picks its PReLU twin.
 *
 * Contract.  All arithmetic is fp32, one rounding per operation, no fused
 * multiply-add and no contraction anywhere:
 *
 *   t = what the call of the chosen in_mode adds b to, scaled as on _scaled /
 *       _actquant / _normquant (a blocked handle: after its last block)
 *   y = t + db[n]                                       rounded
 *   a = act(y):  TSG_ACT_NONE   y
 *                TSG_ACT_PRELU  y > 0 ? y : dalpha[n] * y           (as ever)
 *                TSG_ACT_RELU   y > 0 ? y : (y != y ? y : +0.0f)    -0 -> +0, a NaN
 *                                                                   stays a NaN
 *                TSG_ACT_RELU2  r = RELU(y);  r * r     rounded once; may overflow
 *                                                       to +inf
 *   if (dmul) a = a * widen(mul[m * ldmul + n])         rounded
 *   if (dadd) a = a + widen(add[m * ldadd + n])         rounded, never contracted
 *                                                       with the multiply before it
 *   Y[m * ldY + n] = a rounded ONCE to ytype, as on _xy
 *
 * Widening an fp16 or bf16 operand element to fp32 is exact.  A NULL operand
 * means its operation is not performed (not a multiply by 1, nothing added).
 * The operands may hold any IEEE value -- 0, -0, subnormal, inf, NaN -- and Y is
 * the IEEE result of the operations above (a NaN's payload is not promised).
 * Operands.  dmul and dadd are [M, N] device arrays of multype / addtype
 * (tsg_ytype values: fp32, fp16, bf16), each with its own row stride ldmul /
 * ldadd in elements of its own type, >= N.  They need only the alignment of
 * their element (slices are fine) and are never written (but see in place).
 * Isolation: no value outside [m * ld, m * ld + N) of rows 0 .. M-1 reaches Y.
 * Load rule, the mirror of _xy's store rule: a lane's full-width row segment
 * (its 8 to 128 columns inside N) that starts 16-byte aligned is loaded with
 * 16-byte loads, anything else -- the ragged last column tile, an odd ld, a
 * misaligned base -- element by element; the result is the same bit for bit.
 * In place.  dadd may be exactly dY, with addtype == ytype and ldadd == ldY:
 * h += proj(x).  The same holds for dmul.  Every element is then read by the
 * lane that stores it, before the store.  Any other overlap between Y and an
 * operand is the caller's error: the result is unspecified, nothing faults.
 * Legacy equivalence.  With act TSG_ACT_NONE or TSG_ACT_PRELU and both
 * operands NULL the call IS the existing call of its in_mode: the same path,
 * the same kernel arguments and flags, the same bits; nothing new is launched.
 * Errors.  TSG_ERR_ARG with a message that names the field, nothing enqueued:
 * a NULL d; struct_size != sizeof(tsg_gemm_ex); reserved != 0; an in_mode, act,
 * xtype, ytype, multype or addtype outside its enum; ldY, or the ld of a passed
 * operand, smaller than N; TSG_ACT_PRELU without dalpha; TSG_X_I8 in a
 * quantising in_mode; in TSG_IN_NORMQUANT an eps that is not finite and > 0; a
 * field of another in_mode that is not NULL (dgamma outside NORMQUANT,
 * drow_scale in a quantising in_mode, drow_scale_out in PLAIN).  dalpha is read
 * for TSG_ACT_PRELU only and otherwise ignored.  tsg_gemm_ex_check performs
 * exactly these checks on the host -- no device, no handle -- and
 * tcsc_hip_gemm_dev_ex calls it right after its null-handle check.
 * As on the call of the same in_mode: stream semantics, tcsc_hip_reserve and
 * graph capture, the kernel and image an M picks, the direct-X rule, the work
 * buffer and the scratch, the written-range guarantee of Y.  The epilogue adds
 * no allocation, no launch and no synchronisation: the operands are two more
 * pointers of the kernel that stores Y.
 * Out of scope: SiLU, GELU and SwiGLU (a bit-exact exp needs a contract of its
 * own); quantising Y; operands broadcast per row or per column; the
 * host-pointer calls; the plugin header (tcsc_hip_plugin.hpp); ShardedTCSC.
 * Extension: no reference counterpart.
 *
 * Layout (LP64, no padding, 144 bytes): byte offset of every field on the
 * right.  A later version may only append fields and grow struct_size. */
enum tsg_act { TSG_ACT_NONE = 0, TSG_ACT_PRELU = 1, TSG_ACT_RELU = 2, TSG_ACT_RELU2 = 3 };
enum tsg_in_mode { TSG_IN_PLAIN = 0, TSG_IN_ACTQUANT = 1, TSG_IN_NORMQUANT = 2 };

typedef struct tsg_gemm_ex {
    uint32_t struct_size;       /*   0  sizeof(tsg_gemm_ex); anything else: TSG_ERR_ARG naming struct_size */
    int32_t in_mode;            /*   4  tsg_in_mode */
    const void *dX;             /*   8  M x K row-major elements of xtype */
    int32_t xtype;              /*  16  tsg_xtype */
    int32_t act;                /*  20  tsg_act */
    const float *dgamma;        /*  24  NORMQUANT only (as on _normquant, may be NULL there); else NULL */
    float eps;                  /*  32  NORMQUANT only; ignored otherwise */
    int32_t ytype;              /*  36  tsg_ytype */
    const float *drow_scale;    /*  40  PLAIN only (as on _scaled); NULL in the quantising modes */
    float *drow_scale_out;      /*  48  quantising modes only (as on _actquant); NULL in PLAIN */
    const float *dcol_scale;    /*  56  float[N] or NULL */
    const float *db;            /*  64  float[N] */
    const float *dalpha;        /*  72  float[N]; read for TSG_ACT_PRELU only (then required) */
    const void *dmul;           /*  80  gate operand, [M, N] of multype; NULL: no multiply */
    int64_t ldmul;              /*  88  elements of multype per row of dmul, >= N */
    const void *dadd;           /*  96  residual operand, [M, N] of addtype; NULL: no add */
    int64_t ldadd;              /* 104  elements of addtype per row of dadd, >= N */
    int32_t multype;            /* 112  tsg_ytype values */
    int32_t addtype;            /* 116  tsg_ytype values */
    void *dY;                   /* 120  M x N elements of ytype */
    int64_t ldY;                /* 128  elements of ytype per row of dY, >= N */
    uint64_t reserved;          /* 136  must be 0 */
} tsg_gemm_ex;

int tcsc_hip_gemm_dev_ex(tsg_tcsc *h, const tsg_gemm_ex *d, int M, int N, int K, void *stream);
/* host only: no device, no handle */
int tsg_gemm_ex_check(const tsg_gemm_ex *d, int M, int N, int K);

/* Pre-allocates the per-handle work buffer for row counts up to max_M and, on
 * the weight-compiled kernel, compiles every code image a call with M <= max_M
 * rows runs (and the small-M images), so no later such call allocates or
 * compiles (graph capture).  It covers the host-pointer pipeline's M chunks
 * too (each chunk is a call with fewer rows). */
int tcsc_hip_reserve(tsg_tcsc *h, int max_M);

/* ---- introspection ------------------------------------------------------- */
typedef struct tsg_info {
    int32_t K, N, device, abi_version;
    int64_t nnz_pos, nnz_neg;
    int64_t tcsc_bytes;     /* TCSC::getDataStructureSize() (TCSC.h:43-49) */
    int64_t image_bytes;    /* bytes of the device image (segments + entries) */
    int64_t work_bytes;     /* current work-buffer size */
    int32_t chunk_rows;     /* K rows per LDS chunk of the image registration loaded
                               (the 64-row image's 128 x 8 shape when it could, else the
                               128-row image's 64 x 8, or rx); calls may compile others */
    int32_t tile_rows;      /* M rows per workgroup (same image) */
    int32_t tile_cols;      /* N columns per workgroup (same image) */
    int32_t reserved;
} tsg_info;
int tcsc_hip_info(const tsg_tcsc *h, tsg_info *out);

/* DataStructureInterface::getVectorRepresentation (DataStructureInterface.hpp:13)
 * for the registered matrix: dense K x N row-major ternary ints. */
int tcsc_hip_to_dense(const tsg_tcsc *h, int32_t *W, int K, int N);

/* Kernel timing: when enabled, HIP events bracket every launch of the main
 * (dominant) kernel on its own stream; totals accumulate until reset. */
int tcsc_hip_set_timing(tsg_tcsc *h, int enable);
int tcsc_hip_kernel_time(tsg_tcsc *h, double *total_ms, int64_t *launches, int reset);

/* Name of the device kernel this handle launches (the one timed above):
 * "tsg_jit_kernel" (default: W compiled into gfx950 code at registration) or
 * "tsg_tcsc_rx_kernel" (the register-X walk: W too large for one compiled
 * image, a generated image the loader refused -- logged on stderr -- or
 * TSG_KERNEL=rx at registration). */
const char *tcsc_hip_kernel_name(const tsg_tcsc *h);

/* The device kernel a call with M rows launches on this handle (calls pick
 * per M): "tsg_jit64_kernel" (the weight-compiled 64-row image:
 * one M row per lane; the default for M <= 512 and for configs[2]),
 * "tsg_jit_kernel" (the weight-compiled 128-row image; also what a call runs
 * after the image it picked could not be loaded -- logged on stderr),
 * "tsg_tcsc_ell_kernel" / "tsg_tcsc_ell_pc_kernel" (the small-M walks) or
 * "tsg_tcsc_rx_kernel". */
const char *tcsc_hip_call_kernel(const tsg_tcsc *h, int M);

const char *tcsc_hip_last_error(void);
int tcsc_hip_device_count(int *count);

/* ---- host-side helpers (no GPU needed) -------------------------------------
 * Column slice [n0, n1) of a TCSC, rebased to start at 0: the shard a rank
 * owns when W's columns are split across GPUs (Y[:,n] depends only on
 * column n).  Pass NULL outputs to query nnz_pos/nnz_neg of the slice. */
int tsg_tcsc_slice(const int32_t *col_start_pos, const int32_t *col_start_neg,
                   const int32_t *row_index_pos, const int32_t *row_index_neg, int N,
                   int n0, int n1, int32_t *out_csp, int32_t *out_csn,
                   int32_t *out_rip, int32_t *out_rin, int64_t *nnz_pos, int64_t *nnz_neg);

/* Checks the TCSC invariants the kernels rely on: monotone col_start of
 * length N+1 starting at 0, 0 <= k < K, strictly ascending k per column, no
 * k both +1 and -1 in a column.  TSG_OK or TSG_ERR_ARG (with message). */
int tsg_tcsc_validate(const int32_t *col_start_pos, const int32_t *col_start_neg,
                      const int32_t *row_index_pos, const int32_t *row_index_neg, int K, int N);

/* Synthetic W with the distribution of generateSparseMatrix
 * (cpp_impl/sparseUtils.h:52-87), emitted directly as TCSC restricted to the
 * columns [n0, n1) (rebased).  Deterministic in `seed` (splitmix64 stream,
 * the same draw sequence as the test oracle's dense generator).  Call with
 * NULL arrays to get nnz_pos/nnz_neg, then again to fill. */
int tsg_gen_tcsc(int K, int N, int s, uint64_t seed, int n0, int n1,
                 int32_t *csp, int32_t *csn, int32_t *rip, int32_t *rin,
                 int64_t *nnz_pos, int64_t *nnz_neg);

/* Format conversions between TCSC and CSC + base-3 packed values (see
 * tcsc_hip_create_csc_packed).  NULL outputs query the sizes only.
 * packed has ceil(nnz/5) bytes. */
int tsg_tcsc_to_csc_packed(const int32_t *col_start_pos, const int32_t *col_start_neg,
                           const int32_t *row_index_pos, const int32_t *row_index_neg, int N,
                           int32_t *col_ptr, int32_t *row_idx, uint8_t *packed, int64_t *nnz);
int tsg_csc_packed_to_tcsc(const int32_t *col_ptr, const int32_t *row_idx, const uint8_t *packed,
                           int N, int32_t *col_start_pos, int32_t *col_start_neg,
                           int32_t *row_index_pos, int32_t *row_index_neg, int64_t *nnz_pos,
                           int64_t *nnz_neg);

/* Checks BlockedTCSC<B> arrays (layout as tcsc_hip_create_blocked): monotone
 * column starts, every row inside its block, ascending, no row both +1 and -1. */
int tsg_blocked_tcsc_validate(const int32_t *col_start_pos, const int32_t *col_start_neg,
                              const int32_t *row_index_pos, const int32_t *row_index_neg, int K, int N,
                              int B);

/* X[i] = integer-valued fp32 U{-range..range} (initX, sparseUtils.h:6-23). */
int tsg_gen_x(int64_t len, int range, uint64_t seed, float *X);

#ifdef __cplusplus
}
#endif
#endif /* TERNARY_SPGEMM_H */
