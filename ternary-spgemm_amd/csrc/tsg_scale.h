// tsg_scale.h -- device side of the epilogue scales (include/ternary_spgemm.h
// tcsc_hip_gemm_dev_scaled): a per-row scale (float[M], the dequantisation
// scale of int8 activations) and a per-column scale (float[N], the weight
// scale of W ~ gamma * T), applied to the finished fp32 chain before + b[n].
// Every kernel that stores Y branches once, on whether the call has a scale
// (wave-uniform: the kYScaled flag its launcher sets in the ytype argument,
// tsg_internal.h; rx tests the two pointers), and comes here only then; the
// ELL walk has a second kernel for it (tsg_tcsc_ell_scaled_kernel).  With both
// NULL every kernel runs the code it ran before.
#pragma once

#include <hip/hip_runtime.h>

namespace tsg {

// y = ((chain * rs) * cs) + b: fp32, one rounding per operation, a missing
// scale's multiply not performed.  hipcc contracts a * b + c into one fma by
// default (-ffp-contract=fast-honor-pragmas), and __fmul_rn / __fadd_rn are
// plain * and + in its headers, contracted like any other: the pragma is what
// keeps the roundings apart.  It takes the `contract` flag off these three
// operations themselves, wherever they are inlined, and the backend fuses only
// operations that carry it.  (The Makefile's -ffp-contract=off says the same
// for the whole build; this header does not depend on it.)
__device__ __forceinline__ float scale_bias(float chain, bool has_rs, float rs, bool has_cs, float cs, float b)
{
#pragma clang fp contract(off)
    float t = chain;
    if (has_rs) t = t * rs;
    if (has_cs) t = t * cs;
    return t + b;
}

}  // namespace tsg
