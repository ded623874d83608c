// The sigmoid of the tail kernels (kgnn_tail.hip, kgnn_atom_contrib.hip): one definition, so that swish(pre) is the same
// bits wherever it is taken.
#pragma once
#include <hip/hip_runtime.h>

namespace mkgnn {

// sigmoid on the transcendental unit: v_exp_f32 and v_rcp_f32 (1 ulp each) instead of the library's expf and an IEEE division --
// ~6 instructions for ~60.  The tail's middle kernel evaluates two of them per (atom, hidden unit) and, measured by compiling the
// phases out, was BOUND by them (31 of its 64 us).  Relative error <= 2^-22 + |v| 2^-23: 2e-6 at |v| = 16, against the 1e-5 the
// readout is held to (tests/test_tail.py: against float64 autograd of the reference's formula).
__device__ __forceinline__ float sigmoidf_(float v) {
    const float e = __builtin_amdgcn_exp2f(-1.44269504088896340736f * v);      // e^-v  (inf for v << 0: the reciprocal is then 0)
    return __builtin_amdgcn_rcpf(1.f + e);
}

}  // namespace mkgnn
