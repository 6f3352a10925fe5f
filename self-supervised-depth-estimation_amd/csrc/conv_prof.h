// Measurement hook of the convolution launchers (conv_prof.hip: dc_conv_profile_enable / dc_conv_profile_collect): a hipEvent pair
// around the main kernel of a launch, per kernel family.
#pragma once
#include <hip/hip_runtime.h>

namespace dc {

// the `kind` of dc_conv_profile_collect (bench.py passes these values as integers: they stay)
enum ConvProfKind {
    PROF_WINO_PS = 0,       // wino_ps_kernel / wino4 (forward, data gradient)
    PROF_WINO_WGRAD = 1,    // wino_wgrad_kernel
    PROF_C3B_CONV = 2,      // c3b_conv_kernel (bf16 forward / data gradient)
    PROF_C3B_WGRAD = 3,     // c3b_wgrad_kernel (bf16)
    PROF_G1 = 4,            // the 1x1 GEMM family (g1_*)
    PROF_CG = 5,            // cg_* (3x3 / 2)
    PROF_STEM = 6,          // stem (7x7 / 2)
    PROF_G1X3 = 7,          // g1x3 (split-operand 1x1 GEMMs)
    PROF_KINDS
};

// -> the end event (conv_prof_end records it) or nullptr: the hook is off, this launch is not sampled, or the events are used up
hipEvent_t conv_prof_begin(ConvProfKind kind, double algorithmic_flops, double executed_flops, double algorithmic_bytes, hipStream_t st);
void conv_prof_end(hipEvent_t e, hipStream_t st);

}  // namespace dc
