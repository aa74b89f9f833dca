// Which kernels are compiled without packed fp32 (v_pk_fma_f32 / v_pk_add_f32 / v_pk_mul_f32).
//
// A packed fp32 instruction beside MFMAs holds the SIMD's issue for longer than the two single instructions it replaces, and
// the f4 arithmetic of the decoder bodies (tri_gather_reduce, the layer-boundary accumulations, load_bias, the embedding and output layers) sits
// between the MFMAs of the chains.  NSK_SINGLE_ISSUE in front of a __global__ function takes the packed-fp32-ops feature away from that kernel alone:
// every body is __forceinline__ and is selected with the features of the kernel it lands in, so one body can be single-issue in a decoder kernel
// and packed in an evaluation kernel.  Each half of a v_pk_fma_f32 is the IEEE fma of a v_fma_f32: the results are the same bits
// (tools/ab_outputs.py, tools/ab_outputs_steps.py).  The host pass sees no attribute: x86 has no such feature.
// Kept packed, because the same-box A/B showed no gain: k_decode_bwd_frozen, k_decode_bwd_track, k_decode_bwd_multi, and with
// them the kernels without matrix instructions and the one-decoder / fp32 measuring sticks nobody times.  A callee that is not always_inline
// (HIP's atomicAdd(float*, float), __syncthreads) can stay a CALL in a kernel whose features differ from its own: k_decode_bwd_track kept six such
// calls when it was tried; the three kernels below have none (tools/isa_diff.py lists functions that are no kernels).
// tools/isa_count.py --no-packed-f32 k_decode_ on the `make asm` text is the check that this still holds after a body was touched.
#pragma once
#if defined(__HIP_DEVICE_COMPILE__)
#define NSK_SINGLE_ISSUE __attribute__((target("no-packed-fp32-ops")))
#else
#define NSK_SINGLE_ISSUE
#endif
