// The thread-per-pair kernels of a super-step compiled for ONE horizon: bmpc_pair_n20.hip, bmpc_pair_n30.hip define BMPC_FIXED_N and
// include this file, nothing else.  The bodies are those of bmpc_pair_kernels.hpp, instantiated on PipeArgsN<BMPC_FIXED_N>
// (bmpc_pipeline.hpp): the slot-major strides NP = N - 1 and N are constants, so a row group is one base register plus immediate
// offsets instead of one 64-bit address add per row, and the uniform products (slot * NP) are gone.  Integer address arithmetic
// only: with -ffp-contract=on every floating-point expression is contracted as in the generic kernels, and the results are bitwise
// theirs (tests/test_fixed_stride_emu.py on the CPU, tests/test_gpu_fixed_stride.py on the GPU).
// Only what bmpc_pipeline.hip dispatches is instantiated (launch_eval, launch_direction, launch_trial; BMPC_FIXED_STRIDE=0 in the
// environment runs the generic kernels everywhere).  bmpc_k_curv as a kernel of its own (BMPC_SPLIT_LAUNCHES=1) has no fixed-horizon
// form -- with the strides assumed constant it spilled two registers where the generic one spills none --; inside
// bmpc_k_eval_curv_split, whose registers are those of k_eval, its body takes the constants like the other two.
#include "bmpc_platform_hip.hpp"

#define BMPC_NT 64
#include "bmpc_pair_kernels.hpp"
#include "bmpc_internal.hpp"

#ifndef BMPC_FIXED_N
#error "BMPC_FIXED_N: the horizon this translation unit is compiled for"
#endif

using namespace bmpc;

#define BMPC_CAT_(a, b) a##b
#define BMPC_CAT(a, b) BMPC_CAT_(a, b)
#define KN(stem) BMPC_CAT(BMPC_CAT(stem, _n), BMPC_FIXED_N)      // bmpc_k_step -> bmpc_k_step_n20: the profile tools match the stem

// the launch argument read through the fixed-horizon view
#define DVN(H) (*reinterpret_cast<const PipeArgsN<BMPC_FIXED_N>*>(&(H)))
static_assert(sizeof(PipeArgsN<BMPC_FIXED_N>) == sizeof(PipeArgsH), "the fixed-horizon view adds nothing to the argument block");

extern __shared__ __attribute__((aligned(16))) double bmpc_dyn_lds[];

__global__ __launch_bounds__(64, 1) void KN(bmpc_k_points)(PipeArgsH H) { k_points_body(DVN(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds); }
__global__ __launch_bounds__(64, 1) void KN(bmpc_k_pose)(PipeArgsH H) { k_pose_body(DVN(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds); }
__global__ __launch_bounds__(64, 1) void KN(bmpc_k_eval_main)(PipeArgsH H) { k_eval_body<1>(DVN(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds); }
__global__ __launch_bounds__(64, 1) void KN(bmpc_k_eval_chain)(PipeArgsH H) { k_eval_body<2>(DVN(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds); }
__global__ __launch_bounds__(64, 1) void KN(bmpc_k_points_pose)(PipeArgsH H, int nw) {
    if ((int)blockIdx.x < nw) k_points_body(DVN(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds);
    else k_pose_body(DVN(H), (int)blockIdx.x - nw, threadIdx.x, (LDSD*)bmpc_dyn_lds);
}
__global__ __launch_bounds__(64, 1) void KN(bmpc_k_eval_curv_split)(PipeArgsH H, int nw) {
    if ((int)blockIdx.x < nw) k_eval_body<1>(DVN(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds);
    else if ((int)blockIdx.x < 2 * nw) k_eval_body<2>(DVN(H), (int)blockIdx.x - nw, threadIdx.x, (LDSD*)bmpc_dyn_lds);
    else k_curv_body(DVN(H), (int)blockIdx.x - 2 * nw, threadIdx.x, (LDSD*)bmpc_dyn_lds);
}
__global__ __launch_bounds__(64, 1) void KN(bmpc_k_step)(PipeArgsH H) { k_step_body(DVN(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds); }
__global__ __launch_bounds__(64, 1) void KN(bmpc_k_trial)(PipeArgsH H) { k_trial_body_t<1>(DVN(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds); }
__global__ __launch_bounds__(64 * TRIAL_SPEC, 1) void KN(bmpc_k_trial_spec)(PipeArgsH H) {
    k_trial_spec_body(DVN(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds);
}

// one launch of kernel `kern` (bmpc_internal.hpp, FX_*) with the grid, block and dynamic LDS the caller computed as for the generic kernel
extern "C" void KN(bmpc_pair_launch)(int kern, const PipeArgsH* A, int nw, unsigned nb, unsigned nt, size_t lds_bytes, hipStream_t st) {
    if (nb == 0) return;
    switch (kern) {
    case FX_POINTS: hipLaunchKernelGGL(KN(bmpc_k_points), dim3(nb), dim3(nt), lds_bytes, st, *A); break;
    case FX_POSE: hipLaunchKernelGGL(KN(bmpc_k_pose), dim3(nb), dim3(nt), lds_bytes, st, *A); break;
    case FX_EVAL_MAIN: hipLaunchKernelGGL(KN(bmpc_k_eval_main), dim3(nb), dim3(nt), lds_bytes, st, *A); break;
    case FX_EVAL_CHAIN: hipLaunchKernelGGL(KN(bmpc_k_eval_chain), dim3(nb), dim3(nt), lds_bytes, st, *A); break;
    case FX_POINTS_POSE: hipLaunchKernelGGL(KN(bmpc_k_points_pose), dim3(nb), dim3(nt), lds_bytes, st, *A, nw); break;
    case FX_EVAL_CURV_SPLIT: hipLaunchKernelGGL(KN(bmpc_k_eval_curv_split), dim3(nb), dim3(nt), lds_bytes, st, *A, nw); break;
    case FX_STEP: hipLaunchKernelGGL(KN(bmpc_k_step), dim3(nb), dim3(nt), lds_bytes, st, *A); break;
    case FX_TRIAL: hipLaunchKernelGGL(KN(bmpc_k_trial), dim3(nb), dim3(nt), lds_bytes, st, *A); break;
    case FX_TRIAL_SPEC: hipLaunchKernelGGL(KN(bmpc_k_trial_spec), dim3(nb), dim3(nt), lds_bytes, st, *A); break;
    default: abort();      // (a kernel that has no fixed-horizon form is the caller's error: nothing falls back quietly)
    }
}
