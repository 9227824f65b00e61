// Kernels of the batch-synchronous pipeline engine (gfx950) + their launch functions.
// Device code: bmpc_stage.hpp / bmpc_pair_kernels.hpp / bmpc_ric_kernel.hpp.  Host sequencing:
// bmpc_capi.hip (pipe_solve).
#include "bmpc_platform_hip.hpp"
#include <atomic>
#include <cstdlib>
#include <utility>

#define BMPC_NT 64
#include "bmpc_pair_kernels.hpp"
#include "bmpc_ric_kernel.hpp"
#include "bmpc_stage_matrix.hpp"
#include "bmpc_internal.hpp"
#include "../../include/boundmpc.h"

using namespace bmpc;

#ifndef BMPC_TRIAL_NW
#define BMPC_TRIAL_NW 1      // wavefronts per group of pairs in k_trial: 1 = one walks all rows, 4 = one part of the walk each (measured, not kept: EXPERIMENTS.md)
#endif

// the launch argument is the host view of the argument block; device code reads it through the
// layout-identical view whose pointers are global-address-space qualified
#define DV(H) (*reinterpret_cast<const PipeArgs*>(&(H)))

// thread-per-pair kernels: one wavefront per workgroup, floor(64/(N-1)) instances per wavefront; compiled for one wavefront per SIMD
// (the second launch bound: the allocator may use the whole register file -- two wavefronts per SIMD spill, EXPERIMENTS.md)
__global__ __launch_bounds__(64) void bmpc_k_init_inst(PipeArgsH H) { k_init_inst_body(DV(H), blockIdx.x * 64 + threadIdx.x); }
// dynamic LDS of the thread-per-pair kernels: [emitter tile (k_eval, k_curv)] [staged parameter vectors]
extern __shared__ __attribute__((aligned(16))) double bmpc_dyn_lds[];
__global__ __launch_bounds__(64, 1) void bmpc_k_init(PipeArgsH H) { k_init_body(DV(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds); }
__global__ __launch_bounds__(64, 1) void bmpc_k_pose(PipeArgsH H) { k_pose_body(DV(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds); }
__global__ __launch_bounds__(64, 1) void bmpc_k_eval(PipeArgsH H) {
    k_eval_body<0>(DV(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds);
}
__global__ __launch_bounds__(64, 1) void bmpc_k_points(PipeArgsH H) { k_points_body(DV(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds); }
__global__ __launch_bounds__(64, 1) void bmpc_k_curv(PipeArgsH H) {
    __shared__ double lds[EM_DOUBLES + 8];
    k_curv_body(DV(H), blockIdx.x, threadIdx.x, (LDSD*)lds);
}
// Two pairs of kernels of a super-step do not depend on each other -- k_points / k_pose (both read the iterate, write disjoint side
// fields) and k_eval / k_curv (disjoint fields of the stage record) -- and are launched as ONE grid each: the first nw workgroups
// run one body, the rest the other.  Same work in the bulk regime, two launches fewer; in the straggler tail, where a launch costs
// its single-thread latency, the two bodies run side by side (k_points 39 + k_pose 41 us -> 41, k_eval 113 + k_curv ~50 -> 113).
// BMPC_SPLIT_LAUNCHES=1 in the environment keeps the four launches (per-kernel profiles).
__global__ __launch_bounds__(64, 1) void bmpc_k_points_pose(PipeArgsH H, int nw) {
    if ((int)blockIdx.x < nw) k_points_body(DV(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds);
    else k_pose_body(DV(H), (int)blockIdx.x - nw, threadIdx.x, (LDSD*)bmpc_dyn_lds);
}
// What lets k_eval and k_curv share a grid: k_curv reads nothing k_eval writes -- the iterate, the curvature list (k_points) and the
// partials PT_FORCE (k_pose, k_points) and PT_SIG (k_pose), all complete before this launch -- and writes record fields of its own.
__global__ __launch_bounds__(64, 1) void bmpc_k_eval_curv(PipeArgsH H, int nw) {
    if ((int)blockIdx.x < nw) k_eval_body<0>(DV(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds);
    else k_curv_body(DV(H), (int)blockIdx.x - nw, threadIdx.x, (LDSD*)bmpc_dyn_lds);
}
// k_eval as two wavefronts side by side (up to BMPC_EVAL_SPLIT_WGS groups of pairs: always, by default) -- everything but the chained block /
// the chained block alone (bmpc_pair_kernels.hpp, k_eval_body) -- beside k_curv
__global__ __launch_bounds__(64, 1) void bmpc_k_eval_curv_split(PipeArgsH H, int nw) {
    if ((int)blockIdx.x < nw) k_eval_body<1>(DV(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds);
    else if ((int)blockIdx.x < 2 * nw) k_eval_body<2>(DV(H), (int)blockIdx.x - nw, threadIdx.x, (LDSD*)bmpc_dyn_lds);
    else k_curv_body(DV(H), (int)blockIdx.x - 2 * nw, threadIdx.x, (LDSD*)bmpc_dyn_lds);
}
// (the two bodies as kernels of their own: per-kernel profiles, BMPC_SPLIT_LAUNCHES=1)
__global__ __launch_bounds__(64, 1) void bmpc_k_eval_main(PipeArgsH H) { k_eval_body<1>(DV(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds); }
__global__ __launch_bounds__(64, 1) void bmpc_k_eval_chain(PipeArgsH H) { k_eval_body<2>(DV(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds); }
#ifndef BMPC_EVAL_SPLIT_WGS
// groups of pairs up to which bmpc_k_eval_curv_split replaces bmpc_k_eval_curv (0 = never).  Always: built for the latency of the tail
// regime (a third of k_eval's arithmetic beside the rest), the two lighter bodies also beat the one-wavefront kernel in the bulk regime
// (544 - 566 -> 493 - 497 us at 8192 live, bench 124.3 - 125.0 -> 127.4 - 127.9 k solves/s in an ABAB run on one box)
#define BMPC_EVAL_SPLIT_WGS (1 << 30)
#endif
#ifndef BMPC_RIC_NT
#define BMPC_RIC_NT 128     // lanes cooperating on one instance in the Riccati kernel
#endif
#ifndef BMPC_RIC_SPEC_BELOW
#define BMPC_RIC_SPEC_BELOW 512     // live instances below which bmpc_k_ric_att(_thr) + bmpc_k_ric_sel replace bmpc_k_ric_lat / bmpc_k_ric (2 .. 5 attempts per instance)
#endif
#ifndef BMPC_RIC_WPE
#define BMPC_RIC_WPE 3      // wavefronts per SIMD the throughput variant is compiled for
#endif
// disable_tail_calls: a call site marked `tail` (LLVM marks every call that is handed no pointer into the caller's stack frame)
// makes the callee save and restore the 64 callee-saved VGPRs it uses (the register-usage propagation that lets the sweeps clobber
// them is skipped for functions with such call sites): 128 scratch accesses per lane and sweep
__global__ __launch_bounds__(BMPC_RIC_NT, BMPC_RIC_WPE) __attribute__((disable_tail_calls)) void bmpc_k_ric(PipeArgsH H) {          // throughput variant: 6 workgroups per CU (3 wavefronts / SIMD)
    __shared__ __attribute__((aligned(16))) double lds[RIC_LDS_DOUBLES];
    k_ric_body<BMPC_RIC_NT, true>(ric_kernel_args(), blockIdx.x, threadIdx.x, (LDSD*)lds);
}
__global__ __launch_bounds__(BMPC_RIC_NT, 1) __attribute__((disable_tail_calls)) void bmpc_k_ric_lat(PipeArgsH H) {      // latency variant for the straggler tail
    __shared__ __attribute__((aligned(16))) double lds[RIC_LDS_DOUBLES];
    k_ric_body<BMPC_RIC_NT, false>(ric_kernel_args(), blockIdx.x, threadIdx.x, (LDSD*)lds);
}
// the speculative pair for the deep tail (few instances alive, each on a CU of its own): RIC_NATT factorisation attempts of every
// instance side by side, then the selection + forward start (bmpc_ric_kernel.hpp)
__global__ __launch_bounds__(BMPC_RIC_NT, 1) __attribute__((disable_tail_calls)) void bmpc_k_ric_att(PipeArgsH H) {
    __shared__ __attribute__((aligned(16))) double lds[RIC_LDS_DOUBLES];
    k_ric_att_body<BMPC_RIC_NT, false>(ric_kernel_args(), blockIdx.x, threadIdx.x, (LDSD*)lds);
}
// (the same with the throughput compilation of the sweeps: more attempts than 512 workgroups -- two per CU -- can hold)
__global__ __launch_bounds__(BMPC_RIC_NT, BMPC_RIC_WPE) __attribute__((disable_tail_calls)) void bmpc_k_ric_att_thr(PipeArgsH H) {
    __shared__ __attribute__((aligned(16))) double lds[RIC_LDS_DOUBLES];
    k_ric_att_body<BMPC_RIC_NT, true>(ric_kernel_args(), blockIdx.x, threadIdx.x, (LDSD*)lds);
}
__global__ __launch_bounds__(BMPC_RIC_NT, 1) __attribute__((disable_tail_calls)) void bmpc_k_ric_sel(PipeArgsH H) {
    __shared__ __attribute__((aligned(16))) double lds[RIC_LDS_DOUBLES];
    k_ric_body<BMPC_RIC_NT, false, true>(ric_kernel_args(), blockIdx.x, threadIdx.x, (LDSD*)lds);
}
#ifndef BMPC_RIC_LAT_BELOW
#define BMPC_RIC_LAT_BELOW 512      // fewer active instances than this: the latency variant (every wavefront has a SIMD to itself anyway)
#endif
__global__ __launch_bounds__(64) void bmpc_k_fwd(PipeArgsH H) {
    __shared__ __attribute__((aligned(16))) double lds[FW_LDS_DOUBLES];
    k_fwd_body(DV(H), blockIdx.x, threadIdx.x, (LDSD*)lds);
}
__global__ __launch_bounds__(64, 1) void bmpc_k_step(PipeArgsH H) { k_step_body(DV(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds); }
__global__ __launch_bounds__(64) void bmpc_k_init_fin(PipeArgsH H) { k_init_fin_body(DV(H), blockIdx.x * 64 + threadIdx.x); }
__global__ __launch_bounds__(64) void bmpc_k_admit(PipeArgsH H) { k_admit_body(DV(H), blockIdx.x * 64 + threadIdx.x); }
__global__ void bmpc_k_pool_reset(PipeArgsH H, int done_too) { if (threadIdx.x == 0 && blockIdx.x == 0) k_pool_reset_body(DV(H), done_too != 0); }
__global__ __launch_bounds__(64 * BMPC_TRIAL_NW, BMPC_TRIAL_NW == 4 ? 2 : 1) void bmpc_k_trial(PipeArgsH H) {
    k_trial_body_t<BMPC_TRIAL_NW>(DV(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds);
}
// the line search of the tail regime: four step lengths side by side, one wavefront (one SIMD) each (bmpc_pair_kernels.hpp)
__global__ __launch_bounds__(64 * TRIAL_SPEC, 1) void bmpc_k_trial_spec(PipeArgsH H) {
    k_trial_spec_body(DV(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds);
}
#ifndef BMPC_TRIAL_SPEC_WGS
#define BMPC_TRIAL_SPEC_WGS 256       // groups of pairs up to which bmpc_k_trial_spec replaces bmpc_k_trial: one workgroup (four SIMDs) per CU (0 = never)
#endif
__global__ void bmpc_k_rotate(PipeArgsH H) { if (threadIdx.x == 0 && blockIdx.x == 0) k_rotate_body(DV(H)); }
__global__ __launch_bounds__(64, 1) void bmpc_k_out(PipeArgsH H) { k_out_body(DV(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds); }
__global__ __launch_bounds__(64, 1) void bmpc_k_mult(PipeArgsH H) { k_mult_body(DV(H), blockIdx.x, threadIdx.x, (LDSD*)bmpc_dyn_lds); }
__global__ __launch_bounds__(64) void bmpc_k_mult_sweep(PipeArgsH H) { k_mult_sweep_body(DV(H), blockIdx.x * 64 + threadIdx.x); }
__global__ __launch_bounds__(64) void bmpc_k_fin(PipeArgsH H) { k_fin_body(DV(H), blockIdx.x * 64 + threadIdx.x); }

#define LAUNCH(kern, nb, nt)                                            \
    do {                                                                \
        if ((nb) > 0) hipLaunchKernelGGL(kern, dim3(nb), dim3(nt), 0, st, *A); \
    } while (0)
#define LAUNCH_DYN(kern, nb, nt, lds_doubles)                           \
    do {                                                                \
        if ((nb) > 0) hipLaunchKernelGGL(kern, dim3(nb), dim3(nt), (lds_doubles) * sizeof(double), st, *A); \
    } while (0)

// first fill of the pool: n0 = min(B, slots) slots take the first n0 input rows (cnt[0] = cnt[6] = cnt[9] = n0 set by the host)
extern "C" hipError_t bmpc_pipe_launch_init(const PipeArgsH* A, int n0, hipStream_t st) {
    LAUNCH(bmpc_k_init_inst, (n0 + 63) / 64, 64);
    LAUNCH_DYN(bmpc_k_init, waves_for(A->N, n0), 64, pair_lds_doubles(A->N, false));
    LAUNCH(bmpc_k_init_fin, (n0 + 63) / 64, 64);
    hipLaunchKernelGGL(bmpc_k_pool_reset, dim3(1), dim3(64), 0, st, *A, 0);
    return hipGetLastError();
}

// retirement of the instances that finished (at most n_max), first half: outputs in the reference layout
extern "C" hipError_t bmpc_pipe_launch_retire_out(const PipeArgsH* A, int n_max, hipStream_t st) {
    LAUNCH_DYN(bmpc_k_out, waves_for(A->N, n_max), 64, pair_lds_doubles(A->N, false));
    LAUNCH(bmpc_k_fin, (n_max + 63) / 64, 64);
    return hipGetLastError();
}
// second half: while input rows are left (or, closed loop, the row has its next problem ready) the slots are refilled and
// initialised.  A solve of B <= slots instances without a retire hook never refills.
extern "C" hipError_t bmpc_pipe_launch_retire_admit(const PipeArgsH* A, int n_max, int refill, hipStream_t st) {
    LAUNCH(bmpc_k_admit, (n_max + 63) / 64, 64);
    if (refill) {
        LAUNCH_DYN(bmpc_k_init, waves_for(A->N, n_max), 64, pair_lds_doubles(A->N, false));
        LAUNCH(bmpc_k_init_fin, (n_max + 63) / 64, 64);
    }
    hipLaunchKernelGGL(bmpc_k_pool_reset, dim3(1), dim3(64), 0, st, *A, 1);
    return hipGetLastError();
}

// The pair kernels compiled for the workspace's horizon (bmpc_pair_fixed.hpp: the SoA strides are compile-time constants), or null:
// the generic kernels of this file.  Slot-major layout (NP = N - 1) and N = 20 or 30 only.  BMPC_FIXED_STRIDE=0 in the environment
// (read once): the generic kernels everywhere -- A/B runs and the test that the two agree bitwise.
static bmpc_pair_launcher fixed_launcher(const PipeArgsH* A) {
    static const int fixed_stride = env_int("BMPC_FIXED_STRIDE", 1);
    if (!fixed_stride || A->NP != (size_t)(A->N - 1)) return nullptr;
    return A->N == 20 ? bmpc_pair_launch_n20 : A->N == 30 ? bmpc_pair_launch_n30 : nullptr;
}
static std::atomic<long> fixed_launches{0};      // launches that went to a fixed-horizon kernel (the tests' proof of which kernels ran)
extern "C" long bmpc_pipe_fixed_launches(void) { return fixed_launches.load(); }
#define LAUNCH_FX(fx, kern, nb, nt, lds_doubles) \
    (fixed_launches++, fx(kern, A, nw, (unsigned)(nb), (unsigned)(nt), (lds_doubles) * sizeof(double), st))

// the evaluation launches of a super-step for nw groups of pairs: k_points || k_pose, then k_eval (|| k_curv)
static void launch_eval(const PipeArgsH* A, int nw, hipStream_t st) {
    static const int split_launches = env_int("BMPC_SPLIT_LAUNCHES", 0);
    static const int eval_split_wgs = env_int("BMPC_EVAL_SPLIT_WGS", BMPC_EVAL_SPLIT_WGS);      // (read once; 0 = never)
    const bmpc_pair_launcher fx = fixed_launcher(A);
    if (split_launches) {
        if (fx) {
            LAUNCH_FX(fx, FX_POINTS, nw, 64, pair_lds_doubles(A->N, false));
            LAUNCH_FX(fx, FX_POSE, nw, 64, pair_lds_doubles(A->N, false));
        } else {
            LAUNCH_DYN(bmpc_k_points, nw, 64, pair_lds_doubles(A->N, false));
            LAUNCH_DYN(bmpc_k_pose, nw, 64, pair_lds_doubles(A->N, false));
        }
        if (nw <= eval_split_wgs && fx) {
            LAUNCH_FX(fx, FX_EVAL_MAIN, nw, 64, pair_lds_doubles(A->N, true));
            LAUNCH_FX(fx, FX_EVAL_CHAIN, nw, 64, pair_lds_doubles(A->N, true));
        } else if (nw <= eval_split_wgs) {
            LAUNCH_DYN(bmpc_k_eval_main, nw, 64, pair_lds_doubles(A->N, true));
            LAUNCH_DYN(bmpc_k_eval_chain, nw, 64, pair_lds_doubles(A->N, true));
        } else
            LAUNCH_DYN(bmpc_k_eval, nw, 64, pair_lds_doubles(A->N, true));
        LAUNCH(bmpc_k_curv, nw, 64);
    } else if (nw > 0) {
        if (fx) LAUNCH_FX(fx, FX_POINTS_POSE, 2 * nw, 64, pair_lds_doubles(A->N, false));
        else hipLaunchKernelGGL(bmpc_k_points_pose, dim3(2 * nw), dim3(64), pair_lds_doubles(A->N, false) * sizeof(double), st, *A, nw);
        if (nw <= eval_split_wgs && fx)
            LAUNCH_FX(fx, FX_EVAL_CURV_SPLIT, A->o.hess == 2 ? 3 * nw : 2 * nw, 64, pair_lds_doubles(A->N, true));
        else if (nw <= eval_split_wgs)
            hipLaunchKernelGGL(bmpc_k_eval_curv_split, dim3(A->o.hess == 2 ? 3 * nw : 2 * nw), dim3(64), pair_lds_doubles(A->N, true) * sizeof(double), st, *A, nw);
        else
            hipLaunchKernelGGL(bmpc_k_eval_curv, dim3(A->o.hess == 2 ? 2 * nw : nw), dim3(64), pair_lds_doubles(A->N, true) * sizeof(double), st, *A, nw);
    }
}

// the factorisation and direction launches of a super-step for at most n_act active instances in nw groups of pairs: the Riccati
// kernel in the variant the number of live instances selects, k_fwd, k_step
// e0 / e1 (optional): events recorded around the Riccati launch (bmpc_debug_time_ric); *was_lat: which variant was launched
static void launch_direction(PipeArgsH* A, int n_act, int nw, hipStream_t st, hipEvent_t e0, hipEvent_t e1, int* was_lat) {
    // BMPC_RIC_LAT_BELOW in the environment (read once): A/B runs and the test that the two variants agree bitwise
    static const int lat_below = env_int("BMPC_RIC_LAT_BELOW", BMPC_RIC_LAT_BELOW);
    if (e0) (void)hipEventRecord(e0, st);
    // BMPC_RIC_SPEC_BELOW (read once; 0 = never): below it the factorisation attempts of an iteration run side by side
    static const int spec_below = env_int("BMPC_RIC_SPEC_BELOW", BMPC_RIC_SPEC_BELOW);
    if (n_act < spec_below && n_act > 0) {
        // as many attempts per instance as the chip holds at once: up to 512 workgroups with the latency compilation of the sweeps
        // (two per CU), up to 1536 with the throughput compilation (six per CU)
        const int natt = n_act * RIC_NATT <= 512 ? RIC_NATT : 1536 / n_act;
        A->natt = natt < 2 ? 2 : (natt > RIC_NATT ? RIC_NATT : natt);
        if (n_act * A->natt <= 512) LAUNCH(bmpc_k_ric_att, n_act * A->natt, BMPC_RIC_NT);
        else LAUNCH(bmpc_k_ric_att_thr, n_act * A->natt, BMPC_RIC_NT);
        LAUNCH(bmpc_k_ric_sel, n_act, BMPC_RIC_NT);
    } else if (n_act < lat_below) LAUNCH(bmpc_k_ric_lat, n_act, BMPC_RIC_NT);
    else LAUNCH(bmpc_k_ric, n_act, BMPC_RIC_NT);
    if (e1) (void)hipEventRecord(e1, st);
    if (was_lat) *was_lat = n_act < lat_below || n_act < spec_below;      // (the launches of the tail regime, whichever kernels ran)
    LAUNCH(bmpc_k_fwd, n_act, 64);
    if (const bmpc_pair_launcher fx = fixed_launcher(A)) LAUNCH_FX(fx, FX_STEP, nw, 64, pair_lds_doubles(A->N, false));
    else LAUNCH_DYN(bmpc_k_step, nw, 64, pair_lds_doubles(A->N, false));
}

// the line search of a super-step for nw groups of pairs: trial points (+ multiplier update) + filter test, backtracking inside
static void launch_trial(const PipeArgsH* A, int nw, hipStream_t st) {
    // BMPC_TRIAL_SPEC_WGS (read once; 0 = never): up to that many groups of pairs the step lengths of a line search are tried side by side (slot-major layout)
    static const int trial_spec_wgs = env_int("BMPC_TRIAL_SPEC_WGS", BMPC_TRIAL_SPEC_WGS);
    const bmpc_pair_launcher fx = fixed_launcher(A);
    if (nw <= trial_spec_wgs && A->NP == (size_t)(A->N - 1)) {
        if (fx) LAUNCH_FX(fx, FX_TRIAL_SPEC, nw, 64 * TRIAL_SPEC, trial_lds_doubles(A->N, TRIAL_SPEC));
        else LAUNCH_DYN(bmpc_k_trial_spec, nw, 64 * TRIAL_SPEC, trial_lds_doubles(A->N, TRIAL_SPEC));
    } else if (fx && BMPC_TRIAL_NW == 1)      // (the four-wavefront k_trial of an experiment build has no fixed-horizon form)
        LAUNCH_FX(fx, FX_TRIAL, nw, 64, trial_lds_doubles(A->N, 1));
    else
        LAUNCH_DYN(bmpc_k_trial, nw, 64 * BMPC_TRIAL_NW, trial_lds_doubles(A->N, BMPC_TRIAL_NW));
}

// the host's view of the double-buffered lists after bmpc_k_rotate: the *_next lists are the current ones
static void swap_lists(PipeArgsH* A) { std::swap(A->L.eval, A->L.eval_next); std::swap(A->L.trial, A->L.trial_next); }
// one super-step for at most n_act active instances; swaps the double-buffered lists in *A
extern "C" hipError_t bmpc_pipe_launch_step(PipeArgsH* A, int n_act, hipStream_t st, hipEvent_t e0, hipEvent_t e1, int* was_lat) {
    const int nw = waves_for(A->N, n_act);
    launch_eval(A, nw, st);
    launch_direction(A, n_act, nw, st, e0, e1, was_lat);
    launch_trial(A, nw, st);
    LAUNCH(bmpc_k_rotate, 1, 64);
    swap_lists(A);
    return hipGetLastError();
}

// multipliers of the solve whose final iterate is still in the workspace (A->lam_g, A->lam_x: device outputs)
extern "C" hipError_t bmpc_pipe_launch_mult(const PipeArgsH* A, hipStream_t st) {
    LAUNCH_DYN(bmpc_k_mult, waves_for(A->N, A->B), 64, pair_lds_doubles(A->N, false));
    LAUNCH(bmpc_k_mult_sweep, (A->B + 63) / 64, 64);
    return hipGetLastError();
}

// test entry bmpc_debug_superstep (bmpc_stage_matrix.hpp): kernels of their own beside the product's, which they do not touch
__global__ __launch_bounds__(64) void bmpc_k_dbg_set_rows(PipeArgsH H, const double* t, const double* z, const int* mode) {
    k_set_rows_body(DV(H), (size_t)blockIdx.x * 64 + threadIdx.x, (GCD)t, (GCD)z, (GCI)mode);
}
__global__ __launch_bounds__(64) void bmpc_k_dbg_newton_out(PipeArgsH H, double* dzeta, double* dt, double* dz, double* state) {
    k_newton_out_body(DV(H), (size_t)blockIdx.x * 64 + threadIdx.x, (GD)dzeta, (GD)dt, (GD)dz, (GD)state);
}
__global__ __launch_bounds__(BMPC_RIC_NT, 1) void bmpc_k_dbg_stage_matrices(PipeArgsH H, const double* lam_pi, double* Hout) {
    __shared__ __attribute__((aligned(16))) double lds[RIC_LDS_DOUBLES];
    k_stage_matrix_body<BMPC_RIC_NT>(ric_kernel_args(), blockIdx.x, threadIdx.x, (LDSD*)lds, (GCD)lam_pi, (GD)Hout);
}
__global__ __launch_bounds__(64) void bmpc_k_dbg_ls_plant(PipeArgsH H, const double* plant, int after_step, int nan_other) {
    k_ls_plant_body(DV(H), (size_t)blockIdx.x * 64 + threadIdx.x, (GCD)plant, after_step, nan_other);
}
__global__ __launch_bounds__(64) void bmpc_k_dbg_ls_out(PipeArgsH H, double* zeta0, double* t0, double* z0, double* zeta1, double* t1,
                                                        double* z1, double* ls) {
    k_ls_out_body(DV(H), (size_t)blockIdx.x * 64 + threadIdx.x, (GD)zeta0, (GD)t0, (GD)z0, (GD)zeta1, (GD)t1, (GD)z1, (GD)ls);
}
__global__ __launch_bounds__(64) void bmpc_k_dbg_ctl_plant(PipeArgsH H, const double* plant) {
    k_ctl_plant_body(DV(H), (size_t)blockIdx.x * 64 + threadIdx.x, (GCD)plant);
}
__global__ __launch_bounds__(64) void bmpc_k_dbg_ctl_out(PipeArgsH H, double* ctl, int after_trial) {
    k_ctl_out_body(DV(H), (size_t)blockIdx.x * 64 + threadIdx.x, (GD)ctl, after_trial);
}
// B instances in slots 0 .. B-1, just initialised (bmpc_pipe_launch_init); d: the entry's record with device pointers, which
// bmpc_debug_superstep has checked.  State planted, then the evaluation, the factorisation / direction and the trial launches of a
// super-step exactly as bmpc_pipe_launch_step issues them for B live instances, as far as the requested outputs reach -- no rotate --
// with a copy-out after each.  The line-search state (and the NaN in the copies the trial writes, when rows are given) is planted
// only when the trial runs.
extern "C" hipError_t bmpc_pipe_launch_superstep(PipeArgsH* A, const bmpc_debug_step* d, hipStream_t st) {
    const unsigned nbi = (unsigned)((A->B + 63) / 64);                                      // one thread per instance
    const unsigned nb = (unsigned)(((size_t)A->B * (A->N - 1) * NSLOT + 63) / 64);          // ... per (instance, stage, slot)
    const int nw = waves_for(A->N, A->B);
    const bool trial = d->ls != nullptr;
    if (d->t) hipLaunchKernelGGL(bmpc_k_dbg_set_rows, dim3(nb), dim3(64), 0, st, *A, d->t, d->z, d->H ? (const int*)nullptr : d->mode);
    if (trial && (d->t || d->plant0)) hipLaunchKernelGGL(bmpc_k_dbg_ls_plant, dim3(nb), dim3(64), 0, st, *A, d->plant0, 0, d->t ? 1 : 0);
    if (d->ctl_plant) hipLaunchKernelGGL(bmpc_k_dbg_ctl_plant, dim3(nbi), dim3(64), 0, st, *A, d->ctl_plant);
    launch_eval(A, nw, st);
    if (d->H) {
        hipLaunchKernelGGL(bmpc_k_dbg_stage_matrices, dim3(A->B), dim3(BMPC_RIC_NT), 0, st, *A, d->lam_pi, d->H);
        return hipGetLastError();
    }
    launch_direction(A, A->B, nw, st, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(bmpc_k_dbg_newton_out, dim3(nb), dim3(64), 0, st, *A, d->dzeta, d->dt, d->dz, d->state);
    if (d->ctl) hipLaunchKernelGGL(bmpc_k_dbg_ctl_out, dim3(nbi), dim3(64), 0, st, *A, d->ctl, 0);
    if (!trial) return hipGetLastError();
    if (d->plant1) hipLaunchKernelGGL(bmpc_k_dbg_ls_plant, dim3(nb), dim3(64), 0, st, *A, d->plant1, 1, 0);
    launch_trial(A, nw, st);
    hipLaunchKernelGGL(bmpc_k_dbg_ls_out, dim3(nb), dim3(64), 0, st, *A, d->zeta0, d->t0, d->z0, d->zeta1, d->t1, d->z1, d->ls);
    if (d->ctl) hipLaunchKernelGGL(bmpc_k_dbg_ctl_out, dim3(nbi), dim3(64), 0, st, *A, d->ctl, 1);
    return hipGetLastError();
}

extern "C" void bmpc_pipe_build_table(int* tbl) { build_scatter_table(tbl); }
extern "C" int bmpc_pipe_hrec(void) { return HREC; }
extern "C" int bmpc_pipe_krec(void) { return KREC; }
extern "C" int bmpc_pipe_npart(void) { return NPART; }
extern "C" void bmpc_pipe_ls_sizes(int* plant0, int* plant1, int* out) { *plant0 = LS_PLANT0; *plant1 = LS_PLANT1; *out = LS_OUT; }
extern "C" void bmpc_pipe_ctl_sizes(int* plant, int* out) { *plant = CTL_PLANT; *out = CTL_OUT; }
extern "C" size_t bmpc_pipe_state_bytes(void) { return sizeof(InstState); }
