// Batched inverse kinematics (include/boundmpc.h bmpc_ik): one thread per (instance, seed), the whole projected Levenberg-Marquardt
// solve inside one launch (body: bmpc_ik.hpp).  The n_seeds lanes of an instance are adjacent and n_seeds divides the wavefront, so
// the best seed is picked with shuffles inside the wavefront.
#include "bmpc_platform_hip.hpp"

#include "bmpc_ik.hpp"
#include "bmpc_internal.hpp"

using namespace bmpc;

constexpr int IK_NT = 256;   // __launch_bounds__(IK_NT, 2): at least 2 waves per SIMD, i.e. at most 256 VGPRs (AGPRs included)

__global__ __launch_bounds__(IK_NT, 2) void bmpc_ik_kernel(int B, int log2s, IkOpts o, const RobotConst* rc, const double* pd_,
                                                        const double* rd_, const double* q0_, const double* lo_, const double* hi_,
                                                        double* q_out, double* cost_out, double* perr_out, double* rerr_out,
                                                        int* iters_out, int* status_out, int* seed_out) {
    const long t = (long)blockIdx.x * IK_NT + threadIdx.x;
    const int ns = 1 << log2s;
    if (t >= ((long)B << log2s)) return;          // whole seed groups only: a group never straddles this test
    const long b = t >> log2s;
    const int s = (int)(t & (ns - 1));
    double pd[3], rd[9], q0[7], lo[7], hi[7], q[7];
    for (int a = 0; a < 3; a++) pd[a] = pd_[b * 3 + a];
    for (int a = 0; a < 9; a++) rd[a] = rd_[b * 9 + a];
    for (int j = 0; j < 7; j++) {
        q0[j] = q0_[b * 7 + j];
        lo[j] = lo_ ? lo_[b * 7 + j] : rc->q_lo[j];
        hi[j] = hi_ ? hi_[b * 7 + j] : rc->q_hi[j];
    }
    ik_seed(s, q0, lo, hi, q);
    double cost;
    int iters, status;
    ik_solve_lane(rc, o, pd, rd, lo, hi, q, cost, iters, status);
    // best seed of the group: butterfly over the group's lanes (every lane ends with the winner's key)
    int bst = status, bs = s;
    double bf = cost;
    for (int m = 1; m < ns; m <<= 1) {
        const int ost = __shfl_xor(bst, m), os = __shfl_xor(bs, m);
        const double of = __shfl_xor(bf, m);
        if (ik_better(ost, of, os, bst, bf, bs)) { bst = ost; bf = of; bs = os; }
    }
    if (s != bs) return;
    ik_store(rc, b, s, q, cost, iters, status, pd, rd, q_out, cost_out, perr_out, rerr_out, iters_out, status_out, seed_out);
}

extern "C" hipError_t bmpc_launch_ik(int B, int log2s, const IkOpts* o, const RobotConst* rc, const double* pd, const double* rd,
                                     const double* q0, const double* lo, const double* hi, double* q, double* cost, double* pos_err,
                                     double* rot_err, int* iters, int* status, int* seed, hipStream_t st) {
    const long n = (long)B << log2s;
    hipLaunchKernelGGL(bmpc_ik_kernel, dim3((unsigned)((n + IK_NT - 1) / IK_NT)), dim3(IK_NT), 0, st, B, log2s, *o, rc, pd, rd, q0,
                       lo, hi, q, cost, pos_err, rot_err, iters, status, seed);
    return hipGetLastError();
}
