// Batched convex free-space sets (include/boundmpc.h bmpc_convex_sets): one thread per seed (point mode) or segment (segment mode),
// the whole set growth inside one launch (body: bmpc_sets.hpp).  Lanes never exchange data, so a result does not depend on the batch
// size or on the instance's position.  Storage: obstacle rows and vertices in global memory, read alike by
// every lane; the set's rows in the lane's output rows; the per-obstacle distances of a round in LDS, [obstacle][lane].
#include "bmpc_platform_hip.hpp"

#define BMPC_NT 64
#include "bmpc_internal.hpp"
#include "bmpc_sets.hpp"

using namespace bmpc;

constexpr int SETS_NT = 64;   // one wavefront per workgroup: 64 x 32 doubles of LDS (16 KiB)

// A A^T of every obstacle (the segment mode's projections): one thread per (obstacle, row i).  On the device because bmpc_convex_sets_dev
// hands in device pointers; why this is not the loop's host-side A A^T: bmpc_freespace.hpp
__global__ void bmpc_sets_aat_kernel(int n_obs, const double* A, const int* nrows, double* AAt) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_obs * SETS_OROWS) return;
    sets_aat_row(A, nrows, t / SETS_OROWS, t % SETS_OROWS, AAt);
}

__global__ __launch_bounds__(SETS_NT) void bmpc_sets_kernel(int B, int segment, int fixed_mid, int optimize, SetScene sc,
                                                            const double* p0_, const double* p1_, double* A_out, double* b_out,
                                                            int* nrows_out, double* q_out, double* c_out, int* rounds_out,
                                                            int* newton_out, int* collision_out, int* status_out) {
    __shared__ double sdist[SETS_MAXOBS * SETS_NT];
    const long t = (long)blockIdx.x * SETS_NT + threadIdx.x;
    if (t >= B) return;
    double* A = A_out + t * SETS_ROWS * 3;
    double* b = b_out + t * SETS_ROWS;
    const double p0[3] = {p0_[3 * t], p0_[3 * t + 1], p0_[3 * t + 2]};
    double qe[9], c[3];
    SetResult r;
    if (segment) {
        const double p1[3] = {p1_[3 * t], p1_[3 * t + 1], p1_[3 * t + 2]};
        r = sets_segment_lane(sc, p0, p1, sdist + threadIdx.x, SETS_NT, A, b, qe, c);
    } else {
        r = sets_point_lane(sc, p0, fixed_mid != 0, optimize != 0, sdist + threadIdx.x, SETS_NT, A, b, qe, c);
    }
    // rows past the set's (and all rows of a failed instance past what was written) are zero
    const int n = r.status == SETS_OK ? r.nrows : 0;
    for (int i = n; i < SETS_ROWS; i++) {
        A[3 * i] = 0.0; A[3 * i + 1] = 0.0; A[3 * i + 2] = 0.0;
        b[i] = 0.0;
    }
    for (int k = 0; k < 9; k++) q_out[9 * t + k] = qe[k];
    for (int k = 0; k < 3; k++) c_out[3 * t + k] = c[k];
    nrows_out[t] = n;
    if (rounds_out) rounds_out[t] = r.rounds;
    if (newton_out) newton_out[t] = r.newton;
    if (collision_out) collision_out[t] = r.collision;
    status_out[t] = r.status;
}

extern "C" hipError_t bmpc_launch_sets(int B, int segment, int fixed_mid, int optimize, const SetScene* sc, double* AAt_ws,
                                       const double* p0, const double* p1, double* A, double* b, int* nrows, double* q, double* c,
                                       int* rounds, int* newton, int* collision, int* status, hipStream_t st) {
    SetScene s = *sc;
    if (segment && s.obs.n_obs > 0) {
        const int n = s.obs.n_obs * SETS_OROWS;
        hipLaunchKernelGGL(bmpc_sets_aat_kernel, dim3((n + 63) / 64), dim3(64), 0, st, s.obs.n_obs, s.obs.A, s.obs.nrows, AAt_ws);
        s.obs.AAt = AAt_ws;
    }
    hipLaunchKernelGGL(bmpc_sets_kernel, dim3((unsigned)((B + SETS_NT - 1) / SETS_NT)), dim3(SETS_NT), 0, st, B, segment, fixed_mid,
                       optimize, s, p0, p1, A, b, nrows, q, c, rounds, newton, collision, status);
    return hipGetLastError();
}

// Test entry bmpc_debug_sets_parts (include/boundmpc.h): one lane per item runs ONE part of the set growth, the same inlined functions
// as bmpc_sets_kernel -- mode 0: sp_polyhedron around p in the given metric E (nrows: the row count, or minus the status);
// mode 1 / 2: sp_mvie with a fixed / free centre on given rows (copied into the lane's output rows first: that is where the product
// keeps the rows it inscribes in).
__global__ __launch_bounds__(SETS_NT) void bmpc_sets_parts_kernel(int B, int mode, SetScene sc, const double* E_, const double* p_,
                                                                  const double* A_in, const double* b_in, const int* m_in,
                                                                  double* A_out, double* b_out, int* nrows_out, double* q_out,
                                                                  double* c_out, int* newton_out, int* status_out) {
    __shared__ double sdist[SETS_MAXOBS * SETS_NT];
    const long t = (long)blockIdx.x * SETS_NT + threadIdx.x;
    if (t >= B) return;
    double* A = A_out + t * SETS_ROWS * 3;
    double* b = b_out + t * SETS_ROWS;
    double c[3] = {p_[3 * t], p_[3 * t + 1], p_[3 * t + 2]};
    double q[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int n = 0, newton = 0, status = SETS_OK;
    if (mode == 0) {
        double E[9], Qe[9];
        for (int k = 0; k < 9; k++) E[k] = E_[9 * t + k];
        sp_inv3(E, Qe);
        n = sp_polyhedron(sc, E, Qe, c, sdist + threadIdx.x, SETS_NT, A, b);
        if (n < 0) status = -n;
        for (int k = 0; k < 9; k++) q[k] = Qe[k];
    } else {
        n = min(max(m_in[t], 0), SETS_ROWS);
        for (int i = 0; i < 3 * n; i++) A[i] = A_in[t * SETS_ROWS * 3 + i];
        for (int i = 0; i < n; i++) b[i] = b_in[t * SETS_ROWS + i];
        status = sp_mvie(A, b, n, mode == 1, c, q, newton);
    }
    for (int i = max(n, 0); i < SETS_ROWS; i++) {
        A[3 * i] = 0.0; A[3 * i + 1] = 0.0; A[3 * i + 2] = 0.0;
        b[i] = 0.0;
    }
    for (int k = 0; k < 9; k++) q_out[9 * t + k] = q[k];
    for (int k = 0; k < 3; k++) c_out[3 * t + k] = c[k];
    nrows_out[t] = n;
    newton_out[t] = newton;
    status_out[t] = status;
}

extern "C" hipError_t bmpc_launch_sets_parts(int B, int mode, const SetScene* sc, const double* E, const double* p, const double* A_in,
                                             const double* b_in, const int* m_in, double* A, double* b, int* nrows, double* q, double* c,
                                             int* newton, int* status, hipStream_t st) {
    hipLaunchKernelGGL(bmpc_sets_parts_kernel, dim3((unsigned)((B + SETS_NT - 1) / SETS_NT)), dim3(SETS_NT), 0, st, B, mode, *sc, E, p,
                       A_in, b_in, m_in, A, b, nrows, q, c, newton, status);
    return hipGetLastError();
}
