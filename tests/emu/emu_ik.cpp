// CPU build of the batched inverse-kinematics kernel body (boundplanner_amd/csrc/bmpc_ik.hpp) -- TEST INFRASTRUCTURE ONLY.
// The identical per-lane source under the emulator's platform macros; the best seed of an instance is picked with a serial loop
// under the same total order (ik_better) as the wavefront shuffles of bmpc_ik.hip.  Never shipped, never used by the product path.
#include <algorithm>
#include <thread>
#include <vector>

#include "emu_platform.hpp"
#include "../../boundplanner_amd/csrc/bmpc_ik.hpp"
#include "../../boundplanner_amd/csrc/bmpc_robot.hpp"

using namespace bmpc;

// same arguments as bmpc_ik (include/boundmpc.h) plus the robot table (NULL: iiwa14); opts4 = {tol_cost, tol_grad, lambda0, max_iter}
extern "C" int emu_ik_solve(const bmpc_robot* robot, int B, int n_seeds, const double* opts4, const double* pd, const double* rd,
                            const double* q0, const double* lo, const double* hi, double* q, double* cost, double* pos_err,
                            double* rot_err, int* iters, int* status, int* seed, int nthreads) {
    if (B < 0 || n_seeds < 1 || n_seeds > 64 || (n_seeds & (n_seeds - 1))) return 1;
    bmpc_robot r;
    if (robot) r = *robot; else robot_iiwa14(r);
    RobotConst rc;
    fill_robot_const(rc, r);
    const IkOpts o{opts4[0], opts4[1], opts4[2], (int)opts4[3]};
    auto one = [&](long b) {
        double lb[7], hb[7];
        for (int j = 0; j < 7; j++) { lb[j] = lo ? lo[b * 7 + j] : rc.q_lo[j]; hb[j] = hi ? hi[b * 7 + j] : rc.q_hi[j]; }
        double bq[7], bf = 0.0;
        int bit = 0, bst = 0, bs = -1;
        for (int s = 0; s < n_seeds; s++) {
            double qs[7], f;
            int it, st;
            ik_seed(s, q0 + b * 7, lb, hb, qs);
            ik_solve_lane(&rc, o, pd + b * 3, rd + b * 9, lb, hb, qs, f, it, st);
            if (bs < 0 || ik_better(st, f, s, bst, bf, bs)) {
                std::copy(qs, qs + 7, bq);
                bf = f; bit = it; bst = st; bs = s;
            }
        }
        ik_store(&rc, b, bs, bq, bf, bit, bst, pd + b * 3, rd + b * 9, q, cost, pos_err, rot_err, iters, status, seed);
    };
    const int nt = std::max(1, std::min(nthreads, B));
    std::vector<std::thread> th;
    for (int k = 0; k < nt; k++)
        th.emplace_back([&, k] { for (long b = k; b < B; b += nt) one(b); });
    for (auto& t : th) t.join();
    return 0;
}

// the model of one configuration: J(q), the half gradient gh [7] and the Gauss-Newton matrix H [28] (packed lower) of ik_eval
extern "C" double emu_ik_model(const bmpc_robot* robot, const double* q, const double* pd, const double* rd, double* gh, double* H) {
    bmpc_robot r;
    if (robot) r = *robot; else robot_iiwa14(r);
    RobotConst rc;
    fill_robot_const(rc, r);
    return ik_eval<true>(&rc, q, pd, rd, H, gh);
}
