// CPU build of the path installation of the device loop (boundplanner_amd/csrc/bmpc_loop.hpp: loop_install_path) -- TEST
// INFRASTRUCTURE ONLY: what bmpc_loop_replan / bmpc_loop_init_rollouts + bmpc_loop_k_install do, rollout by rollout, from the
// identical source.  Built with the flags of emu_loop.cpp (tests/test_device_loop_replan.py).
#include "emu_platform.hpp"
#include "../../boundplanner_amd/csrc/bmpc_loop.hpp"
#include "../../boundplanner_amd/csrc/bmpc_robot.hpp"

using namespace bmpc;

// R rollouts, states S [R][state doubles] rewritten in place; the records in the layout of bmpc_loop_replan (strides of 8 via points)
extern "C" void emu_loop_install_replan(int N, int R, double* S, const int* n_pts, const double* p_via, const double* r_via, const double* bp1,
                                        const double* br1, const double* e_r_bound, const double* a_sets, const double* b_sets) {
    RobotConst rc;
    fill_robot_const(rc);
    constexpr size_t NS = LP_MAXPTS - 1;
    for (size_t r = 0; r < (size_t)R; r++)
        loop_install_path(&rc, N, S + r * LS_SIZE, LP_INSTALL_REPLAN, n_pts[r], p_via + 3 * LP_MAXPTS * r, r_via + 9 * LP_MAXPTS * r,
                          bp1 + 3 * NS * r, br1 + 3 * NS * r, e_r_bound + 6 * NS * r, a_sets + 45 * NS * r, b_sets + LP_ROWS * NS * r, nullptr,
                          nullptr);
}

// R rollouts at rest at q0 [R][7] with weights [11], as bmpc_loop_init_rollouts
extern "C" void emu_loop_install_fresh(int N, int R, double* S, const double* q0, const double* weights) {
    RobotConst rc;
    fill_robot_const(rc);
    for (size_t r = 0; r < (size_t)R; r++)
        loop_install_path(&rc, N, S + r * LS_SIZE, LP_INSTALL_FRESH, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, q0 + 7 * r,
                          weights);
}
