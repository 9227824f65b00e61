// CPU build of the device loop's collision rows for one segment (boundplanner_amd/csrc/bmpc_freespace.hpp) -- TEST INFRASTRUCTURE
// ONLY: what bmpc_loop_k_colpairs + loop_prepare do for one collision point whose segment [p0, p1] is given directly, so that
// tests/test_segment_rows.py can hold the loop's use of separating_halfspaces against the set kernel's (emu_sets.cpp).
#include <vector>

#include "emu_platform.hpp"
#include "../../boundplanner_amd/csrc/bmpc_freespace.hpp"

using namespace bmpc;

// Obstacles in the layout of bmpc_loop_set_obstacles.  Rows 6.. of a [15][3], b [15] are written (rows 0..5 are the caller's);
// returns the row count, or -1 when the rows do not fit 15 (loop_prepare marks the rollout dead there); touched as the set kernel's
// `collision`.
extern "C" int emu_loop_segment_rows(int n_obs, const double* A, const double* b, const int* nrows, const double* V, const int* nv,
                                     const double* p0, const double* p1, double* a, double* bb, int* touched) {
    std::vector<double> hd((size_t)n_obs * LP_OBS_DOUBLES + 1), res((size_t)n_obs * LP_CRES + 1, 0.0);
    std::vector<int> hi((size_t)n_obs * LP_OBS_INTS + 1);
    loop_pack_obstacles(n_obs, A, b, nrows, V, nv, hd.data(), hi.data());
    const LoopScene sc = loop_scene_over(n_obs, hd.data(), hi.data());
    for (int ob = 0; ob < n_obs; ob++)           // loop_collision_pair, without the kinematics
        loop_closest_pair(sc.A + 45 * ob, sc.b + LP_ROWS * ob, sc.AAt + LP_ROWS * LP_ROWS * ob, sc.nrows[ob],
                          sc.is_box[ob] ? sc.box + 6 * ob : nullptr, p0, p1, res.data() + LP_CRES * ob);
    const double* r = res.data();
    bool t;
    const int n = separating_halfspaces(sc, [r](int i) { return r + LP_CRES * i; }, r + 6, LP_CRES, p0, p1, LP_ROWS, a, bb, 6, t);
    *touched = t;
    return n == FS_OVERFLOW ? -1 : n;
}
