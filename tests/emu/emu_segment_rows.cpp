// CPU build of the device loop's collision rows for one segment (boundplanner_amd/csrc/bmpc_freespace.hpp) -- TEST INFRASTRUCTURE
// ONLY: what bmpc_loop_k_colpairs + loop_prepare do for one collision point whose segment [p0, p1] is given directly, so that
// tests/test_segment_rows.py can hold the loop's use of separating_halfspaces against the set kernel's (emu_sets.cpp).
#include <vector>

#include "emu_platform.hpp"
#include "../../boundplanner_amd/csrc/bmpc_freespace.hpp"

using namespace bmpc;

// Obstacles in the layout of bmpc_loop_set_obstacles.  Rows 6.. of a [15][3], b [15] are written (rows 0..5 are the caller's);
// returns the row count, -1 (FS_OVERFLOW) when the rows do not fit 15 or -2 (FS_NUMERICAL) when a closest pair was not found
// (loop_prepare marks the rollout dead in both); touched as the set kernel's `collision`.
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
    return n;
}

// the closest-pair record of one obstacle {A x <= b} (nr rows, as given: the loop's packing detects an axis-aligned box and clamps,
// use_box = 0 takes the general path as the set kernel does): x(3), y(3), distance, phi
extern "C" void emu_closest_pair(int nr, const double* A, const double* b, int use_box, const double* p0, const double* p1, double* out) {
    const int nv = 0;
    double A15[45] = {0}, b15[LP_ROWS] = {0}, V[3 * LP_NV] = {0};
    for (int i = 0; i < 3 * nr; i++) A15[i] = A[i];
    for (int i = 0; i < nr; i++) b15[i] = b[i];
    std::vector<double> hd(LP_OBS_DOUBLES);
    int hi[LP_OBS_INTS];
    loop_pack_obstacles(1, A15, b15, &nr, V, &nv, hd.data(), hi);
    const LoopScene sc = loop_scene_over(1, hd.data(), hi);
    loop_closest_pair(sc.A, sc.b, sc.AAt, nr, use_box && sc.is_box[0] ? sc.box : nullptr, p0, p1, out);
}
