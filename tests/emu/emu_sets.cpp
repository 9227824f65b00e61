// CPU build of the batched convex-set kernel body (boundplanner_amd/csrc/bmpc_sets.hpp) -- TEST INFRASTRUCTURE ONLY.
// The identical per-lane source under the emulator's platform macros, one CPU thread per stripe of instances.  Never shipped, never
// used by the product path.
#include <algorithm>
#include <thread>
#include <vector>

#include "emu_platform.hpp"
#include "../../boundplanner_amd/csrc/bmpc_sets.hpp"

using namespace bmpc;

// Same arguments as bmpc_convex_sets (include/boundmpc.h) without the handle; p1 == NULL: point mode.  Returns 1 on misuse.
extern "C" int emu_convex_sets(int n_obs, const double* obs_A, const double* obs_b, const int* obs_nrows, const double* obs_V,
                               const int* obs_nv, const double* e_min, const double* e_max, int B, const double* p0, const double* p1,
                               int fixed_mid, int optimize, double* A, double* b, int* nrows, double* q, double* c, int* rounds,
                               int* newton, int* collision, int* status, int nthreads) {
    if (B < 0 || n_obs < 0 || n_obs > SETS_MAXOBS) return 1;
    for (int o = 0; o < n_obs; o++)
        if (obs_nrows[o] < 0 || obs_nrows[o] > SETS_OROWS || obs_nv[o] < 1 || obs_nv[o] > SETS_NV) return 1;
    std::vector<double> AAt((size_t)std::max(n_obs, 1) * SETS_OROWS * SETS_OROWS, 0.0);
    for (int o = 0; o < n_obs; o++)
        for (int i = 0; i < SETS_OROWS; i++) sets_aat_row(obs_A, obs_nrows, o, i, AAt.data());
    SetScene sc{n_obs, obs_A, obs_b, obs_nrows, obs_V, obs_nv, AAt.data(), {e_min[0], e_min[1], e_min[2]}, {e_max[0], e_max[1], e_max[2]}};
    auto one = [&](long t) {
        double dist[SETS_MAXOBS];
        double* At = A + t * SETS_ROWS * 3;
        double* bt = b + t * SETS_ROWS;
        SetResult r = p1 ? sets_segment_lane(sc, p0 + 3 * t, p1 + 3 * t, dist, 1, At, bt, q + 9 * t, c + 3 * t)
                         : sets_point_lane(sc, p0 + 3 * t, fixed_mid != 0, optimize != 0, dist, 1, At, bt, q + 9 * t, c + 3 * t);
        const int n = r.status == SETS_OK ? r.nrows : 0;
        for (int i = n; i < SETS_ROWS; i++) { At[3 * i] = At[3 * i + 1] = At[3 * i + 2] = 0.0; bt[i] = 0.0; }
        nrows[t] = n;
        if (rounds) rounds[t] = r.rounds;
        if (newton) newton[t] = r.newton;
        if (collision) collision[t] = r.collision;
        status[t] = r.status;
    };
    const int nt = std::max(1, std::min(nthreads, B));
    std::vector<std::thread> th;
    for (int k = 0; k < nt; k++)
        th.emplace_back([&, k] { for (long t = k; t < B; t += nt) one(t); });
    for (auto& t : th) t.join();
    return 0;
}

// the ellipsoid-metric projection of one obstacle (compute_set_projs for one row set): rows A [nr][3], b [nr]; E [9]; p0 [3] -> pt [3]
extern "C" int emu_sets_project(int nr, const double* A, const double* b, const double* E, const double* p0, double* pt) {
    if (nr < 0 || nr > SETS_OROWS) return 1;
    double Ap[SETS_OROWS * 3] = {0}, bp[SETS_OROWS] = {0};
    std::copy(A, A + 3 * nr, Ap);
    std::copy(b, b + nr, bp);
    const int nv = 1;
    const double V[3] = {0, 0, 0};
    SetScene sc{1, Ap, bp, &nr, V, &nv, nullptr, {0, 0, 0}, {0, 0, 0}};
    return sp_project(sc, 0, E, p0, pt) ? 0 : 2;
}

// the MVIE of m <= 20 rows: fixed_mid != 0: centre c fixed (in), else free (c: the start's seed point, out: the centre).
// q [9]; returns the set status (0 ok, 3 no interior point, 4 numerical); newton: Newton steps
extern "C" int emu_sets_mvie(int m, const double* A, const double* b, int fixed_mid, double* c, double* q, int* newton) {
    int nw = 0;
    const int st = sp_mvie(A, b, m, fixed_mid != 0, c, q, nw);
    if (newton) *newton = nw;
    return st;
}

// One round of the polyhedron growth (sp_polyhedron) around p [3] in a given metric E [9] (symmetric; Qe = E^-1 is formed as the lane
// forms it): rows A [20][3], b [20].  Returns the row count, minus the set status (-1 violates, -2 too many rows, -4 numerical), or
// -100 on misuse.
extern "C" int emu_sets_polyhedron(int n_obs, const double* obs_A, const double* obs_b, const int* obs_nrows, const double* obs_V,
                                   const int* obs_nv, const double* e_min, const double* e_max, const double* E, const double* p,
                                   double* A, double* b) {
    if (n_obs < 0 || n_obs > SETS_MAXOBS) return -100;
    for (int o = 0; o < n_obs; o++)
        if (obs_nrows[o] < 0 || obs_nrows[o] > SETS_OROWS || obs_nv[o] < 1 || obs_nv[o] > SETS_NV) return -100;
    SetScene sc{n_obs, obs_A, obs_b, obs_nrows, obs_V, obs_nv, nullptr, {e_min[0], e_min[1], e_min[2]}, {e_max[0], e_max[1], e_max[2]}};
    double dist[SETS_MAXOBS], Qe[9];
    sp_inv3(E, Qe);
    const int n = sp_polyhedron(sc, E, Qe, p, dist, 1, A, b);
    for (int i = n < 0 ? 0 : n; i < SETS_ROWS; i++) { A[3 * i] = A[3 * i + 1] = A[3 * i + 2] = 0.0; b[i] = 0.0; }
    return n;
}
