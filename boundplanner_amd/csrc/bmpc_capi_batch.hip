// libboundmpc_hip.so, C ABI (include/boundmpc.h) of the batched one-launch kernels: kinematics (bmpc_fk.hip), inverse kinematics
// (bmpc_ik.hip), convex free-space sets (bmpc_sets.hip).  Every kernel has one function here that checks the arguments, takes the
// handle and launches; its entry points are that function on the caller's device pointers (the _dev entry: the caller's stream, no
// wait) or on host arrays staged through one block (bmpc_staging.hpp: the handle's stream, waited for).
#include "bmpc_platform_hip.hpp"

#define BMPC_NT 64
#include "bmpc_handle.hpp"
#include "bmpc_ik.hpp"
#include "bmpc_internal.hpp"
#include "bmpc_sets.hpp"
#include "bmpc_staging.hpp"

#include <cmath>

using namespace bmpc;

// doubles per instance of the kinematic arrays: a joint vector, a point, a rotation, the 6 collision points, a 6 x 7 Jacobian
constexpr size_t N_JOINTS = 7, N_POINT = 3, N_ROT = 9, N_COLPTS = 6 * 3, N_JAC = 6 * 7;

// Takes the handle like every other entry that uses its stream: a concurrent call on the handle returns 4, a handle that ran into its
// watchdog 5, and the wait is the watchdog's (a GPU that does not finish is an error after bmpc_opts.watchdog_ms, not a stuck thread);
// after that error the staging block is leaked like the workspace.  (Earlier versions took no guard and waited without a bound.)
extern "C" int bmpc_fk(bmpc_handle* h, int B, const double* q, const double* dq, double* ee_pos, double* ee_rot, double* col_pts,
                       double* jac, double* dvdq) {
    if (!h || B < 0 || !q) { if (h) h->err = "bmpc_fk: null argument"; return 1; }
    if (B == 0) return 0;
    WEDGED_FAIL(h);
    BUSY_OR_FAIL(h, "bmpc_fk");
    HIPCHK(h, hipSetDevice(h->o.device));
    const size_t n = (size_t)B;
    Staging s;
    s.in(&q, n * N_JOINTS); s.in(&dq, n * N_JOINTS);           // dq null: zero velocities
    s.out(&ee_pos, n * N_POINT); s.out(&ee_rot, n * N_ROT); s.out(&col_pts, n * N_COLPTS); s.out(&jac, n * N_JAC); s.out(&dvdq, n * N_JAC);
    return s.run(h, h->stream, [&]() -> int {
        HIPCHK(h, bmpc_launch_fk(B, h->d_rc, q, dq, ee_pos, ee_rot, col_pts, jac, dvdq, h->stream));
        return 0;
    });
}

// ------------------------------------------------------------------------------------------
// batched inverse kinematics (bmpc_ik.hip)
// ------------------------------------------------------------------------------------------
extern "C" void bmpc_default_ik_opts(bmpc_ik_opts* o) {
    if (!o) return;
    o->tol_cost = 1e-20; o->tol_grad = 1e-10; o->lambda0 = 1e-3; o->max_iter = 500;
}

// both entries; host: the pointers are host arrays, staged around the launch
static int ik_run(bmpc_handle* h, const char* what, bool host, int B, int n_seeds, const bmpc_ik_opts* o, const double* pd,
                  const double* rd, const double* q0, const double* lo, const double* hi, double* q, double* cost, double* pos_err,
                  double* rot_err, int* iters, int* status, int* seed, hipStream_t st) {
    if (B < 0 || !pd || !rd || !q0 || !q) { h->err = std::string(what) + ": null argument or B < 0"; return 1; }
    if (n_seeds < 1 || n_seeds > 64 || (n_seeds & (n_seeds - 1))) {
        h->err = std::string(what) + ": n_seeds must be a power of two in [1, 64]";
        return 1;
    }
    if (B > (1 << 24)) { h->err = std::string(what) + ": B > 2^24"; return 1; }
    bmpc_ik_opts d;
    bmpc_default_ik_opts(&d);
    if (o) d = *o;
    if (!(d.lambda0 > 0.0) || !std::isfinite(d.lambda0)) { h->err = std::string(what) + ": lambda0 must be positive and finite"; return 1; }
    const IkOpts io{d.tol_cost, d.tol_grad, d.lambda0, d.max_iter};
    int log2s = 0;
    while ((1 << log2s) < n_seeds) log2s++;
    if (B == 0) return 0;
    WEDGED_FAIL(h);
    BUSY_OR_FAIL(h, what);       // an asynchronous solve in flight: 4 (nothing is waited for)
    HIPCHK(h, hipSetDevice(h->o.device));
    auto launch = [&]() -> int {
        HIPCHK(h, bmpc_launch_ik(B, log2s, &io, h->d_rc, pd, rd, q0, lo, hi, q, cost, pos_err, rot_err, iters, status, seed, st));
        return 0;
    };
    if (!host) return launch();
    const size_t n = (size_t)B;
    Staging s;
    s.in(&pd, n * N_POINT); s.in(&rd, n * N_ROT); s.in(&q0, n * N_JOINTS); s.in(&lo, n * N_JOINTS); s.in(&hi, n * N_JOINTS);
    s.out(&q, n * N_JOINTS); s.out(&cost, n); s.out(&pos_err, n); s.out(&rot_err, n);
    s.out(&iters, n); s.out(&status, n); s.out(&seed, n);
    return s.run(h, st, launch);
}

extern "C" int bmpc_ik_dev(bmpc_handle* h, int B, int n_seeds, const bmpc_ik_opts* o, const double* d_pd, const double* d_rd,
                           const double* d_q0, const double* d_lo, const double* d_hi, double* d_q, double* d_cost, double* d_pos_err,
                           double* d_rot_err, int* d_iters, int* d_status, int* d_seed, void* stream) {
    if (!h) return 1;
    return ik_run(h, "bmpc_ik_dev", false, B, n_seeds, o, d_pd, d_rd, d_q0, d_lo, d_hi, d_q, d_cost, d_pos_err, d_rot_err, d_iters,
                  d_status, d_seed, (hipStream_t)stream);
}

extern "C" int bmpc_ik(bmpc_handle* h, int B, int n_seeds, const bmpc_ik_opts* o, const double* pd, const double* rd,
                       const double* q0, const double* lo, const double* hi, double* q, double* cost, double* pos_err,
                       double* rot_err, int* iters, int* status, int* seed) {
    if (!h) return 1;
    return ik_run(h, "bmpc_ik", true, B, n_seeds, o, pd, rd, q0, lo, hi, q, cost, pos_err, rot_err, iters, status, seed, h->stream);
}

// ------------------------------------------------------------------------------------------
// batched convex free-space sets (bmpc_sets.hip)
// ------------------------------------------------------------------------------------------
extern "C" void bmpc_default_sets_opts(bmpc_sets_opts* o) {
    if (!o) return;
    o->segment = 0; o->fixed_mid = 0; o->optimize = 1;
}

// both entries; host: the pointers are host arrays, staged around the launch (and the obstacle tables can be checked)
static int sets_run(bmpc_handle* h, const char* what, bool host, const bmpc_sets_opts* o, int n_obs, const double* obs_A,
                    const double* obs_b, const int* obs_nrows, const double* obs_V, const int* obs_nv, const double* e_min,
                    const double* e_max, int B, const double* p0, const double* p1, double* A, double* b, int* nrows, double* q_ellipse,
                    double* centre, int* rounds, int* newton, int* collision, int* status, hipStream_t st) {
    const bool ptrs = (n_obs == 0 || (obs_A && obs_b && obs_nrows && obs_V && obs_nv)) && e_min && e_max && p0 && (!o || !o->segment || p1) &&
                      A && b && nrows && q_ellipse && centre && status;
    if (B < 0 || !ptrs) { h->err = std::string(what) + ": null argument or B < 0"; return 1; }
    if (n_obs < 0 || n_obs > SETS_MAXOBS) { h->err = std::string(what) + ": n_obs must be in [0, 32]"; return 1; }
    if (B > (1 << 24)) { h->err = std::string(what) + ": B > 2^24"; return 1; }
    bmpc_sets_opts so;
    bmpc_default_sets_opts(&so);
    if (o) so = *o;
    for (int i = 0; host && i < n_obs; i++)
        if (obs_nrows[i] < 0 || obs_nrows[i] > SETS_OROWS || obs_nv[i] < 1 || obs_nv[i] > SETS_NV) {
            h->err = std::string(what) + ": obstacle " + std::to_string(i) + ": rows must be in [0, 15], vertices in [1, 32]";
            return 1;
        }
    if (B == 0) return 0;
    WEDGED_FAIL(h);
    BUSY_OR_FAIL(h, what);
    HIPCHK(h, hipSetDevice(h->o.device));
    if (!so.segment) p1 = nullptr;
    // the kernel reads the workspace box from its argument block (SetScene holds it by value); the _dev entry's is on the device:
    // two small copies on the caller's stream and a wait
    double box[6];
    if (host) {
        for (int a = 0; a < 3; a++) { box[a] = e_min[a]; box[3 + a] = e_max[a]; }
    } else {
        HIPCHK(h, hipMemcpyAsync(box, e_min, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipMemcpyAsync(box + 3, e_max, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
    }
    double* aat = nullptr;                // A A^T of the obstacles (segment mode)
    const size_t n_aat = so.segment ? (size_t)n_obs * SETS_OROWS * SETS_OROWS : 0;
    auto launch = [&]() -> int {
        const SetScene sc{n_obs, obs_A, obs_b, obs_nrows, obs_V, obs_nv, nullptr, {box[0], box[1], box[2]}, {box[3], box[4], box[5]}};
        HIPCHK(h, bmpc_launch_sets(B, so.segment != 0, so.fixed_mid != 0, so.optimize != 0, &sc, aat, p0, p1, A, b, nrows, q_ellipse,
                                   centre, rounds, newton, collision, status, st));
        return 0;
    };
    if (!host) {                          // stream-ordered allocation: nothing waits
        if (n_aat) HIPCHK(h, hipMallocAsync((void**)&aat, n_aat * sizeof(double), st));
        if (int r = launch()) return r;
        if (aat) HIPCHK(h, hipFreeAsync(aat, st));
        return 0;
    }
    const size_t n = (size_t)B, no = (size_t)n_obs;
    Staging s;
    s.in(&obs_A, no * SETS_OROWS * 3); s.in(&obs_b, no * SETS_OROWS); s.in(&obs_nrows, no);
    s.in(&obs_V, no * SETS_NV * 3); s.in(&obs_nv, no); s.scratch(&aat, n_aat);
    s.in(&p0, n * 3); s.in(&p1, n * 3);
    s.out(&A, n * SETS_ROWS * 3); s.out(&b, n * SETS_ROWS); s.out(&nrows, n); s.out(&q_ellipse, n * 9); s.out(&centre, n * 3);
    s.out(&rounds, n); s.out(&newton, n); s.out(&collision, n); s.out(&status, n);
    return s.run(h, st, launch);
}

extern "C" int bmpc_convex_sets_dev(bmpc_handle* h, const bmpc_sets_opts* o, int n_obs, const double* d_obs_A, const double* d_obs_b,
                                    const int* d_obs_nrows, const double* d_obs_V, const int* d_obs_nv, const double* d_e_min,
                                    const double* d_e_max, int B, const double* d_p0, const double* d_p1, double* d_A, double* d_b,
                                    int* d_nrows, double* d_q_ellipse, double* d_centre, int* d_rounds, int* d_newton, int* d_collision,
                                    int* d_status, void* stream) {
    if (!h) return 1;
    return sets_run(h, "bmpc_convex_sets_dev", false, o, n_obs, d_obs_A, d_obs_b, d_obs_nrows, d_obs_V, d_obs_nv, d_e_min, d_e_max, B, d_p0,
                    d_p1, d_A, d_b, d_nrows, d_q_ellipse, d_centre, d_rounds, d_newton, d_collision, d_status, (hipStream_t)stream);
}

extern "C" int bmpc_convex_sets(bmpc_handle* h, const bmpc_sets_opts* o, int n_obs, const double* obs_A, const double* obs_b,
                                const int* obs_nrows, const double* obs_V, const int* obs_nv, const double* e_min, const double* e_max,
                                int B, const double* p0, const double* p1, double* A, double* b, int* nrows, double* q_ellipse,
                                double* centre, int* rounds, int* newton, int* collision, int* status) {
    if (!h) return 1;
    return sets_run(h, "bmpc_convex_sets", true, o, n_obs, obs_A, obs_b, obs_nrows, obs_V, obs_nv, e_min, e_max, B, p0, p1, A, b, nrows,
                    q_ellipse, centre, rounds, newton, collision, status, h->stream);
}

// test entry (include/boundmpc.h): the parts of the set growth, one lane per item; host pointers
extern "C" int bmpc_debug_sets_parts(bmpc_handle* h, int mode, int n_obs, const double* obs_A, const double* obs_b, const int* obs_nrows,
                                     const double* obs_V, const int* obs_nv, const double* e_min, const double* e_max, int B,
                                     const double* E, const double* p, const double* rows_A, const double* rows_b, const int* rows_m,
                                     double* A, double* b, int* nrows, double* q, double* c, int* newton, int* status) {
    if (!h) return 1;
    const char* what = "bmpc_debug_sets_parts";
    const bool poly = mode == 0;
    const bool ptrs = p && A && b && nrows && q && c && newton && status &&
                      (poly ? (E && e_min && e_max && (n_obs == 0 || (obs_A && obs_b && obs_nrows && obs_V && obs_nv)))
                            : (rows_A && rows_b && rows_m));
    if (mode < 0 || mode > 2 || B < 0 || !ptrs) { h->err = std::string(what) + ": mode must be 0, 1 or 2; null argument or B < 0"; return 1; }
    if (!poly) n_obs = 0;
    if (n_obs < 0 || n_obs > SETS_MAXOBS || B > (1 << 24)) { h->err = std::string(what) + ": n_obs must be in [0, 32], B <= 2^24"; return 1; }
    for (int i = 0; i < n_obs; i++)
        if (obs_nrows[i] < 0 || obs_nrows[i] > SETS_OROWS || obs_nv[i] < 1 || obs_nv[i] > SETS_NV) {
            h->err = std::string(what) + ": obstacle " + std::to_string(i) + ": rows must be in [0, 15], vertices in [1, 32]";
            return 1;
        }
    for (int t = 0; !poly && t < B; t++)
        if (rows_m[t] < 0 || rows_m[t] > SETS_ROWS) { h->err = std::string(what) + ": rows_m must be in [0, 20]"; return 1; }
    if (B == 0) return 0;
    WEDGED_FAIL(h);
    BUSY_OR_FAIL(h, what);
    HIPCHK(h, hipSetDevice(h->o.device));
    const double lo[3] = {poly ? e_min[0] : 0.0, poly ? e_min[1] : 0.0, poly ? e_min[2] : 0.0};
    const double hi[3] = {poly ? e_max[0] : 0.0, poly ? e_max[1] : 0.0, poly ? e_max[2] : 0.0};
    if (poly) rows_A = rows_b = nullptr, rows_m = nullptr;
    else E = nullptr;
    const size_t n = (size_t)B, no = (size_t)n_obs;
    Staging s;
    s.in(&obs_A, no * SETS_OROWS * 3); s.in(&obs_b, no * SETS_OROWS); s.in(&obs_nrows, no); s.in(&obs_V, no * SETS_NV * 3); s.in(&obs_nv, no);
    s.in(&E, n * 9); s.in(&p, n * 3); s.in(&rows_A, n * SETS_ROWS * 3); s.in(&rows_b, n * SETS_ROWS); s.in(&rows_m, n);
    s.out(&A, n * SETS_ROWS * 3); s.out(&b, n * SETS_ROWS); s.out(&nrows, n); s.out(&q, n * 9); s.out(&c, n * 3); s.out(&newton, n);
    s.out(&status, n);
    return s.run(h, h->stream, [&]() -> int {
        const SetScene sc{n_obs, obs_A, obs_b, obs_nrows, obs_V, obs_nv, nullptr, {lo[0], lo[1], lo[2]}, {hi[0], hi[1], hi[2]}};
        HIPCHK(h, bmpc_launch_sets_parts(B, mode, &sc, E, p, rows_A, rows_b, rows_m, A, b, nrows, q, c, newton, status, h->stream));
        return 0;
    });
}
