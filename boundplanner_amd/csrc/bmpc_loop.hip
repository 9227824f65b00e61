// Device-resident closed loop (include/boundmpc.h, bmpc_loop_*): kernels around the batched solve for
// gfx950.  Per-rollout logic: bmpc_loop.hpp (one thread per rollout -- it is sequential, data-dependent
// bookkeeping on 3-vectors, a few microseconds per step); bulk row traffic (start vector, bound rows,
// warm-start copy) goes through element-wise kernels so that every HBM access is coalesced.
#include "bmpc_platform_hip.hpp"

#define BMPC_NT 64
#include "bmpc_loop.hpp"
#include "bmpc_robot.hpp"

#include <chrono>
#include <climits>
#include <string>
#include <vector>

#include "../../include/boundmpc.h"
#include "bmpc_internal.hpp"

using namespace bmpc;

__global__ __launch_bounds__(256) void bmpc_loop_k_bounds(int R, int N, const RobotConst* rc, double* lbx, double* ubx) {
    const int n_w = 44 * N + 6;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)R * n_w) return;
    loop_bound_const(rc, N, (int)(e % n_w), lbx + e, ubx + e);
}

// Every kernel below runs either over all R rollouts (list == nullptr) or over the rollouts of a device list of length
// *n_list (bmpc_loop_run_async: the rollouts whose solve has just retired).
#define LOOP_ROLLOUT(e, r)                                  \
    int r = (e);                                            \
    if (list) { if ((e) >= *n_list) return; r = list[e]; }  \
    else if ((e) >= R) return;

// closest pairs collision-point segment <-> obstacle of the shared scene (bmpc_loop_set_obstacles): one thread per (rollout, collision
// point), blockIdx.y = obstacle, so that the obstacle's rows are wave-uniform (scalar loads)
__global__ __launch_bounds__(64) void bmpc_loop_k_colpairs(int R, const RobotConst* rc, LoopScene sc, const double* S, double* colres,
                                                           const int* list, const int* n_list) {
    const int e6 = blockIdx.x * 64 + threadIdx.x, ob = blockIdx.y;
    const int e = e6 / 6, pt = e6 - 6 * e;
    LOOP_ROLLOUT(e, r)
    const double* s = S + (size_t)r * LS_SIZE;
    if (s[LS_dead] != 0.0) return;
    loop_collision_pair(rc, sc, s, pt, ob, colres + (((size_t)r * 6 + pt) * sc.n_obs + ob) * LP_CRES);
}

// the prepare phase of rollout r in the scene sc, res: the closest-pair results of the rollout (both prepare kernels)
static __device__ __forceinline__ void prepare_rollout(int r, int N, const RobotConst* rc, double* S, const double* prev, double* p,
                                                       double* lbx, double* ubx, const LoopScene& sc, const double* res) {
    const size_t n_w = 44 * N + 6;
    double* s = S + (size_t)r * LS_SIZE;
    if (s[LS_dead] != 0.0) return;
    loop_prepare(rc, N, s, prev + r * n_w, p + (size_t)r * NPAR, lbx + r * n_w, ubx + r * n_w, &sc, res);
}

__global__ __launch_bounds__(64) void bmpc_loop_k_prepare(int R, int N, const RobotConst* rc, double* S, const double* prev,
                                                          double* p, double* lbx, double* ubx, LoopScene sc, const double* colres,
                                                          const int* list, const int* n_list) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    LOOP_ROLLOUT(e, r)
    prepare_rollout(r, N, rc, S, prev, p, lbx, ubx, sc, colres ? colres + (size_t)r * 6 * sc.n_obs * LP_CRES : nullptr);
}

// The same two kernels with one scene per rollout (bmpc_loop_set_scenes).  The rollouts of a wavefront look at different scenes -- and
// bmpc_loop_run_async hands over an arbitrary list of rollouts -- so nothing about the obstacle is wave-uniform here: every lane
// resolves (rollout, collision point, obstacle slot = blockIdx.y) -> scene -> obstacle itself and reads the obstacle's rows with its
// own (vector) loads; a lane whose scene has no obstacle in this slot has nothing to do.  The arithmetic is the shared source
// (loop_collision_pair, loop_prepare), so an obstacle gives bitwise the numbers it gives through bmpc_loop_k_colpairs.
__global__ __launch_bounds__(64) void bmpc_loop_k_colpairs_scenes(int R, const RobotConst* rc, LoopSceneTable tab, const double* S,
                                                                  double* colres, const int* list, const int* n_list) {
    const int e6 = blockIdx.x * 64 + threadIdx.x, ob = blockIdx.y;
    const int e = e6 / 6, pt = e6 - 6 * e;
    LOOP_ROLLOUT(e, r)
    const LoopScene sc = loop_scene_of(tab, r);
    if (ob >= sc.n_obs) return;
    const double* s = S + (size_t)r * LS_SIZE;
    if (s[LS_dead] != 0.0) return;
    loop_collision_pair(rc, sc, s, pt, ob, colres + loop_colres_of(tab, r) + (size_t)(pt * sc.n_obs + ob) * LP_CRES);
}

__global__ __launch_bounds__(64) void bmpc_loop_k_prepare_scenes(int R, int N, const RobotConst* rc, double* S, const double* prev,
                                                                 double* p, double* lbx, double* ubx, LoopSceneTable tab,
                                                                 const double* colres, const int* list, const int* n_list) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    LOOP_ROLLOUT(e, r)
    prepare_rollout(r, N, rc, S, prev, p, lbx, ubx, loop_scene_of(tab, r), colres + loop_colres_of(tab, r));
}

__global__ __launch_bounds__(256) void bmpc_loop_k_x0(int R, int N, const double* S, const double* prev, double* x0,
                                                      const int* list, const int* n_list) {
    const int n_w = 44 * N + 6;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int e = (int)(idx / n_w), i = (int)(idx - (size_t)e * n_w);
    LOOP_ROLLOUT(e, r)
    x0[(size_t)r * n_w + i] = loop_x0_elem(N, S + (size_t)r * LS_SIZE, prev + (size_t)r * n_w, i);
}

// steps_left (bmpc_loop_run_async): per-rollout countdown; the log row of a rollout's step is (steps taken so far) * R + r,
// cont[r] tells the solver whether the rollout has another problem coming
__global__ __launch_bounds__(64) void bmpc_loop_k_finish(int R, int N, double dt, const RobotConst* rc, double* S, const double* x,
                                                         const double* prev, const int* status, const double* viol,
                                                         const int* iters, double* log, const int* list, const int* n_list,
                                                         int* steps_left, int* cont, int nsteps, const double* par, double* rec,
                                                         const int* rec_slot) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    LOOP_ROLLOUT(e, r)
    const size_t n_w = 44 * N + 6;
    double* s = S + (size_t)r * LS_SIZE;
    double* lg = log ? log + (size_t)r * LP_LOGW : nullptr;
    if (steps_left) {
        const int left = steps_left[r];
        if (log) lg = log + ((size_t)(nsteps - left) * R + r) * LP_LOGW;
        steps_left[r] = left - 1;
        cont[r] = left - 1 > 0;
    }
    if (s[LS_dead] != 0.0) {
        s[LS_accept] = 0.0;
        if (lg) { for (int i = 0; i < LP_LOGW; i++) lg[i] = 0.0; lg[4] = 1.0; }
        return;
    }
    double* rc_ = (rec && rec_slot[r] >= 0) ? rec + (size_t)rec_slot[r] * lp_rec_doubles(N) : nullptr;
    loop_finish(rc, N, dt, s, x + r * n_w, prev + r * n_w, status[r], viol[r], iters[r], lg, rc_, par + (size_t)r * NPAR);
}

// prev_solution <- accepted solution (BoundMPC.py:643)
__global__ __launch_bounds__(256) void bmpc_loop_k_keep(int R, int N, const double* S, const double* x, double* prev,
                                                        const int* list, const int* n_list) {
    const int n_w = 44 * N + 6;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int e = (int)(idx / n_w), i = (int)(idx - (size_t)e * n_w);
    LOOP_ROLLOUT(e, r)
    const size_t o = (size_t)r * n_w + i;
    if (S[(size_t)r * LS_SIZE + LS_accept] != 0.0) prev[o] = x[o];
}

// a reference path for `count` rollouts, one per thread (loop_install_path): the rollouts of a device list with one staged path
// record each (bmpc_loop_replan), or rollouts first .. first + count - 1 put at rest at q0 on their trivial start-up path
// (bmpc_loop_init_rollouts: list == nullptr).  Records have the fixed strides of LP_MAXPTS via points.
__global__ __launch_bounds__(64) void bmpc_loop_k_install(int count, int N, const RobotConst* rc, double* S, int mode, const int* list,
                                                          int first, const int* n_pts, const double* p_via, const double* r_via,
                                                          const double* bp1, const double* br1, const double* e_r_bound,
                                                          const double* a_sets, const double* b_sets, const double* q0,
                                                          const double* weights) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= count) return;
    double* s = S + (size_t)(list ? list[e] : first + e) * LS_SIZE;
    constexpr int NS = LP_MAXPTS - 1;
    const size_t i = (size_t)e;
    if (mode == LP_INSTALL_FRESH)
        loop_install_path(rc, N, s, mode, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, q0 + 7 * i, weights);
    else
        loop_install_path(rc, N, s, mode, n_pts[e], p_via + 3 * LP_MAXPTS * i, r_via + 9 * LP_MAXPTS * i, bp1 + 3 * NS * i, br1 + 3 * NS * i,
                          e_r_bound + 6 * NS * i, a_sets + 45 * NS * i, b_sets + LP_ROWS * NS * i, nullptr, nullptr);
}

struct bmpc_loop {
    bmpc_handle* h = nullptr;
    int R = 0, N = 0, n_w = 0, dev = 0;
    double dt = 0.1;
    RobotConst* d_rc = nullptr;
    double *d_S = nullptr, *d_prev = nullptr, *d_x0 = nullptr, *d_lbx = nullptr, *d_ubx = nullptr, *d_p = nullptr,
           *d_x = nullptr, *d_f = nullptr, *d_viol = nullptr, *d_log = nullptr;
    int *d_iters = nullptr, *d_status = nullptr;
    LoopScene sc{0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // device pointers
    double* d_scene = nullptr;     // A | b | AAt | V
    int* d_scene_i = nullptr;      // nrows | nv
    double* d_colres = nullptr;
    LoopSceneTable tab{};          // bmpc_loop_set_scenes: one scene per rollout (n_scenes > 0); its obstacles live in d_scene / d_scene_i too
    int *d_first = nullptr, *d_rollout_scene = nullptr;
    int *d_steps_left = nullptr, *d_cont = nullptr;    // bmpc_loop_run_async
    int* d_rec_slot = nullptr;     // [R] index of the rollout's record in a step's block, or -1 (bmpc_loop_set_record)
    int n_rec = 0;
    double* d_rec = nullptr;       // [steps][n_rec][lp_rec_doubles(N)] of the last bmpc_loop_run
    size_t rec_cap = 0, rec_steps = 0;
    int async_nsteps = 0;
    void* d_inst = nullptr;        // staged arguments of bmpc_loop_replan / bmpc_loop_init_rollouts (grows, never shrinks)
    size_t inst_cap = 0;
    float inst_ms = 0.f;           // the last install kernel by the events e0 / e1
    double* async_log = nullptr;
    size_t log_cap = 0;
    hipStream_t st = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::string err;
};

#define LCHK(L, call)                                                            \
    do {                                                                         \
        hipError_t e_ = (call);                                                  \
        if (e_ != hipSuccess) {                                                  \
            (L)->err = std::string(#call) + ": " + hipGetErrorString(e_);        \
            return 2;                                                            \
        }                                                                        \
    } while (0)

extern "C" int bmpc_loop_state_doubles(void) { return LS_SIZE; }
extern "C" int bmpc_loop_log_doubles(void) { return LP_LOGW; }
extern "C" int bmpc_loop_record_doubles(int N) { return lp_rec_doubles(N); }

// MPCData records (include/boundmpc.h): the rollouts whose steps bmpc_loop_run records from now on (n = 0: none)
extern "C" int bmpc_loop_set_record(bmpc_loop* L, int n, const int* rollouts) {
    if (!L || n < 0 || (n > 0 && !rollouts)) return 1;
    LCHK(L, hipSetDevice(L->dev));
    std::vector<int> slot((size_t)L->R, -1);
    for (int j = 0; j < n; j++) {
        if (rollouts[j] < 0 || rollouts[j] >= L->R) { L->err = "bmpc_loop_set_record: rollout index out of range"; return 1; }
        if (slot[(size_t)rollouts[j]] >= 0) { L->err = "bmpc_loop_set_record: a rollout is listed twice"; return 1; }
        slot[(size_t)rollouts[j]] = j;
    }
    if (!L->d_rec_slot) LCHK(L, hipMalloc((void**)&L->d_rec_slot, (size_t)L->R * sizeof(int)));
    LCHK(L, hipStreamSynchronize(L->st));
    LCHK(L, hipMemcpy(L->d_rec_slot, slot.data(), slot.size() * sizeof(int), hipMemcpyHostToDevice));
    L->n_rec = n; L->rec_steps = 0;
    return 0;
}
// the records of the last bmpc_loop_run: out [steps][n][bmpc_loop_record_doubles(N)], room for max_steps steps (out == NULL: only
// *steps is returned, to size the buffer); more recorded steps than room: rc 1, nothing copied
extern "C" int bmpc_loop_records(bmpc_loop* L, double* out, int max_steps, int* steps) {
    if (!L || (!out && !steps)) return 1;
    LCHK(L, hipSetDevice(L->dev));
    LCHK(L, hipStreamSynchronize(L->st));
    if (steps) *steps = (int)L->rec_steps;
    if (!out) return 0;
    if (L->rec_steps > (size_t)(max_steps < 0 ? 0 : max_steps)) { L->err = "bmpc_loop_records: more recorded steps than the buffer holds"; return 1; }
    if (L->rec_steps > 0)
        LCHK(L, hipMemcpy(out, L->d_rec, L->rec_steps * L->n_rec * lp_rec_doubles(L->N) * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int bmpc_loop_field(const char* name, int* offset, int* count) { return loop_field_lookup(name, offset, count); }
extern "C" const char* bmpc_loop_last_error(const bmpc_loop* L) { return L ? L->err.c_str() : "null loop"; }

extern "C" void bmpc_loop_destroy(bmpc_loop* L) {
    if (!L) return;
    if (L->st) { (void)hipSetDevice(L->dev); (void)hipStreamSynchronize(L->st); }     // nothing of the loop still in flight
    double* bufs[] = {L->d_S, L->d_prev, L->d_x0, L->d_lbx, L->d_ubx, L->d_p, L->d_x, L->d_f, L->d_viol, L->d_log};
    for (double* b : bufs) if (b) (void)hipFree(b);
    if (L->d_rec) (void)hipFree(L->d_rec);
    if (L->d_rec_slot) (void)hipFree(L->d_rec_slot);
    if (L->d_iters) (void)hipFree(L->d_iters);
    if (L->d_status) (void)hipFree(L->d_status);
    if (L->d_rc) (void)hipFree(L->d_rc);
    if (L->d_scene) (void)hipFree(L->d_scene);
    if (L->d_scene_i) (void)hipFree(L->d_scene_i);
    if (L->d_colres) (void)hipFree(L->d_colres);
    if (L->d_first) (void)hipFree(L->d_first);
    if (L->d_rollout_scene) (void)hipFree(L->d_rollout_scene);
    if (L->d_steps_left) (void)hipFree(L->d_steps_left);
    if (L->d_cont) (void)hipFree(L->d_cont);
    if (L->d_inst) (void)hipFree(L->d_inst);
    if (L->e0) (void)hipEventDestroy(L->e0);
    if (L->e1) (void)hipEventDestroy(L->e1);
    if (L->h) bmpc_handle_release(L->h);     // a bmpc_destroy deferred because of this loop runs now
    delete L;
}

extern "C" int bmpc_loop_create(bmpc_handle* h, int R, bmpc_loop** out) {
    if (!h || !out || R <= 0) return 1;
    bmpc_loop* L = new bmpc_loop();
    *out = L;
    L->R = R;
    bmpc_opts o;
    if (bmpc_get_opts(h, &o) != 0) { L->err = "bmpc_get_opts failed"; return 1; }
    if (o.N > LP_NMAX) { L->err = "horizon too long for the device loop"; return 1; }
    L->N = o.N; L->dt = o.dt; L->n_w = 44 * o.N + 6;
    L->dev = o.device;
    LCHK(L, hipSetDevice(o.device));
    RobotConst rc;
    bmpc_robot rob;
    if (bmpc_get_robot(h, &rob) != 0) { L->err = "bmpc_get_robot failed"; return 1; }
    fill_robot_const(rc, rob);                 // the loop works on the robot the handle has at this moment
    LCHK(L, hipMalloc((void**)&L->d_rc, sizeof(RobotConst)));
    LCHK(L, hipMemcpy(L->d_rc, &rc, sizeof(RobotConst), hipMemcpyHostToDevice));
    const size_t nw = (size_t)R * L->n_w * sizeof(double);
    LCHK(L, hipMalloc((void**)&L->d_S, (size_t)R * LS_SIZE * sizeof(double)));
    LCHK(L, hipMemset(L->d_S, 0, (size_t)R * LS_SIZE * sizeof(double)));
    double** rows[] = {&L->d_prev, &L->d_x0, &L->d_lbx, &L->d_ubx, &L->d_x};
    for (double** b : rows) { LCHK(L, hipMalloc((void**)b, nw)); LCHK(L, hipMemset(*b, 0, nw)); }
    LCHK(L, hipMalloc((void**)&L->d_p, (size_t)R * NPAR * sizeof(double)));
    LCHK(L, hipMalloc((void**)&L->d_f, (size_t)R * sizeof(double)));
    LCHK(L, hipMalloc((void**)&L->d_viol, (size_t)R * sizeof(double)));
    LCHK(L, hipMalloc((void**)&L->d_iters, (size_t)R * sizeof(int)));
    LCHK(L, hipMalloc((void**)&L->d_status, (size_t)R * sizeof(int)));
    LCHK(L, hipMemset(L->d_viol, 0, (size_t)R * sizeof(double)));
    LCHK(L, hipMemset(L->d_iters, 0, (size_t)R * sizeof(int)));
    LCHK(L, hipMemset(L->d_status, 0, (size_t)R * sizeof(int)));
    L->h = h;
    bmpc_handle_retain(h);                    // the handle outlives the loop even if the caller destroys it first
    L->st = (hipStream_t)bmpc_stream(h);      // the handle's stream: one stream (one hardware queue) per solver handle
    LCHK(L, hipEventCreate(&L->e0));
    LCHK(L, hipEventCreate(&L->e1));
    const size_t ne = (size_t)R * L->n_w;
    hipLaunchKernelGGL(bmpc_loop_k_bounds, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, L->st, R, L->N, L->d_rc, L->d_lbx, L->d_ubx);
    LCHK(L, hipGetLastError());
    LCHK(L, hipStreamSynchronize(L->st));
    return 0;
}

static bool range_ok(bmpc_loop* L, int first, int count) {
    if (!L || first < 0 || count <= 0 || first + count > L->R) { if (L) L->err = "rollout range out of bounds"; return false; }
    return true;
}

extern "C" int bmpc_loop_upload(bmpc_loop* L, int first, int count, const double* state, const double* prev) {
    if (!range_ok(L, first, count) || !state) return 1;
    LCHK(L, hipSetDevice(L->dev));      // the calling host thread may be new
    LCHK(L, hipMemcpy(L->d_S + (size_t)first * LS_SIZE, state, (size_t)count * LS_SIZE * sizeof(double), hipMemcpyHostToDevice));
    if (prev) LCHK(L, hipMemcpy(L->d_prev + (size_t)first * L->n_w, prev, (size_t)count * L->n_w * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int bmpc_loop_download(bmpc_loop* L, int first, int count, double* state, double* prev) {
    if (!range_ok(L, first, count)) return 1;
    LCHK(L, hipSetDevice(L->dev));      // the calling host thread may be new
    LCHK(L, hipStreamSynchronize(L->st));
    if (state) LCHK(L, hipMemcpy(state, L->d_S + (size_t)first * LS_SIZE, (size_t)count * LS_SIZE * sizeof(double), hipMemcpyDeviceToHost));
    if (prev) LCHK(L, hipMemcpy(prev, L->d_prev + (size_t)first * L->n_w, (size_t)count * L->n_w * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// forget the installed obstacles, shared scene or table (the loop's stream is idle)
static void drop_obstacles(bmpc_loop* L) {
    void* bufs[] = {L->d_scene, L->d_scene_i, L->d_colres, L->d_first, L->d_rollout_scene};
    for (void* b : bufs) if (b) (void)hipFree(b);
    L->d_scene = nullptr; L->d_scene_i = nullptr; L->d_colres = nullptr; L->d_first = nullptr; L->d_rollout_scene = nullptr;
    L->sc = LoopScene{0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    L->tab = LoopSceneTable{};
}

static bool obstacles_ok(bmpc_loop* L, size_t n, const int* nrows, const int* nv) {
    for (size_t i = 0; i < n; i++)
        if (nrows[i] < 1 || nrows[i] > LP_ROWS || nv[i] < 1 || nv[i] > LP_NV) { L->err = "obstacle with too many rows or vertices"; return false; }
    return true;
}

// n > 0 obstacles (one scene, or all scenes of a table back to back) -> d_scene / d_scene_i, the closest-pair results for `stride`
// obstacles per rollout -> d_colres; `all`: the LoopScene over the n obstacles
static int install_obstacles(bmpc_loop* L, size_t n, const double* A, const double* b, const int* nrows, const double* V, const int* nv,
                             int stride, LoopScene* all) {
    std::vector<double> h(n * LP_OBS_DOUBLES);
    std::vector<int> hi(n * LP_OBS_INTS);
    loop_pack_obstacles(n, A, b, nrows, V, nv, h.data(), hi.data());
    LCHK(L, hipMalloc((void**)&L->d_scene, h.size() * sizeof(double)));
    LCHK(L, hipMemcpy(L->d_scene, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    LCHK(L, hipMalloc((void**)&L->d_scene_i, hi.size() * sizeof(int)));
    LCHK(L, hipMemcpy(L->d_scene_i, hi.data(), hi.size() * sizeof(int), hipMemcpyHostToDevice));
    LCHK(L, hipMalloc((void**)&L->d_colres, (size_t)L->R * 6 * stride * LP_CRES * sizeof(double)));
    LCHK(L, hipMemset(L->d_colres, 0, (size_t)L->R * 6 * stride * LP_CRES * sizeof(double)));
    *all = loop_scene_over(n, L->d_scene, L->d_scene_i);
    return 0;
}

extern "C" int bmpc_loop_set_obstacles(bmpc_loop* L, int n_obs, const double* A, const double* b, const int* nrows, const double* V,
                                       const int* nv) {
    if (!L || n_obs < 0 || n_obs > LP_MAXOBS || (n_obs > 0 && (!A || !b || !nrows || !V || !nv))) { if (L) L->err = "bmpc_loop_set_obstacles: bad arguments"; return 1; }
    LCHK(L, hipSetDevice(L->dev));
    LCHK(L, hipStreamSynchronize(L->st));
    drop_obstacles(L);
    if (n_obs == 0) return 0;
    if (!obstacles_ok(L, (size_t)n_obs, nrows, nv)) return 1;
    return install_obstacles(L, (size_t)n_obs, A, b, nrows, V, nv, n_obs, &L->sc);
}

extern "C" int bmpc_loop_set_scenes(bmpc_loop* L, int n_scenes, const int* n_obs, const double* A, const double* b, const int* nrows,
                                    const double* V, const int* nv) {
    if (!L) return 1;
    if (n_scenes < 0 || (n_scenes > 0 && !n_obs)) { L->err = "bmpc_loop_set_scenes: bad arguments"; return 1; }
    std::vector<int> first((size_t)n_scenes + 1, 0);
    int max_obs = 0;
    for (int s = 0; s < n_scenes; s++) {
        if (n_obs[s] < 0 || n_obs[s] > LP_MAXOBS) { L->err = "bmpc_loop_set_scenes: a scene has more than 16 obstacles (or fewer than 0)"; return 1; }
        if (first[s] > INT_MAX - LP_MAXOBS) { L->err = "bmpc_loop_set_scenes: too many obstacles"; return 1; }
        first[s + 1] = first[s] + n_obs[s];
        if (n_obs[s] > max_obs) max_obs = n_obs[s];
    }
    const size_t total = (size_t)first[n_scenes];
    if (total > 0 && (!A || !b || !nrows || !V || !nv)) { L->err = "bmpc_loop_set_scenes: bad arguments"; return 1; }
    if (!obstacles_ok(L, total, nrows, nv)) return 1;
    LCHK(L, hipSetDevice(L->dev));
    LCHK(L, hipStreamSynchronize(L->st));
    drop_obstacles(L);
    if (n_scenes == 0) return 0;
    LoopSceneTable tab{};
    if (total > 0) { if (int rc = install_obstacles(L, total, A, b, nrows, V, nv, max_obs, &tab.all)) return rc; }
    const std::vector<int> none((size_t)L->R, -1);
    LCHK(L, hipMalloc((void**)&L->d_first, first.size() * sizeof(int)));
    LCHK(L, hipMemcpy(L->d_first, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice));
    LCHK(L, hipMalloc((void**)&L->d_rollout_scene, none.size() * sizeof(int)));
    LCHK(L, hipMemcpy(L->d_rollout_scene, none.data(), none.size() * sizeof(int), hipMemcpyHostToDevice));
    tab.first = L->d_first; tab.scene = L->d_rollout_scene; tab.n_scenes = n_scenes; tab.max_obs = max_obs;
    L->tab = tab;
    return 0;
}

extern "C" int bmpc_loop_set_rollout_scenes(bmpc_loop* L, int first, int count, const int* scene) {
    if (!range_ok(L, first, count)) return 1;
    if (!scene) { L->err = "bmpc_loop_set_rollout_scenes: bad arguments"; return 1; }
    for (int i = 0; i < count; i++)
        if (scene[i] < -1 || scene[i] >= L->tab.n_scenes) { L->err = "bmpc_loop_set_rollout_scenes: scene index out of range"; return 1; }
    if (L->tab.n_scenes == 0) return 0;       // no table: every rollout is at -1 already (or on the shared scene of bmpc_loop_set_obstacles)
    LCHK(L, hipSetDevice(L->dev));
    LCHK(L, hipStreamSynchronize(L->st));
    LCHK(L, hipMemcpy(L->d_rollout_scene + first, scene, (size_t)count * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

// ---- reference paths installed on the device (loop_install_path) ---------------------------------------------------------
// The arguments are checked on the host before anything is enqueued, so an error leaves the device state as it was.  Then, on
// the loop's stream and therefore after whatever is in flight: the staged copies, one bmpc_loop_k_install, the wait.
namespace {
struct InstArg { const void* host; size_t bytes; size_t off; };
constexpr size_t INST_ALIGN = 256;

int install_run(bmpc_loop* L, int count, int mode, int first, InstArg* a, int n_args) {
    size_t total = 0;
    for (int i = 0; i < n_args; i++) { a[i].off = total; total += (a[i].bytes + INST_ALIGN - 1) / INST_ALIGN * INST_ALIGN; }
    LCHK(L, hipSetDevice(L->dev));      // the calling host thread may be new
    if (total > L->inst_cap) {          // (every call here waits for its kernel, so the old block is idle)
        if (L->d_inst) (void)hipFree(L->d_inst);
        L->d_inst = nullptr; L->inst_cap = 0;
        LCHK(L, hipMalloc(&L->d_inst, total));
        L->inst_cap = total;
    }
    const char* d = (const char*)L->d_inst;
    for (int i = 0; i < n_args; i++)
        LCHK(L, hipMemcpyAsync((void*)(d + a[i].off), a[i].host, a[i].bytes, hipMemcpyHostToDevice, L->st));
    auto D = [&](int i) { return (const double*)(d + a[i].off); };
    LCHK(L, hipEventRecord(L->e0, L->st));
    if (mode == LP_INSTALL_FRESH)
        hipLaunchKernelGGL(bmpc_loop_k_install, dim3((count + 63) / 64), dim3(64), 0, L->st, count, L->N, L->d_rc, L->d_S, mode, (const int*)nullptr,
                           first, (const int*)nullptr, (const double*)nullptr, (const double*)nullptr, (const double*)nullptr, (const double*)nullptr,
                           (const double*)nullptr, (const double*)nullptr, (const double*)nullptr, D(0), D(1));
    else
        hipLaunchKernelGGL(bmpc_loop_k_install, dim3((count + 63) / 64), dim3(64), 0, L->st, count, L->N, L->d_rc, L->d_S, mode,
                           (const int*)(d + a[0].off), 0, (const int*)(d + a[1].off), D(2), D(3), D(4), D(5), D(6), D(7), D(8),
                           (const double*)nullptr, (const double*)nullptr);
    LCHK(L, hipGetLastError());
    LCHK(L, hipEventRecord(L->e1, L->st));
    LCHK(L, hipStreamSynchronize(L->st));
    LCHK(L, hipEventElapsedTime(&L->inst_ms, L->e0, L->e1));
    return 0;
}
}  // namespace

extern "C" int bmpc_loop_replan(bmpc_loop* L, int count, const int* rollouts, const int* n_pts, const double* p_via, const double* r_via,
                                const double* bp1, const double* br1, const double* e_r_bound, const double* a_sets, const double* b_sets) {
    if (!L) return 1;
    if (count == 0) return 0;
    if (count < 0 || !rollouts || !n_pts || !p_via || !r_via || !bp1 || !br1 || !e_r_bound || !a_sets || !b_sets) {
        L->err = "bmpc_loop_replan: bad arguments"; return 1;
    }
    std::vector<char> seen((size_t)L->R, 0);
    for (int i = 0; i < count; i++) {
        if (rollouts[i] < 0 || rollouts[i] >= L->R) { L->err = "bmpc_loop_replan: rollout index out of range"; return 1; }
        if (seen[(size_t)rollouts[i]]) { L->err = "bmpc_loop_replan: a rollout is listed twice"; return 1; }
        seen[(size_t)rollouts[i]] = 1;
        if (n_pts[i] < 2 || n_pts[i] > LP_MAXPTS) { L->err = "bmpc_loop_replan: a path needs 2 to 8 via points"; return 1; }
    }
    const size_t c = (size_t)count, NS = LP_MAXPTS - 1, D = sizeof(double);
    InstArg a[9] = {{rollouts, c * sizeof(int), 0}, {n_pts, c * sizeof(int), 0}, {p_via, c * 3 * LP_MAXPTS * D, 0}, {r_via, c * 9 * LP_MAXPTS * D, 0},
                    {bp1, c * 3 * NS * D, 0}, {br1, c * 3 * NS * D, 0}, {e_r_bound, c * 6 * NS * D, 0}, {a_sets, c * 45 * NS * D, 0},
                    {b_sets, c * LP_ROWS * NS * D, 0}};
    return install_run(L, count, LP_INSTALL_REPLAN, 0, a, 9);
}

extern "C" int bmpc_loop_init_rollouts(bmpc_loop* L, int first, int count, const double* q0, const double* weights) {
    if (!L) return 1;
    if (count == 0) return 0;
    if (!range_ok(L, first, count)) return 1;
    if (!q0 || !weights) { L->err = "bmpc_loop_init_rollouts: bad arguments"; return 1; }
    InstArg a[2] = {{q0, (size_t)count * 7 * sizeof(double), 0}, {weights, 11 * sizeof(double), 0}};
    return install_run(L, count, LP_INSTALL_FRESH, first, a, 2);
}

extern "C" float bmpc_loop_install_ms(const bmpc_loop* L) { return L ? L->inst_ms : 0.f; }

// n rollouts at most: all of them (list == nullptr, n == R) or those of a device list
static int launch_prepare(bmpc_loop* L, hipStream_t st, int n, const int* list = nullptr, const int* n_list = nullptr) {
    const size_t ne = (size_t)n * L->n_w;
    if (L->tab.n_scenes > 0) {             // one scene per rollout
        if (L->tab.max_obs > 0)
            hipLaunchKernelGGL(bmpc_loop_k_colpairs_scenes, dim3((n * 6 + 63) / 64, L->tab.max_obs), dim3(64), 0, st, L->R, L->d_rc, L->tab,
                               L->d_S, L->d_colres, list, n_list);
        hipLaunchKernelGGL(bmpc_loop_k_prepare_scenes, dim3((n + 63) / 64), dim3(64), 0, st, L->R, L->N, L->d_rc, L->d_S, L->d_prev,
                           L->d_p, L->d_lbx, L->d_ubx, L->tab, L->d_colres, list, n_list);
    } else {
        if (L->sc.n_obs > 0) {
            hipLaunchKernelGGL(bmpc_loop_k_colpairs, dim3((n * 6 + 63) / 64, L->sc.n_obs), dim3(64), 0, st, L->R, L->d_rc, L->sc, L->d_S,
                               L->d_colres, list, n_list);
        }
        hipLaunchKernelGGL(bmpc_loop_k_prepare, dim3((n + 63) / 64), dim3(64), 0, st, L->R, L->N, L->d_rc, L->d_S, L->d_prev,
                           L->d_p, L->d_lbx, L->d_ubx, L->sc, L->d_colres, list, n_list);
    }
    hipLaunchKernelGGL(bmpc_loop_k_x0, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, L->R, L->N, L->d_S, L->d_prev, L->d_x0,
                       list, n_list);
    LCHK(L, hipGetLastError());
    return 0;
}

static int launch_finish(bmpc_loop* L, hipStream_t st, int n, double* d_log_rows, const int* list = nullptr, const int* n_list = nullptr,
                         int* steps_left = nullptr, int* cont = nullptr, int nsteps = 0, double* d_rec_rows = nullptr) {
    const size_t ne = (size_t)n * L->n_w;
    hipLaunchKernelGGL(bmpc_loop_k_finish, dim3((n + 63) / 64), dim3(64), 0, st, L->R, L->N, L->dt, L->d_rc, L->d_S, L->d_x,
                       L->d_prev, L->d_status, L->d_viol, L->d_iters, d_log_rows, list, n_list, steps_left, cont, nsteps, L->d_p, d_rec_rows, L->d_rec_slot);
    hipLaunchKernelGGL(bmpc_loop_k_keep, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, L->R, L->N, L->d_S, L->d_x, L->d_prev,
                       list, n_list);
    LCHK(L, hipGetLastError());
    return 0;
}

static int ensure_log(bmpc_loop* L, size_t rows) {
    if (rows <= L->log_cap) return 0;
    if (L->d_log) (void)hipFree(L->d_log);
    L->d_log = nullptr; L->log_cap = 0;
    LCHK(L, hipMalloc((void**)&L->d_log, rows * LP_LOGW * sizeof(double)));
    L->log_cap = rows;
    return 0;
}

static int do_solve(bmpc_loop* L) {
    int rc = bmpc_solve_dev(L->h, L->R, L->d_x0, L->d_lbx, L->d_ubx, L->d_p, L->d_x, nullptr, L->d_f, L->d_iters, L->d_status,
                            L->d_viol, (void*)L->st);
    if (rc != 0) { L->err = std::string("bmpc_solve_dev: ") + bmpc_last_error(L->h); return rc; }
    return 0;
}

extern "C" int bmpc_loop_prepare(bmpc_loop* L) {
    if (!L) return 1;
    LCHK(L, hipSetDevice(L->dev));      // the calling host thread may be new
    if (int rc = launch_prepare(L, L->st, L->R)) return rc;
    LCHK(L, hipStreamSynchronize(L->st));
    return 0;
}

extern "C" int bmpc_loop_solve(bmpc_loop* L) { return L ? do_solve(L) : 1; }

extern "C" int bmpc_loop_finish(bmpc_loop* L, double* log) {
    if (!L) return 1;
    LCHK(L, hipSetDevice(L->dev));      // the calling host thread may be new
    if (log) { if (int rc = ensure_log(L, (size_t)L->R)) return rc; }
    if (L->n_rec > 0) {
        const size_t need = (size_t)L->n_rec * lp_rec_doubles(L->N);
        if (need > L->rec_cap) {
            if (L->d_rec) (void)hipFree(L->d_rec);
            L->d_rec = nullptr; L->rec_cap = 0;
            LCHK(L, hipMalloc((void**)&L->d_rec, need * sizeof(double)));
            L->rec_cap = need;
        }
    }
    if (L->n_rec > 0) LCHK(L, hipMemsetAsync(L->d_rec, 0, (size_t)L->n_rec * lp_rec_doubles(L->N) * sizeof(double), L->st));      // (a dead rollout's record stays zero)
    if (int rc = launch_finish(L, L->st, L->R, log ? L->d_log : nullptr, nullptr, nullptr, nullptr, nullptr, 0, L->n_rec > 0 ? L->d_rec : nullptr)) return rc;
    L->rec_steps = L->n_rec > 0 ? 1 : 0;
    LCHK(L, hipStreamSynchronize(L->st));
    if (log) LCHK(L, hipMemcpy(log, L->d_log, (size_t)L->R * LP_LOGW * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int bmpc_loop_run(bmpc_loop* L, int nsteps, double* log, float* ms_total, float* ms_solve) {
    if (!L || nsteps <= 0) return 1;
    LCHK(L, hipSetDevice(L->dev));      // the calling host thread may be new
    if (log) { if (int rc = ensure_log(L, (size_t)nsteps * L->R)) return rc; }
    if (L->n_rec > 0) {
        const size_t need = (size_t)nsteps * L->n_rec * lp_rec_doubles(L->N);
        if (need > L->rec_cap) {
            if (L->d_rec) (void)hipFree(L->d_rec);
            L->d_rec = nullptr; L->rec_cap = 0;
            LCHK(L, hipMalloc((void**)&L->d_rec, need * sizeof(double)));
            L->rec_cap = need;
        }
    }
    double solve_s = 0.0;
    if (L->n_rec > 0) LCHK(L, hipMemsetAsync(L->d_rec, 0, (size_t)nsteps * L->n_rec * lp_rec_doubles(L->N) * sizeof(double), L->st));     // (a dead rollout's record stays zero)
    LCHK(L, hipEventRecord(L->e0, L->st));
    for (int s = 0; s < nsteps; s++) {
        if (int rc = launch_prepare(L, L->st, L->R)) return rc;
        auto t0 = std::chrono::steady_clock::now();
        if (int rc = do_solve(L)) return rc;
        solve_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        double* recs = L->n_rec > 0 ? L->d_rec + (size_t)s * L->n_rec * lp_rec_doubles(L->N) : nullptr;
        if (int rc = launch_finish(L, L->st, L->R, log ? L->d_log + (size_t)s * L->R * LP_LOGW : nullptr, nullptr, nullptr, nullptr, nullptr, 0, recs)) return rc;
    }
    L->rec_steps = L->n_rec > 0 ? (size_t)nsteps : 0;
    LCHK(L, hipEventRecord(L->e1, L->st));
    LCHK(L, hipStreamSynchronize(L->st));
    float ms = 0.f;
    LCHK(L, hipEventElapsedTime(&ms, L->e0, L->e1));
    if (ms_total) *ms_total = ms;
    if (ms_solve) *ms_solve = (float)(1e3 * solve_s);
    if (log) LCHK(L, hipMemcpy(log, L->d_log, (size_t)nsteps * L->R * LP_LOGW * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// ---- closed loop without lock step ---------------------------------------------------------------------------------------
// The rollouts are independent, so nothing but convenience makes them wait for each other: here every rollout is a row of
// ONE hooked solver call (bmpc_capi.hip).  When the solve of a rollout's current step retires, the hook below runs the
// finish / keep / collision-pair / prepare / start-vector kernels for just those rollouts, and the solver re-admits the
// slot with the rollout's next problem at the start of the following super-step.  The straggler tail is then paid once per
// run instead of once per MPC step.  Per-rollout arithmetic does not depend on the schedule: the log equals bmpc_loop_run's.
static int loop_retire_hook(void* ctx, const int* d_done, const int* d_n_done, int n_max, void* stream) {
    bmpc_loop* L = (bmpc_loop*)ctx;
    hipStream_t st = (hipStream_t)stream;
    if (n_max > L->R) n_max = L->R;          // the solver's slot count may exceed the rollouts (workspace sized by max_batch)
    if (int rc = launch_finish(L, st, n_max, L->async_log, d_done, d_n_done, L->d_steps_left, L->d_cont, L->async_nsteps)) return rc;
    if (int rc = launch_prepare(L, st, n_max, d_done, d_n_done)) return rc;
    return 0;
}

extern "C" int bmpc_loop_run_async(bmpc_loop* L, int nsteps, double* log, float* ms_total) {
    if (!L || nsteps <= 0) return 1;
    LCHK(L, hipSetDevice(L->dev));
    if (log) { if (int rc = ensure_log(L, (size_t)nsteps * L->R)) return rc; }
    if (!L->d_steps_left) {
        LCHK(L, hipMalloc((void**)&L->d_steps_left, (size_t)L->R * sizeof(int)));
        LCHK(L, hipMalloc((void**)&L->d_cont, (size_t)L->R * sizeof(int)));
    }
    std::vector<int> left((size_t)L->R, nsteps);
    LCHK(L, hipMemcpyAsync(L->d_steps_left, left.data(), left.size() * sizeof(int), hipMemcpyHostToDevice, L->st));
    LCHK(L, hipMemsetAsync(L->d_cont, 0, (size_t)L->R * sizeof(int), L->st));
    LCHK(L, hipStreamSynchronize(L->st));       // `left` goes out of scope below
    L->async_nsteps = nsteps;
    L->async_log = log ? L->d_log : nullptr;
    LCHK(L, hipEventRecord(L->e0, L->st));
    if (int rc = launch_prepare(L, L->st, L->R)) return rc;         // step 0 of every rollout
    int rc = bmpc_solve_dev_hooked(L->h, L->R, L->d_x0, L->d_lbx, L->d_ubx, L->d_p, L->d_x, L->d_f, L->d_iters, L->d_status, L->d_viol,
                                   (void*)L->st, loop_retire_hook, L, L->d_cont);
    if (rc != 0) { L->err = std::string("bmpc_solve_dev_hooked: ") + bmpc_last_error(L->h); return rc; }
    LCHK(L, hipEventRecord(L->e1, L->st));
    LCHK(L, hipStreamSynchronize(L->st));
    float ms = 0.f;
    LCHK(L, hipEventElapsedTime(&ms, L->e0, L->e1));
    if (ms_total) *ms_total = ms;
    if (log) LCHK(L, hipMemcpy(log, L->d_log, (size_t)nsteps * L->R * LP_LOGW * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int bmpc_loop_problem(bmpc_loop* L, double* x0, double* lbx, double* ubx, double* p) {
    if (!L) return 1;
    LCHK(L, hipSetDevice(L->dev));      // the calling host thread may be new
    LCHK(L, hipStreamSynchronize(L->st));
    const size_t nw = (size_t)L->R * L->n_w * sizeof(double);
    if (x0) LCHK(L, hipMemcpy(x0, L->d_x0, nw, hipMemcpyDeviceToHost));
    if (lbx) LCHK(L, hipMemcpy(lbx, L->d_lbx, nw, hipMemcpyDeviceToHost));
    if (ubx) LCHK(L, hipMemcpy(ubx, L->d_ubx, nw, hipMemcpyDeviceToHost));
    if (p) LCHK(L, hipMemcpy(p, L->d_p, (size_t)L->R * NPAR * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int bmpc_loop_solution(bmpc_loop* L, double* x, int* iters, int* status, double* viol) {
    if (!L) return 1;
    LCHK(L, hipSetDevice(L->dev));      // the calling host thread may be new
    LCHK(L, hipStreamSynchronize(L->st));
    if (x) LCHK(L, hipMemcpy(x, L->d_x, (size_t)L->R * L->n_w * sizeof(double), hipMemcpyDeviceToHost));
    if (iters) LCHK(L, hipMemcpy(iters, L->d_iters, (size_t)L->R * sizeof(int), hipMemcpyDeviceToHost));
    if (status) LCHK(L, hipMemcpy(status, L->d_status, (size_t)L->R * sizeof(int), hipMemcpyDeviceToHost));
    if (viol) LCHK(L, hipMemcpy(viol, L->d_viol, (size_t)L->R * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int bmpc_loop_set_solution(bmpc_loop* L, const double* x, const int* iters, const int* status, const double* viol) {
    if (!L || !x || !status || !viol) return 1;
    LCHK(L, hipSetDevice(L->dev));      // the calling host thread may be new
    LCHK(L, hipMemcpy(L->d_x, x, (size_t)L->R * L->n_w * sizeof(double), hipMemcpyHostToDevice));
    if (iters) LCHK(L, hipMemcpy(L->d_iters, iters, (size_t)L->R * sizeof(int), hipMemcpyHostToDevice));
    LCHK(L, hipMemcpy(L->d_status, status, (size_t)L->R * sizeof(int), hipMemcpyHostToDevice));
    LCHK(L, hipMemcpy(L->d_viol, viol, (size_t)L->R * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}
