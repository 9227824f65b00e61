// libboundmpc_hip.so: C ABI (include/boundmpc.h) of the handle and the solver + the solver's launch sequence for gfx950.
// The batched one-launch kernels' entries (bmpc_fk, bmpc_ik, bmpc_convex_sets): bmpc_capi_batch.hip.
#include "bmpc_platform_hip.hpp"

#define BMPC_NT 64
#include "bmpc_handle.hpp"
#include "bmpc_internal.hpp"
#include "bmpc_staging.hpp"
#include "bmpc_debug_step.hpp"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace bmpc;

static int pipe_ensure(bmpc_handle* h, int B);

// (contract: bmpc_handle.hpp)
int wait_stream(bmpc_handle* h, hipStream_t st) {
    if (h->o.watchdog_ms <= 0) { HIPCHK(h, hipStreamSynchronize(st)); return 0; }
    HIPCHK(h, hipEventRecord(h->ev_wait, st));
    const auto t0 = std::chrono::steady_clock::now();
    for (long spins = 0;; spins++) {
        const hipError_t q = hipEventQuery(h->ev_wait);
        if (q == hipSuccess) return 0;
        if (q != hipErrorNotReady) { h->err = std::string("hipEventQuery: ") + hipGetErrorString(q); return 2; }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms > h->o.watchdog_ms) {
            h->wedged = true;
            h->err = "watchdog: the GPU did not finish the enqueued work within " + std::to_string(h->o.watchdog_ms) +
                     " ms (bmpc_opts.watchdog_ms); the handle is unusable, destroy it";
            return 5;
        }
        if (ms < 2.0) std::this_thread::yield();            // a burst of super-steps takes a few ms: stay responsive
        else std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

extern "C" void bmpc_default_opts(bmpc_opts* o, int N) {
    o->N = N; o->nr_segs = 4; o->dt = 0.1; o->tol = 1e-5; o->max_iter = 100; o->device = 0;
    o->hess = 2; o->hess_switch = 1.0; o->mu_init = 0.1; o->kappa_mu = 0.1; o->theta_mu = 2.0; o->kappa_eps = 1000.0;
    o->mu_floor_k = 1e4; o->inertia = 2; o->dw0 = 1e-4; o->inertia_err = 1e-2; o->stall_n = 8; o->gn_backoff = 2; o->slack_reset = 1; o->ls_alpha_mem = 0.0; o->trial_repeats = 9;
    o->max_batch = 0; o->pool_slots = 0; o->watchdog_ms = 30000;
}

extern "C" int bmpc_create(const bmpc_opts* o, bmpc_handle** out) {
    if (!o || !out) return 1;
    *out = nullptr;
    if (o->N < 3 || o->N > 64 || o->nr_segs != 4 || !(o->dt > 0)) return 1;
    if (o->inertia < 0 || o->inertia > 2 || !(o->dw0 > 0) || o->mu_floor_k < 0) return 1;
    if (o->pool_slots < 0 || (o->pool_slots > 0 && o->pool_slots < 64)) return 1;
    bmpc_handle* h = new bmpc_handle();
    h->o = *o;
    h->o.trial_repeats = o->trial_repeats < 0 ? 0 : (o->trial_repeats > 9 ? 9 : o->trial_repeats);     // a line search has at most ten trials
    h->n_w = 44 * o->N + 6;
    h->n_g = 147 * (o->N - 1) + 21;
    *out = h;   // returned even on a HIP failure so that bmpc_last_error() can be read
    int ndev = 0;
    HIPCHK(h, hipGetDeviceCount(&ndev));
    if (ndev <= 0) { h->err = "no HIP device"; return 2; }
    HIPCHK(h, hipSetDevice(o->device));
    hipDeviceProp_t prop;
    HIPCHK(h, hipGetDeviceProperties(&prop, o->device));
    h->n_cu = prop.multiProcessorCount;
    h->nblocks_max = h->n_cu * 3;      // rows of the diagnostic cycle counters
    RobotConst rc;
    robot_iiwa14(h->robot);
    fill_robot_const(rc, h->robot);
    HIPCHK(h, hipMalloc((void**)&h->d_rc, sizeof(RobotConst)));
    HIPCHK(h, hipMemcpy(h->d_rc, &rc, sizeof(RobotConst), hipMemcpyHostToDevice));
    HIPCHK(h, hipMalloc((void**)&h->d_prof, (size_t)h->nblocks_max * 16 * sizeof(double)));
    HIPCHK(h, hipMemset(h->d_prof, 0, (size_t)h->nblocks_max * 16 * sizeof(double)));
    {
        std::vector<int> tbl(3 * HREC);
        bmpc_pipe_build_table(tbl.data());
        HIPCHK(h, hipMalloc((void**)&h->d_pipe_tbl, tbl.size() * sizeof(int)));
        HIPCHK(h, hipMemcpy(h->d_pipe_tbl, tbl.data(), tbl.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(h, hipHostMalloc((void**)&h->h_cnt, NCNT * sizeof(int)));
    }
    HIPCHK(h, hipStreamCreate(&h->stream));
    HIPCHK(h, hipEventCreate(&h->ev0));
    HIPCHK(h, hipEventCreate(&h->ev1));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_wait, hipEventDisableTiming));
    if (o->max_batch > 0) return pipe_ensure(h, o->max_batch);   // workspace up front
    return 0;
}

// (bmpc_internal.hpp)
extern "C" void bmpc_handle_retain(bmpc_handle* h) { if (h) h->n_loops.fetch_add(1); }
extern "C" void bmpc_handle_release(bmpc_handle* h) {
    if (!h) return;
    if (h->n_loops.fetch_sub(1) == 1 && h->destroy_pending) { h->destroy_pending = false; bmpc_destroy(h); }
}

extern "C" void bmpc_destroy(bmpc_handle* h) {
    if (!h) return;
    if (h->n_loops.load() > 0) { h->destroy_pending = true; return; }     // deferred until the last loop is gone
    if (h->worker.joinable()) h->worker.join();
    if (h->wedged) {
        // The handle ran into its watchdog: its stream may never drain, and kernels still queued on it may write the workspace.
        // Nothing is waited for and nothing is freed -- device buffers, events and the stream are leaked on purpose (a
        // hipStreamSynchronize / hipFree here is the unbounded wait the watchdog exists to prevent).  The process should end
        // with an error and let a fresh one take over (include/boundmpc.h, bmpc_opts.watchdog_ms).
        delete h;
        return;
    }
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (hipEvent_t e : h->ric_ev) if (e) (void)hipEventDestroy(e);
    void* bufs[] = {h->d_x0, h->d_lbx, h->d_ubx, h->d_p, h->d_x, h->d_g, h->d_f, h->d_viol, h->d_iters, h->d_status, h->d_rc, h->d_prof,
                    h->d_pipe, h->d_pipe_st, h->d_pipe_lists, h->d_pipe_tbl, h->d_lam_g, h->d_lam_x};
    for (void* b : bufs) if (b) (void)hipFree(b);
    if (h->h_cnt) (void)hipHostFree(h->h_cnt);
    for (hipEvent_t e : {h->ev0, h->ev1, h->ev_wait}) if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

extern "C" const char* bmpc_last_error(const bmpc_handle* h) { return h ? h->err.c_str() : "null handle"; }

extern "C" int bmpc_dims(const bmpc_handle* h, int* n_w, int* n_g, int* n_p) {
    if (!h) return 1;
    if (n_w) *n_w = h->n_w;
    if (n_g) *n_g = h->n_g;
    if (n_p) *n_p = NPAR;
    return 0;
}

extern "C" void bmpc_robot_iiwa14(bmpc_robot* r) { if (r) robot_iiwa14(*r); }
extern "C" void bmpc_robot_gen3(bmpc_robot* r) { if (r) robot_gen3(*r); }

extern "C" int bmpc_set_robot(bmpc_handle* h, const bmpc_robot* r) {
    if (!h || !r) return 1;
    WEDGED_FAIL(h);
    int rc_ = bmpc_wait(h);
    if (rc_) return rc_;
    BUSY_OR_FAIL(h, "bmpc_set_robot");
    for (int i = 0; i < 7; i++)
        if (!(r->q_lower[i] <= r->q_upper[i]) || !(r->dq_max[i] > 0) || !(r->col_joint_sizes[i] >= 0)) { h->err = "bmpc_set_robot: inconsistent limits"; return 1; }
    if (!(r->ddq_max > 0) || !(r->u_max > 0)) { h->err = "bmpc_set_robot: inconsistent limits"; return 1; }
    HIPCHK(h, hipSetDevice(h->o.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    RobotConst rc;
    fill_robot_const(rc, *r);
    HIPCHK(h, hipMemcpy(h->d_rc, &rc, sizeof(RobotConst), hipMemcpyHostToDevice));
    h->robot = *r;
    h->last_valid = false;
    return 0;
}
extern "C" int bmpc_get_robot(const bmpc_handle* h, bmpc_robot* r) {
    if (!h || !r) return 1;
    *r = h->robot;
    return 0;
}

extern "C" void* bmpc_stream(bmpc_handle* h) { return h ? (void*)h->stream : nullptr; }

extern "C" int bmpc_get_opts(const bmpc_handle* h, bmpc_opts* o) {
    if (!h || !o) return 1;
    *o = h->o;
    return 0;
}

extern "C" int bmpc_gbounds(const bmpc_handle* h, double* lbg, double* ubg) {
    if (!h || !lbg || !ubg) return 1;
    const double INF = 1e20;
    const int N = h->o.N;
    int r = 0;
    auto put = [&](int n, double lo, double hi) { for (int i = 0; i < n; i++) { lbg[r] = lo; ubg[r] = hi; r++; } };
    put(35 * (N - 1), 0, 0);
    for (int k = 1; k < N; k++) {
        put(15, -INF, 0); put(3, -INF, 0); put(3, 0, INF); put(90, -INF, 0); put(1, -INF, 0);
        if (k == N - 1) { put(15, -INF, 0); put(3, -INF, 0); put(3, 0, INF); }
    }
    return r == h->n_g ? 0 : 1;
}

// ------------------------------------------------------------------------------------------
// workspace + launch sequence
// ------------------------------------------------------------------------------------------
// The work lists of pipe_solve in d_pipe_lists: 8 lists and the slot -> row map of `cap` ints each, then the NCNT counters.  Returns
// the slot -> row map.
static size_t pipe_list_ints(int cap) { return 9 * (size_t)cap + NCNT; }
static int* pipe_lists_carve(ListsT<0>& L, int* base, int cap) {
    const size_t c = (size_t)cap;
    L.eval = base; L.step = base + c; L.trial = base + 2 * c; L.eval_next = base + 3 * c; L.trial_next = base + 4 * c;
    L.done = base + 5 * c; L.admit = base + 6 * c; L.curv = base + 8 * c; L.cnt = base + 9 * c;
    return base + 7 * c;
}

// workspace for `B` slots; a handle created with pool_slots > 0 never holds more than that many (larger batches stream
// through the pool, bmpc_opts.pool_slots)
static int pipe_ensure(bmpc_handle* h, int B) {
    if (h->o.pool_slots > 0 && B > h->o.pool_slots) B = h->o.pool_slots;
    if (B <= h->pipe_cap) return 0;
    int cap = B > h->o.max_batch ? B : h->o.max_batch;
    if (h->o.pool_slots > 0 && cap > h->o.pool_slots) cap = h->o.pool_slots;
    if (h->d_pipe) { (void)hipFree(h->d_pipe); h->d_pipe = nullptr; }
    if (h->d_pipe_st) { (void)hipFree(h->d_pipe_st); h->d_pipe_st = nullptr; }
    if (h->d_pipe_lists) { (void)hipFree(h->d_pipe_lists); h->d_pipe_lists = nullptr; }
    h->pipe_cap = 0;
    const size_t n = pipe_workspace_doubles(cap, h->o.N, h->slot_major);
    HIPCHK(h, hipMalloc((void**)&h->d_pipe, n * sizeof(double)));
    HIPCHK(h, hipMalloc((void**)&h->d_pipe_st, (size_t)cap * bmpc_pipe_state_bytes()));
    HIPCHK(h, hipMalloc((void**)&h->d_pipe_lists, pipe_list_ints(cap) * sizeof(int)));
    h->pipe_cap = cap;
    return 0;
}

// one super-step; with bmpc_debug_time_ric the Riccati launch is bracketed by an event pair (collected by ric_collect after the
// next wait for the stream)
static hipError_t step_timed(bmpc_handle* h, PipeArgsH* A, int n_act, hipStream_t st) {
    if (!h->time_ric || h->ric_pending >= 8) return bmpc_pipe_launch_step(A, n_act, st, nullptr, nullptr, nullptr);
    const int i = h->ric_pending++;
    h->ric_nact[i] = n_act;
    return bmpc_pipe_launch_step(A, n_act, st, h->ric_ev[2 * i], h->ric_ev[2 * i + 1], &h->ric_is_lat[i]);
}
static void ric_collect(bmpc_handle* h) {        // the stream is idle: every recorded pair has completed
    for (int i = 0; i < h->ric_pending; i++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->ric_ev[2 * i], h->ric_ev[2 * i + 1]) == hipSuccess) {
            h->ric_ms[h->ric_is_lat[i] ? 1 : 0] += ms; h->ric_launches[h->ric_is_lat[i] ? 1 : 0] += 1;
            if (!h->ric_is_lat[i] && h->ric_nact[i] >= h->ric_full_n) { h->ric_full[0] += ms; h->ric_full[1] += 1; h->ric_full[2] += h->ric_nact[i]; }
        }
    }
    h->ric_pending = 0;
}

static SolverOpts solver_opts(const bmpc_opts& o) {
    return SolverOpts{o.N, o.dt, o.tol, o.max_iter, o.hess, o.hess_switch, o.mu_init, o.kappa_mu, o.theta_mu, o.kappa_eps,
                      o.mu_floor_k, o.dw0, o.inertia_err, o.ls_alpha_mem, o.inertia, o.stall_n, o.gn_backoff, o.slack_reset, o.trial_repeats};
}
// The argument block of a run over the handle's workspace (pipe_ensure), all of it that does not depend on the caller's arrays: the
// caller sets x0, lbx, ubx, p, x, f, viol, g, iters, status (and cont).  Whatever the last solve left in the workspace is given up.
static PipeArgsH pipe_args(bmpc_handle* h, int B) {
    const int N = h->o.N, cap = h->pipe_cap;
    PipeArgsH A{};
    A.B = B; A.N = N; A.natt = 0; A.pad0_ = 0;
    A.o = solver_opts(h->o);
    A.rc = h->d_rc;
    pipe_carve(A, h->d_pipe, cap, N, h->slot_major);
    A.st = (InstState*)h->d_pipe_st;
    A.src = pipe_lists_carve(A.L, h->d_pipe_lists, cap);
    A.tbl = h->d_pipe_tbl;
    A.prof = h->d_prof;
    A.lam_g = nullptr; A.lam_x = nullptr; A.cont = nullptr;
    h->last_valid = false;
    return A;
}
// first fill of the pool: slots 0 .. n0-1 take the first n0 input rows and are initialised.  `ev` (optional) is recorded after the
// counter upload and before the launches (ev0 of a solve: bmpc_last_kernel_ms starts at the first kernel).
static int pipe_seed(bmpc_handle* h, const PipeArgsH& A, int n0, hipStream_t st, hipEvent_t ev = nullptr) {
    for (int& c : h->cnt_seed) c = 0;
    h->cnt_seed[0] = n0; h->cnt_seed[6] = n0; h->cnt_seed[9] = n0;
    HIPCHK(h, hipMemcpyAsync(A.L.cnt, h->cnt_seed, sizeof h->cnt_seed, hipMemcpyHostToDevice, st));
    if (ev) HIPCHK(h, hipEventRecord(ev, st));
    HIPCHK(h, bmpc_pipe_launch_init(&A, n0, st));
    return 0;
}

// one pipe_solve between its set-up, its driver and its epilogue
struct PipeRun {
    bmpc_handle* h;
    int B, cap, n0;                 // rows, slots, slots filled at the start
    hipStream_t st;
    PipeArgsH A;
    bmpc_retire_hook hook; void* hook_ctx;
    int steps = 0, retired = 0;
};
// retirement of the (at most n_max) instances that finished: outputs, the caller's hook, (re-)admission
static int retire(PipeRun& R, int n_max, int refill) {
    bmpc_handle* h = R.h;
    HIPCHK(h, bmpc_pipe_launch_retire_out(&R.A, n_max, R.st));
    if (R.hook) { if (int r = R.hook(R.hook_ctx, R.A.L.done, R.A.L.cnt + 8, n_max, (void*)R.st)) { h->err = "retire hook failed"; return r; } }
    HIPCHK(h, bmpc_pipe_launch_retire_admit(&R.A, n_max, refill, R.st));
    return 0;
}
// the counters come back on st; the stream is idle afterwards, so the event pairs of step_timed are collected too
static int read_counters(bmpc_handle* h, const PipeArgsH& A, hipStream_t st) {
    HIPCHK(h, hipMemcpyAsync(h->h_cnt, A.L.cnt, NCNT * sizeof(int), hipMemcpyDeviceToHost, st));
    if (int r = wait_stream(h, st)) return r;
    ric_collect(h);
    return 0;
}

// Driver of a batch.  The workspace is a pool of `cap` slots.  B <= cap: every instance has its slot (slot = row).  B > cap (a handle
// created with pool_slots): the rows stream through the pool -- a slot whose instance has finished is retired (outputs written)
// and takes the next row at the start of the following super-step, so the kernels keep working on ~cap instances until the input
// runs out and only ONE straggler tail is paid for the whole call.
// Every instance advances one stage of its own state machine per super-step; finished instances leave the work lists.  The host
// only needs upper bounds of the list lengths to size the grids, and the retired count to stop: read back every few super-steps.
static int drive_batch(PipeRun& R) {
    bmpc_handle* h = R.h;
    const int B = R.B, cap = R.cap;
    const hipStream_t st = R.st;
    const bool streaming = B > cap;
    int n_act = R.n0, next_row = R.n0;
    const long max_steps = 12L * (h->o.max_iter + 2) * ((B + cap - 1) / cap + 1);
    while (R.retired < B && R.steps < max_steps) {
        const int burst = R.steps < 8 ? 8 : 4;
        // while input rows are left (as far as the host knows: next_row only grows), finished instances make room before
        // every super-step; afterwards they are retired once per burst
        const bool rows_left = streaming && next_row < B;
        for (int i = 0; i < burst; i++, R.steps++) {
            if (rows_left && i > 0) { if (int r = retire(R, cap, 1)) return r; }
            HIPCHK(h, step_timed(h, &R.A, rows_left ? cap : n_act, st));
        }
        if (int r = retire(R, rows_left ? cap : n_act, rows_left ? 1 : 0)) return r;
        if (int r = read_counters(h, R.A, st)) return r;
        R.retired = h->h_cnt[7];
        next_row = h->h_cnt[6] < B ? h->h_cnt[6] : B;
        n_act = next_row - R.retired;
        if (streaming && next_row < B) n_act = cap < B ? cap : B;
        h->n_active.store(B - R.retired);
    }
    return 0;
}

// Driver of the closed loop without lock step (a retire hook: every row is a rollout, its slot is refilled with the same row's next
// problem): a burst of super-steps, then the counters come back and exactly the rollouts whose solve finished in this burst (cnt[8],
// the done list) are retired -- outputs, the caller's hook (post-processing, next problem), re-admission -- with grids sized by that
// count; nothing is launched when nobody finished.  (Round 3 ran the whole retirement sequence before every super-step with grids
// sized for all rollouts: ~1 ms of empty launches per super-step.)  A finished rollout waits at most one burst for its next problem.
static int drive_closed_loop(PipeRun& R) {
    bmpc_handle* h = R.h;
    const int B = R.B;
    const hipStream_t st = R.st;
    int n_act = R.n0;
    while (R.retired < B) {      // (no bound on the super-steps: how long a rollout lasts is the caller's business)
        const int burst = R.steps < 8 ? 8 : 4;
        for (int i = 0; i < burst; i++, R.steps++) HIPCHK(h, step_timed(h, &R.A, n_act, st));
        if (int r = read_counters(h, R.A, st)) return r;
        const int n_done = h->h_cnt[8];
        if (n_done > 0) { if (int r = retire(R, n_done, 1)) return r; }
        R.retired = h->h_cnt[7];      // rows whose rollout has ended (counted by k_admit: one burst behind)
        if (n_done > 0 && R.retired + n_done >= B) {      // possibly the last ones: their retirement decides whether anybody goes on
            if (int r = read_counters(h, R.A, st)) return r;
            R.retired = h->h_cnt[7];
        }
        n_act = B - R.retired;
        h->n_active.store(B - R.retired);
    }
    return 0;
}

static int pipe_solve(bmpc_handle* h, int B, const double* d_x0, const double* d_lbx, const double* d_ubx,
                      const double* d_p, double* d_x, double* d_g, double* d_f, int* d_iters, int* d_status,
                      double* d_viol, hipStream_t st, bmpc_retire_hook hook = nullptr, void* hook_ctx = nullptr,
                      const int* d_cont = nullptr) {
    WEDGED_FAIL(h);
    int rc = pipe_ensure(h, B);
    if (rc) return rc;
    const int cap = h->pipe_cap;
    PipeRun R{h, B, cap, B < cap ? B : cap, st, pipe_args(h, B), hook, hook_ctx};
    PipeArgsH& A = R.A;
    A.x0 = d_x0; A.lbx = d_lbx; A.ubx = d_ubx; A.p = d_p;
    A.x = d_x; A.f = d_f; A.viol = d_viol; A.g = d_g; A.iters = d_iters; A.status = d_status;
    A.cont = d_cont;
    if (hook && B > cap) { h->err = "closed-loop solve: more rollouts than workspace slots"; return 1; }
    if (int r = pipe_seed(h, A, R.n0, st, h->ev0)) return r;
    h->n_active.store(B);
    h->ric_pending = 0; h->ric_ms[0] = h->ric_ms[1] = 0; h->ric_launches[0] = h->ric_launches[1] = 0;
    h->ric_full_n = R.n0; h->ric_full[0] = h->ric_full[1] = h->ric_full[2] = 0;
    if (int r = hook ? drive_closed_loop(R) : drive_batch(R)) return r;
    h->last_steps = R.steps;
    h->ric_sweeps[0] = h->h_cnt[11]; h->ric_sweeps[1] = h->h_cnt[12];
    HIPCHK(h, hipEventRecord(h->ev1, st));
    // the outputs are complete and the per-handle workspace is free when the call returns (the drivers synchronised)
    if (int r = wait_stream(h, st)) return r;
    if (R.retired < B) { h->err = "pipeline did not drain (internal error)"; return 3; }
    const bool streaming = B > cap || hook != nullptr;      // slots were refilled (closed loop: with the same row's next problem)
    h->last_args = A; h->last_valid = !streaming;      // multipliers need every instance's final iterate in its slot
    h->last_args.cont = nullptr;
    return 0;
}

extern "C" int bmpc_solve_dev(bmpc_handle* h, int B, const double* d_x0, const double* d_lbx,
                              const double* d_ubx, const double* d_p, double* d_x, double* d_g, double* d_f,
                              int* d_iters, int* d_status, double* d_viol, void* stream) {
    if (!h || B < 0 || !d_x0 || !d_lbx || !d_ubx || !d_p || !d_x || !d_f || !d_iters || !d_status || !d_viol) {
        if (h) h->err = "bmpc_solve_dev: null argument";
        return 1;
    }
    int wrc = bmpc_wait(h);        // an asynchronous solve in flight owns the workspace
    if (wrc) return wrc;
    if (B == 0) return 0;
    BUSY_OR_FAIL(h, "bmpc_solve_dev");
    HIPCHK(h, hipSetDevice(h->o.device));
    return pipe_solve(h, B, d_x0, d_lbx, d_ubx, d_p, d_x, d_g, d_f, d_iters, d_status, d_viol, (hipStream_t)stream);
}

// (bmpc_internal.hpp; called by bmpc_loop.hip)
extern "C" int bmpc_solve_dev_hooked(bmpc_handle* h, int B, const double* d_x0, const double* d_lbx, const double* d_ubx,
                                     const double* d_p, double* d_x, double* d_f, int* d_iters, int* d_status, double* d_viol,
                                     void* stream, bmpc_retire_hook hook, void* hook_ctx, const int* d_cont) {
    if (!h || B <= 0 || !hook || !d_cont) return 1;
    int wrc = bmpc_wait(h);
    if (wrc) return wrc;
    BUSY_OR_FAIL(h, "bmpc_loop_run_async");
    HIPCHK(h, hipSetDevice(h->o.device));
    return pipe_solve(h, B, d_x0, d_lbx, d_ubx, d_p, d_x, nullptr, d_f, d_iters, d_status, d_viol, (hipStream_t)stream, hook, hook_ctx, d_cont);
}

// Asynchronous form of bmpc_solve_dev: returns at once; the data-dependent launch sequence is driven by
// a worker thread on the handle's own stream.  One solve in flight per handle (a second call waits for
// the first).  Two handles used alternately overlap the straggler tail of one batch (few active
// instances, launch-latency bound) with the bulk of the next.
// unfinished instances of the solve in flight on this handle (0 when idle): lets a caller that keeps
// several batches in flight start the next one when the previous has left its bulk phase
extern "C" int bmpc_active(bmpc_handle* h) { return h ? h->n_active.load() : 0; }

extern "C" int bmpc_wait(bmpc_handle* h) {
    if (!h) return 1;
    if (h->worker.joinable()) h->worker.join();
    int rc = h->worker_rc;
    h->worker_rc = 0;
    return rc;
}

extern "C" int bmpc_solve_dev_async(bmpc_handle* h, int B, const double* d_x0, const double* d_lbx,
                                    const double* d_ubx, const double* d_p, double* d_x, double* d_g, double* d_f,
                                    int* d_iters, int* d_status, double* d_viol) {
    if (!h || B < 0 || !d_x0 || !d_lbx || !d_ubx || !d_p || !d_x || !d_f || !d_iters || !d_status || !d_viol) {
        if (h) h->err = "bmpc_solve_dev_async: null argument";
        return 1;
    }
    int rc = bmpc_wait(h);
    if (rc) return rc;
    if (B == 0) return 0;
    { bool f = false; if (!h->busy.compare_exchange_strong(f, true)) return 4; }
    h->n_active.store(B);
    h->worker = std::thread([=]() {      // the worker owns the handle until it is done (bmpc_wait joins it)
        int r = 0;
        if (hipSetDevice(h->o.device) != hipSuccess) { h->err = "hipSetDevice failed in the worker"; r = 2; }
        if (r == 0) r = pipe_solve(h, B, d_x0, d_lbx, d_ubx, d_p, d_x, d_g, d_f, d_iters, d_status, d_viol, h->stream);
        if (r == 0) r = wait_stream(h, h->stream);
        h->worker_rc = r;
        if (r != 0) h->n_active.store(0);        // a failed solve is not "active" for ever; bmpc_wait reports the code
        h->busy.store(false);
    });
    return 0;
}

// Multipliers of the most recent solve on this handle: its final iterate and row multipliers are still
// in the workspace.  d_lam_g [B][n_g], d_lam_x [B][n_w]: device pointers; enqueued on `stream` and waited for.
extern "C" int bmpc_multipliers_dev(bmpc_handle* h, int B, double* d_lam_g, double* d_lam_x, void* stream) {
    if (!h || !d_lam_g || !d_lam_x) { if (h) h->err = "bmpc_multipliers_dev: null argument"; return 1; }
    WEDGED_FAIL(h);
    int rc = bmpc_wait(h);
    if (rc) return rc;
    if (!h->last_valid || h->last_args.B != B) { h->err = "bmpc_multipliers_dev: no finished solve of this batch size on the handle"; return 1; }
    HIPCHK(h, hipSetDevice(h->o.device));
    PipeArgsH A = h->last_args;
    A.lam_g = d_lam_g; A.lam_x = d_lam_x;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(h, bmpc_pipe_launch_mult(&A, st));
    if (int r = wait_stream(h, st)) return r;
    return 0;
}

// a typed device buffer of the handle: freed if set, null, then `count` elements allocated (0: none)
template <class T> static int dev_realloc(bmpc_handle* h, T** p, size_t count) {
    if (*p) { (void)hipFree(*p); *p = nullptr; }
    if (count) HIPCHK(h, hipMalloc((void**)p, count * sizeof(T)));
    return 0;
}

static int ensure_cap(bmpc_handle* h, int B, bool want_g) {
    if (B <= h->cap && (!want_g || h->cap_g)) return 0;
    int cap = B > h->cap ? B : h->cap;
    if (h->o.max_batch > cap) cap = h->o.max_batch;
    const size_t c = (size_t)cap;
    for (double** b : {&h->d_x0, &h->d_lbx, &h->d_ubx, &h->d_x}) if (int r = dev_realloc(h, b, c * h->n_w)) return r;
    if (int r = dev_realloc(h, &h->d_p, c * NPAR)) return r;
    for (double** b : {&h->d_f, &h->d_viol}) if (int r = dev_realloc(h, b, c)) return r;
    for (int** b : {&h->d_iters, &h->d_status}) if (int r = dev_realloc(h, b, c)) return r;
    h->cap_g = false;
    if (int r = dev_realloc(h, &h->d_g, want_g ? c * h->n_g : 0)) return r;
    h->cap_g = want_g;
    h->cap = cap;
    return 0;
}

extern "C" int bmpc_solve(bmpc_handle* h, int B, const double* x0, const double* lbx, const double* ubx,
                          const double* p, double* x, double* g, double* lam_g, double* lam_x, double* f,
                          int* iters, int* status, double* viol) {
    if (!h || B < 0 || !x0 || !lbx || !ubx || !p || !x || !f || !iters || !status || !viol) {
        if (h) h->err = "bmpc_solve: null argument";
        return 1;
    }
    if (B == 0) return 0;
    WEDGED_FAIL(h);                // (before ensure_cap below, whose hipFree would wait for a stream that never drains)
    int rc = bmpc_wait(h);         // an asynchronous solve in flight owns the workspace
    if (rc) return rc;
    BUSY_OR_FAIL(h, "bmpc_solve");
    // multipliers need every instance's final iterate in its own workspace slot: refused up front (not after the solve) when the
    // call would stream through a smaller pool
    if ((lam_g || lam_x) && h->o.pool_slots > 0 && B > h->o.pool_slots) {
        h->err = "bmpc_solve: lam_g / lam_x need B <= pool_slots (a streamed call keeps no final iterates)";
        return 1;
    }
    HIPCHK(h, hipSetDevice(h->o.device));
    rc = ensure_cap(h, B, g != nullptr);
    if (rc) return rc;
    size_t nw = (size_t)B * h->n_w * sizeof(double);
    hipStream_t st = h->stream;
    HIPCHK(h, hipMemcpyAsync(h->d_x0, x0, nw, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->d_lbx, lbx, nw, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->d_ubx, ubx, nw, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->d_p, p, (size_t)B * NPAR * sizeof(double), hipMemcpyHostToDevice, st));
    rc = pipe_solve(h, B, h->d_x0, h->d_lbx, h->d_ubx, h->d_p, h->d_x, g ? h->d_g : nullptr, h->d_f, h->d_iters,
                    h->d_status, h->d_viol, st);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(x, h->d_x, nw, hipMemcpyDeviceToHost, st));
    if (g) HIPCHK(h, hipMemcpyAsync(g, h->d_g, (size_t)B * h->n_g * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(f, h->d_f, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(viol, h->d_viol, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(iters, h->d_iters, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(status, h->d_status, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    if (int r = wait_stream(h, st)) return r;
    HIPCHK(h, hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
    if (lam_g || lam_x) {
        if (B > h->cap_lam) {
            h->cap_lam = 0;
            if (int r = dev_realloc(h, &h->d_lam_g, (size_t)B * h->n_g)) return r;
            if (int r = dev_realloc(h, &h->d_lam_x, (size_t)B * h->n_w)) return r;
            h->cap_lam = B;
        }
        rc = bmpc_multipliers_dev(h, B, h->d_lam_g, h->d_lam_x, st);
        if (rc) return rc;
        if (lam_g) HIPCHK(h, hipMemcpy(lam_g, h->d_lam_g, (size_t)B * h->n_g * sizeof(double), hipMemcpyDeviceToHost));
        if (lam_x) HIPCHK(h, hipMemcpy(lam_x, h->d_lam_x, (size_t)B * h->n_w * sizeof(double), hipMemcpyDeviceToHost));
    }
    return 0;
}

extern "C" int bmpc_last_kernel_ms(bmpc_handle* h, float* ms) {
    if (!h || !ms) return 1;
    float t = 0.f;
    if (hipEventElapsedTime(&t, h->ev0, h->ev1) == hipSuccess) h->last_ms = t;
    *ms = h->last_ms;
    return 0;
}

// diagnostic: per-phase cycle sums accumulated by a -DBMPC_PROFILE build (zeros otherwise)
extern "C" int bmpc_debug_phase_cycles(bmpc_handle* h, double* out16) {
    if (!h || !out16) return 1;
    std::vector<double> buf((size_t)h->nblocks_max * 16);
    HIPCHK(h, hipMemcpy(buf.data(), h->d_prof, buf.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < 16; i++) out16[i] = 0;
    for (int b = 0; b < h->nblocks_max; b++) for (int i = 0; i < 16; i++) out16[i] += buf[(size_t)b * 16 + i];
    HIPCHK(h, hipMemset(h->d_prof, 0, buf.size() * sizeof(double)));
    return 0;
}

// diagnostic: per-instance solver state the most recent finished solve left in the workspace, row by row (out [B][12], host):
// {iterations, status, mu, alpha (1e300: the line search found no acceptable step), alpha_dual, fraction-to-boundary alpha, delta_w,
//  exact Hessian wanted next, factorisation retries, rejected trials, KKT error of the previous iterate, stall counter} -- with
// max_iter = k these are the decisions of iteration k - 1 (tests/test_iterate_parity.py compares them with the oracle's).  Needs
// a solve that kept every instance in a slot of its own (B <= slots).
extern "C" int bmpc_debug_inst_state(bmpc_handle* h, int B, double* out) {
    if (!h || !out) { if (h) h->err = "bmpc_debug_inst_state: null argument"; return 1; }
    int rc = bmpc_wait(h);
    if (rc) return rc;
    WEDGED_FAIL(h);
    if (!h->last_valid || h->last_args.B != B || B > h->pipe_cap || (h->o.pool_slots > 0 && B > h->o.pool_slots)) {
        h->err = "bmpc_debug_inst_state: no finished solve of this batch size with a slot per instance on the handle"; return 1;
    }
    HIPCHK(h, hipSetDevice(h->o.device));
    std::vector<InstState> st((size_t)B);
    std::vector<int> src((size_t)B);
    HIPCHK(h, hipMemcpy(st.data(), h->d_pipe_st, st.size() * sizeof(InstState), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(src.data(), h->last_args.src, src.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int s = 0; s < B; s++) {
        const InstState& t = st[(size_t)s];
        const int row = src[(size_t)s];
        if (row < 0 || row >= B) { h->err = "bmpc_debug_inst_state: slot map out of range"; return 1; }
        double* o = out + (size_t)row * 12;
        o[0] = t.it; o[1] = t.status; o[2] = t.mu; o[3] = t.alpha; o[4] = t.ad; o[5] = t.ap; o[6] = t.hreg; o[7] = t.hess_mode;
        o[8] = t.tries; o[9] = t.bt; o[10] = t.err_prev; o[11] = t.stall;
    }
    return 0;
}

// The test entry (include/boundmpc.h): one super-step from a planted state, stopped where the requested outputs say.  Host pointers;
// the call owns the handle's workspace and stream and waits for the result.
extern "C" int bmpc_debug_superstep(bmpc_handle* h, int B, const bmpc_debug_step* s) {
    auto refuse = [&](const char* why) { h->err = std::string("bmpc_debug_superstep: ") + why; return 1; };
    if (!h) return 1;
    if (const char* why = bmpc_debug_step_refusal(B, s)) return refuse(why);
    if (s->ls && h->o.trial_repeats < 9) return refuse("needs a handle whose line search ends inside one launch (trial_repeats >= 9)");
    int rc = bmpc_wait(h);
    if (rc) return rc;
    BUSY_OR_FAIL(h, "bmpc_debug_superstep");
    WEDGED_FAIL(h);
    HIPCHK(h, hipSetDevice(h->o.device));
    if (h->o.hess != 2) return refuse("needs a handle with the exact Hessian (hess = 2)");
    if ((rc = pipe_ensure(h, B))) return rc;
    if (B > h->pipe_cap) return refuse("more instances than workspace slots");
    int np0 = 0, np1 = 0, nls = 0, npc = 0, nctl = 0;
    bmpc_pipe_ls_sizes(&np0, &np1, &nls);
    bmpc_pipe_ctl_sizes(&npc, &nctl);
    const size_t N = (size_t)h->o.N, n_w = 44 * N + 6, rows = B * (N - 1) * NSLOT, nz = B * (N - 1) * NZ;
    bmpc_debug_step d = *s;                                  // the record with device pointers, once run() has staged it
    double *x = nullptr, *f = nullptr, *viol = nullptr;      // of the argument block: never written here
    int *iters = nullptr, *status = nullptr;
    Staging g;
    g.in(&d.x0, B * n_w); g.in(&d.lbx, B * n_w); g.in(&d.ubx, B * n_w); g.in(&d.p, (size_t)B * NPAR);
    g.in(&d.t, rows); g.in(&d.z, rows); g.in(&d.mode, (size_t)B);
    g.in(&d.plant0, (size_t)B * np0); g.in(&d.plant1, (size_t)B * np1); g.in(&d.ctl_plant, (size_t)B * npc); g.in(&d.lam_pi, B * N * 3);
    g.out(&d.H, nz * NZ);
    g.out(&d.dzeta, nz); g.out(&d.dt, rows); g.out(&d.dz, rows); g.out(&d.state, (size_t)B * 12);
    g.out(&d.zeta0, nz); g.out(&d.t0, rows); g.out(&d.z0, rows); g.out(&d.zeta1, nz); g.out(&d.t1, rows); g.out(&d.z1, rows);
    g.out(&d.ls, (size_t)B * nls); g.out(&d.ctl, (size_t)B * nctl);
    g.scratch(&x, B * n_w); g.scratch(&f, (size_t)B); g.scratch(&viol, (size_t)B); g.scratch(&iters, (size_t)B); g.scratch(&status, (size_t)B);
    const hipStream_t st = h->stream;
    return g.run(h, st, [&]() -> int {
        PipeArgsH A = pipe_args(h, B);
        A.x0 = d.x0; A.lbx = d.lbx; A.ubx = d.ubx; A.p = d.p;
        A.x = x; A.f = f; A.viol = viol; A.g = nullptr; A.iters = iters; A.status = status;
        if (int r = pipe_seed(h, A, B, st)) return r;
        HIPCHK(h, bmpc_pipe_launch_superstep(&A, &d, st));
        return 0;
    });
}

// diagnostic / measurement: HIP events around every launch of the Riccati kernel (bmpc_k_ric: the throughput variant, bmpc_k_ric_lat:
// the latency variant of nearly empty super-steps) on the handle's stream, from the next solve on.  bmpc_debug_ric_stats returns, for
// the most recent solve, out[0..2] = {summed launch durations in ms, launches, instance-iterations (workgroups that ran)} of
// bmpc_k_ric and out[3..5] the same for bmpc_k_ric_lat.  bench.py's roofline leg: algorithmic flops of the launches / their duration.
extern "C" int bmpc_debug_time_ric(bmpc_handle* h, int on) {
    if (!h) return 1;
    int rc = bmpc_wait(h);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->o.device));
    if (on && !h->ric_ev[0]) for (auto& e : h->ric_ev) HIPCHK(h, hipEventCreate(&e));
    h->time_ric = on != 0;
    return 0;
}
extern "C" int bmpc_debug_ric_stats(bmpc_handle* h, double* out6) {
    if (!h || !out6) return 1;
    int rc = bmpc_wait(h);
    if (rc) return rc;
    for (int v = 0; v < 2; v++) { out6[3 * v] = h->ric_ms[v]; out6[3 * v + 1] = (double)h->ric_launches[v]; out6[3 * v + 2] = (double)h->ric_sweeps[v]; }
    return 0;
}

extern "C" int bmpc_debug_ric_stats_full(bmpc_handle* h, double* out3) {
    if (!h || !out3) return 1;
    int rc = bmpc_wait(h);
    if (rc) return rc;
    for (int i = 0; i < 3; i++) out3[i] = h->ric_full[i];
    return 0;
}

// diagnostic: keep the handle's stream busy for `ms` milliseconds (at most 10 s) -- lets a test exercise the watchdog
extern "C" int bmpc_debug_spin(bmpc_handle* h, int ms) {
    if (!h) return 1;
    WEDGED_FAIL(h);
    HIPCHK(h, hipSetDevice(h->o.device));
    HIPCHK(h, bmpc_launch_spin(ms, h->stream));
    return 0;
}
