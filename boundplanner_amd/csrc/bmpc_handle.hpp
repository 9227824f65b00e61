// The handle behind include/boundmpc.h and what every entry point does with it: error capture (HIPCHK), the bounded wait for a
// stream (wait_stream), the refusal of a handle that ran into its watchdog (WEDGED_FAIL) and of a second concurrent call
// (BusyGuard).  Shared by the files that implement the C ABI (bmpc_capi.hip, bmpc_capi_batch.hip); BMPC_NT is defined by them.
#pragma once
#include "bmpc_internal.hpp"
#include "bmpc_pipeline.hpp"
#include "bmpc_robot.hpp"

#include <atomic>
#include <cstdlib>
#include <string>
#include <thread>

#include "../../include/boundmpc.h"

struct bmpc_handle {
    bmpc_opts o;
    int n_w, n_g, n_cu, nblocks_max;
    bmpc::RobotConst* d_rc = nullptr;
    bmpc_robot robot;              // host copy of the robot table behind d_rc
    double* d_prof = nullptr;   // diagnostic builds only
    // workspace (grown on demand to the largest batch seen)
    int pipe_cap = 0;
    // workspace layout (pipe_carve): slot-major; BMPC_LAYOUT=0 in the environment selects the field-major layout of round 1 (A/B runs)
    int slot_major = env_int("BMPC_LAYOUT", 1);
    double* d_pipe = nullptr;      // one slab: SoA iterate/row arrays, stage records, gains, partials
    void* d_pipe_st = nullptr;     // InstState[cap]
    int* d_pipe_lists = nullptr;   // 8 lists + the slot -> row map of cap ints each + NCNT counters
    int* d_pipe_tbl = nullptr;     // scatter table of the stage record
    int* h_cnt = nullptr;          // pinned host copy of the NCNT counters
    int cnt_seed[bmpc::NCNT] = {0};   // source of the counter upload that seeds the pool (pipe_seed): outlives the enqueued copy
    int last_steps = 0;
    bmpc::PipeArgsH last_args;           // arguments of the most recent pipeline solve (its final iterate stays in the workspace)
    bool last_valid = false;
    double *d_lam_g = nullptr, *d_lam_x = nullptr;   // staging of the multipliers for the host-pointer entry
    int cap_lam = 0;
    // asynchronous solves: one in flight per handle, driven by a worker thread on the handle's stream
    std::thread worker;
    int worker_rc = 0;
    std::atomic<int> n_active{0};  // unfinished instances of the solve in flight (updated at every readback)
    // staging for the host-pointer entry
    double *d_x0 = nullptr, *d_lbx = nullptr, *d_ubx = nullptr, *d_p = nullptr, *d_x = nullptr, *d_g = nullptr,
           *d_f = nullptr, *d_viol = nullptr;
    int *d_iters = nullptr, *d_status = nullptr;
    int cap = 0;
    bool cap_g = false;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_wait = nullptr;
    // bmpc_debug_time_ric: HIP events around every launch of the Riccati kernel (the dominant kernel: bench.py's roofline leg)
    bool time_ric = false;
    hipEvent_t ric_ev[16] = {nullptr};      // 8 pairs: a burst has at most 8 super-steps and ends with a wait for the stream
    int ric_pending = 0, ric_is_lat[8] = {0}, ric_nact[8] = {0};
    int ric_full_n = 0;                     // grid size that counts as "the whole batch" (the first burst of a solve)
    double ric_full[3] = {0, 0, 0};         // launches of bmpc_k_ric over the whole batch: summed duration [ms], launches, instance-iterations
    double ric_ms[2] = {0, 0};              // [0] bmpc_k_ric, [1] bmpc_k_ric_lat: summed launch durations of the last solve
    long ric_launches[2] = {0, 0}, ric_sweeps[2] = {0, 0};
    bool wedged = false;           // a wait ran into the watchdog: the stream may still be busy, the handle refuses further work
    float last_ms = 0.f;
    std::atomic<bool> busy{false}; // a solve is running on this handle (a handle serves one host thread at a time)
    std::atomic<int> n_loops{0};   // device loops borrowing this handle (bmpc_loop_create / bmpc_loop_destroy)
    bool destroy_pending = false;  // bmpc_destroy called while loops were alive: the last loop frees the handle
    std::string err;
};

#define HIPCHK(h, call)                                                                   \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                 \
            return 2;                                                                     \
        }                                                                                 \
    } while (0)

// Wait for everything enqueued on `st` so far.  With bmpc_opts.watchdog_ms > 0 the wait polls an event and gives up after that
// long: a kernel that does not return then costs the caller an error code -- rc 5, bmpc_last_error() --
// instead of a host thread stuck in hipStreamSynchronize for ever.  The handle is unusable afterwards (its stream may never
// drain): destroy it, or end the process when it does not come back.
__attribute__((visibility("hidden"))) int wait_stream(bmpc_handle* h, hipStream_t st);      // bmpc_capi.hip
#define WEDGED_FAIL(h) if ((h)->wedged) { (h)->err = "the handle ran into its watchdog earlier and is unusable"; return 5; }

// one solve at a time per handle: a second host thread entering gets an error instead of a corrupted workspace
struct BusyGuard {
    bmpc_handle* h; bool ok;
    explicit BusyGuard(bmpc_handle* h_) : h(h_) { bool f = false; ok = h->busy.compare_exchange_strong(f, true); }
    ~BusyGuard() { if (ok) h->busy.store(false); }
};
#define BUSY_OR_FAIL(h, what)                                                                                   \
    BusyGuard busy_guard_(h);                                                                                   \
    if (!busy_guard_.ok) return 4;       /* (h->err belongs to the thread that owns the handle: not touched) */
