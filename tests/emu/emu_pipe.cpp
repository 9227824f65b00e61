// CPU thread emulation of the batch-synchronous HIP pipeline -- TEST INFRASTRUCTURE ONLY.
// Compiles the identical device source (bmpc_stage.hpp, bmpc_pair_kernels.hpp,
// bmpc_ric_kernel.hpp) with 64 std::threads standing in for the 64 lanes of a wavefront and a
// barrier for __syncthreads(); workgroups run one after the other.  Lets the kernel logic be
// debugged against the oracle without a GPU.  Never shipped, never used by the product path.
#include <barrier>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

// this build's own platform names (defined before emu_platform.hpp, which keeps them): the lanes of a workgroup are threads, so
// the barriers and the lane index are real, the counter increment is atomic, and the Riccati kernel's trace hooks are compiled in
static std::barrier<>* g_bar = nullptr;
static thread_local int t_lane = 0;
#define BMPC_EMU_TRACE 1
#define BMPC_SYNC() g_bar->arrive_and_wait()
#define BMPC_FENCE_SYNC() g_bar->arrive_and_wait()
#define BMPC_LANE() t_lane
#define BMPC_ATOMIC_INC(ptr) __atomic_fetch_add((ptr), 1, __ATOMIC_RELAXED)
#include "emu_platform.hpp"

#include "../../boundplanner_amd/csrc/bmpc_pair_kernels.hpp"
#include "../../boundplanner_amd/csrc/bmpc_ric_kernel.hpp"
#include "../../boundplanner_amd/csrc/bmpc_stage_matrix.hpp"
#include "../../boundplanner_amd/csrc/bmpc_robot.hpp"

using namespace bmpc;
#ifndef EMU_TRIAL_NW
#define EMU_TRIAL_NW 1
#endif
#ifndef EMU_RIC_NT
#define EMU_RIC_NT 128
#endif

template <class F> static void launch(int nblocks, F body, int nt = 64) {
    if (nblocks <= 0) return;
    std::barrier<> bar(nt);
    g_bar = &bar;
    std::vector<std::thread> th;
    for (int l = 0; l < nt; l++)
        th.emplace_back([&, l] {
            t_lane = l;
            // workgroups run one after the other on the same LDS buffer: nobody starts the next one's LDS writes
            // while a slower lane still reads this one's
            for (int blk = 0; blk < nblocks; blk++) { body(blk, l); bar.arrive_and_wait(); }
        });
    for (auto& t : th) t.join();
}

static bool env_on(const char* name) { const char* e = getenv(name); return e && atoi(e); }      // read at call time: the tests set the knobs with monkeypatch
// bmpc_default_opts, for the two test entries
static SolverOpts default_opts(int N, double dt) { return SolverOpts{N, dt, 1e-5, 100, 2, 1.0, 0.1, 0.1, 2.0, 1000.0, 1e4, 1e-4, 1e-2, 0.0, 2, 8, 2, 1, 9}; }

// Everything a run of the kernel bodies needs beside the caller's arrays -- workspace, instance state, lists, counters, scatter table,
// LDS buffer -- with a PipeArgs wired to it, and the launch sequences of bmpc_pipeline.hip (bmpc_pipe_launch_init, launch_eval,
// launch_direction) as members.  A points into the rig: it is neither copied nor moved.
struct Rig {
    const int N, cap;           // pool of `cap` slots
    const int nb_inst, nw;      // grids over all slots: threads per instance / groups of pairs
    RobotConst rc;
    PipeArgs A;                 // emulation: BMPC_AS1 is empty, host and device views coincide
    std::vector<double> work, lds, xo, fo, vo;
    std::vector<InstState> st;
    std::vector<int> list[9], cnt, tbl, ito, sto;

    Rig(int B, int cap_, int slot_major, const SolverOpts& o, const double* x0, const double* lbx, const double* ubx, const double* p)
        : N(o.N), cap(cap_), nb_inst((cap_ + 63) / 64), nw(waves_for(o.N, cap_)), work(pipe_workspace_doubles(cap_, o.N, slot_major)),
          lds(std::max<size_t>(std::max<size_t>(pair_lds_doubles(o.N, true), trial_lds_doubles(o.N, 4)), RIC_LDS_DOUBLES) + 64),
          st(cap_), cnt(NCNT, 0), tbl(3 * HREC) {
        fill_robot_const(rc);
        A.B = B; A.N = N; A.natt = 0; A.pad0_ = 0;
        A.lam_g = nullptr; A.lam_x = nullptr; A.cont = nullptr;
        A.o = o;
        A.rc = &rc;
        A.x0 = x0; A.lbx = lbx; A.ubx = ubx; A.p = p;
        pipe_carve(A, work.data(), cap, N, slot_major);
        for (auto& v : list) v.resize(cap);
        build_scatter_table(tbl.data());
        A.st = st.data();
        A.L.eval = list[0].data(); A.L.step = list[1].data(); A.L.trial = list[2].data();
        A.L.eval_next = list[3].data(); A.L.trial_next = list[4].data(); A.L.cnt = cnt.data();
        A.L.done = list[5].data(); A.L.admit = list[6].data(); A.L.curv = list[7].data(); A.src = list[8].data();
        A.tbl = tbl.data();
    }
    Rig(const Rig&) = delete;
    Rig& operator=(const Rig&) = delete;

    // the argument block's outputs of a test entry that has none of its own: x, f, viol, iters, status of B rows (never read)
    void own_outputs() {
        xo.resize((size_t)A.B * (44 * N + 6)); fo.resize(A.B); vo.resize(A.B); ito.resize(A.B); sto.resize(A.B);
        A.x = xo.data(); A.f = fo.data(); A.viol = vo.data(); A.g = nullptr; A.iters = ito.data(); A.status = sto.data();
    }
    // bmpc_pipe_launch_init: every slot takes an input row
    void init() {
        cnt[0] = cap; cnt[6] = cap; cnt[9] = cap;
        launch(nb_inst, [&](int blk, int l) { k_init_inst_body(A, blk * 64 + l); });
        launch(nw, [&](int blk, int l) { k_init_body(A, blk, l, lds.data()); });
        launch(nb_inst, [&](int blk, int l) { k_init_fin_body(A, blk * 64 + l); });
        k_pool_reset_body(A, false);
    }
    // (the test entries) rows, and with `mode` the first attempt's Hessian mode, written over the initial ones
    size_t nset() const { return (size_t)A.B * (N - 1) * NSLOT; }
    void set_rows(const double* t, const double* z, const int* mode = nullptr) {
        launch((int)((nset() + 63) / 64), [&](int blk, int l) { k_set_rows_body(A, (size_t)blk * 64 + l, t, z, mode); });
    }
    // launch_eval for n groups of pairs: k_points, k_pose, k_eval (split: the two-wavefront pair of the tail regime on the GPU), then
    // k_curv for the curvature list -- which must have n_curv entries if that is given (false, k_curv not run, otherwise)
    bool eval(int n, bool split, int n_curv = -1) {
        launch(n, [&](int blk, int l) { k_points_body(A, blk, l, lds.data()); });
        launch(n, [&](int blk, int l) { k_pose_body(A, blk, l, lds.data()); });
        if (split) {
            launch(n, [&](int blk, int l) { k_eval_body<2>(A, blk, l, lds.data()); });
            launch(n, [&](int blk, int l) { k_eval_body<1>(A, blk, l, lds.data()); });
        } else
            launch(n, [&](int blk, int l) { k_eval_body<0>(A, blk, l, lds.data()); });
        if (n_curv >= 0 && cnt[10] != n_curv) return false;
        launch(waves_for(N, cnt[10]), [&](int blk, int l) { k_curv_body(A, blk, l, lds.data()); });
        return true;
    }
    // launch_direction: the Riccati body (spec: the speculative pair with three attempts, the deep tail's kernels on the GPU), k_fwd, k_step
    void direction(bool spec) {
        const PipeArgsH& AH = *reinterpret_cast<const PipeArgsH*>(&A);
        if (spec) {
            A.natt = 3;
            launch(cnt[0] * A.natt, [&](int blk, int l) { k_ric_att_body<EMU_RIC_NT, false>(AH, blk, l, lds.data()); }, EMU_RIC_NT);
            launch(cnt[0], [&](int blk, int l) { k_ric_body<EMU_RIC_NT, false, true>(AH, blk, l, lds.data()); }, EMU_RIC_NT);
        } else
            launch(cnt[0], [&](int blk, int l) { k_ric_body<EMU_RIC_NT>(AH, blk, l, lds.data()); }, EMU_RIC_NT);
        launch(cnt[1], [&](int blk, int l) { k_fwd_body(A, blk, l, lds.data()); });
        launch(waves_for(N, cnt[1]), [&](int blk, int l) { k_step_body(A, blk, l, lds.data()); });
    }
    // launch_trial: the line search of the trial list (spec: k_trial_spec_body, the tail regime's kernel on the GPU; slot-major layout)
    void trial(bool spec) {
        if (spec) launch(waves_for(N, cnt[2]), [&](int blk, int l) { k_trial_spec_body(A, blk, l, lds.data()); }, 64 * TRIAL_SPEC);
        else launch(waves_for(N, cnt[2]), [&](int blk, int l) { k_trial_body_t<EMU_TRIAL_NW>(A, blk, l, lds.data()); }, 64 * EMU_TRIAL_NW);
    }
};

extern "C" int emu_pipe_solve(int N, double dt, double tol, int max_iter, int hess, double hess_switch, double mu_init,
                              double kappa_mu, double theta_mu, double kappa_eps, int B, const double* x0,
                              const double* lbx, const double* ubx, const double* p, double* x, double* g, double* f,
                              int* iters, int* status, double* viol, int verbose, double* lam_g, double* lam_x, int slots,
                              double mu_floor_k, double dw0, double inertia_err, int inertia, int stall_n, int gn_backoff, int slack_reset, double ls_alpha_mem, int trial_repeats) {
    const int cap = (slots > 0 && slots < B) ? slots : B;       // pool of `cap` slots: B > cap streams through it
    const char* lay = getenv("BMPC_LAYOUT");
    const int slot_major = lay ? atoi(lay) : 1;
    Rig R(B, cap, slot_major, SolverOpts{N, dt, tol, max_iter, hess, hess_switch, mu_init, kappa_mu, theta_mu, kappa_eps, mu_floor_k, dw0, inertia_err, ls_alpha_mem, inertia, stall_n, gn_backoff, slack_reset, trial_repeats},
          x0, lbx, ubx, p);
    PipeArgs& A = R.A;
    std::vector<int>& cnt = R.cnt;
    double* const lds = R.lds.data();
    A.x = x; A.f = f; A.viol = viol; A.g = g; A.iters = iters; A.status = status;
    R.init();
    auto retire = [&]() {        // bmpc_pipe_launch_retire
        launch(waves_for(N, cnt[8]), [&](int blk, int l) { k_out_body(A, blk, l, lds); });
        launch((cnt[8] + 63) / 64, [&](int blk, int l) { k_fin_body(A, blk * 64 + l); });
        launch((cnt[8] + 63) / 64, [&](int blk, int l) { k_admit_body(A, blk * 64 + l); });
        launch(waves_for(N, cnt[9]), [&](int blk, int l) { k_init_body(A, blk, l, lds); });
        launch((cnt[9] + 63) / 64, [&](int blk, int l) { k_init_fin_body(A, blk * 64 + l); });
        k_pool_reset_body(A, true);
    };
    int steps = 0;
    for (; steps < 12 * (max_iter + 2) * ((B + cap - 1) / cap + 1); steps++) {
        retire();
        if (cnt[7] >= B) break;
        if (verbose) printf("step %d: n_eval %d n_trial %d finished %d retired %d next row %d\n", steps, cnt[0], cnt[2], cnt[5], cnt[7], cnt[6]);
        R.eval(waves_for(N, cnt[0]), env_on("BMPC_EMU_EVAL_SPLIT"));
        R.direction(env_on("BMPC_EMU_RIC_SPEC"));
        R.trial(env_on("BMPC_EMU_TRIAL_SPEC") && slot_major);      // (the tail regime's line search on the GPU)
        k_rotate_body(A);
        std::swap(A.L.eval, A.L.eval_next);
        std::swap(A.L.trial, A.L.trial_next);
    }
    if (lam_g && lam_x) {
        A.lam_g = lam_g; A.lam_x = lam_x;
        launch(R.nw, [&](int blk, int l) { k_mult_body(A, blk, l, lds); });
        launch(R.nb_inst, [&](int blk, int l) { k_mult_sweep_body(A, blk * 64 + l); });
    }
    return steps;
}

// The stage matrices the Riccati sweep factorises, at a GIVEN point with GIVEN row slacks / multipliers and adjoint multipliers of
// the pi dynamics (tests/test_hessian_pin.py): the slots are initialised by the k_init* bodies from x0 = w, then t, z
// ([B][N-1][NSLOT], slot numbering of bmpc_device.hpp) and hess_mode = 1 are written over the initial ones; k_points, k_pose,
// k_eval (split = 0: k_eval_body<0>; 1: the two-wavefront pair <2> + <1>) and k_curv run once; then ric_phase_load_impl<128> runs
// per (instance, stage) with lam_pi[b][k + 1] in R_lam and the stage matrix it leaves in LDS (zeta coordinates) is copied to
// H [B][N-1][41][41] (k_set_rows_body, k_stage_matrix_body: bmpc_stage_matrix.hpp, the bodies of bmpc_debug_stage_matrices).
extern "C" int emu_stage_matrices(int N, double dt, int B, const double* w, const double* lbx, const double* ubx, const double* p,
                                  const double* t, const double* z, const double* lam_pi, int split, double* H) {
    Rig R(B, B, 1, default_opts(N, dt), w, lbx, ubx, p);
    R.own_outputs();
    R.init();
    R.set_rows(t, z);
    if (!R.eval(R.nw, split != 0, B)) return -1;            // every instance is in the curvature list
    launch(B, [&](int b, int lane) {
        k_stage_matrix_body<EMU_RIC_NT>(*reinterpret_cast<const PipeArgsH*>(&R.A), b, lane, R.lds.data(), lam_pi, H);
    }, EMU_RIC_NT);
    return 0;
}

// The Newton step of one super-step from a given state (tests/test_newton_step.py; the bodies of bmpc_debug_newton_step): slots
// initialised by the k_init* bodies from x0 = w, rows and the first attempt's Hessian mode written over them (k_set_rows_body), then
// k_points, k_pose, k_eval, k_curv, the Riccati body (variant 0: k_ric_body, the kernels bmpc_k_ric / bmpc_k_ric_lat; 1: the
// speculative pair k_ric_att_body + k_ric_body<RESUME> with three attempts), k_fwd, k_step, and the copy-out k_newton_out_body.
extern "C" int emu_newton_step(int N, double dt_, int B, const double* w, const double* lbx, const double* ubx, const double* p,
                               const double* t, const double* z, const int* mode, int variant, double* dzeta, double* dt, double* dz,
                               double* state) {
    Rig R(B, B, 1, default_opts(N, dt_), w, lbx, ubx, p);
    R.own_outputs();
    R.init();
    R.set_rows(t, z, mode);
    R.eval(R.nw, false);
    R.direction(variant == 1);
    launch((int)((R.nset() + 63) / 64), [&](int blk, int l) { k_newton_out_body(R.A, (size_t)blk * 64 + l, dzeta, dt, dz, state); });
    return 0;
}

// Newton step and filter line search of one super-step from a given state (tests/test_line_search.py; the bodies of
// bmpc_debug_line_search): emu_newton_step's sequence -- rows and mode overwritten only when t is given --, line-search state planted
// before the evaluation bodies (plant0, with a NaN in the copies the trial writes when rows are given) and after k_step (plant1)
// (k_ls_plant_body; null = nothing), the copy-out of the Newton step, then the trial body ONCE (variant 0: k_trial_body, the kernel
// bmpc_k_trial; 1: k_trial_spec_body, bmpc_k_trial_spec) with the default trial_repeats -- the search ends inside it --, no
// k_rotate, and the copy-out k_ls_out_body.
extern "C" int emu_line_search(int N, double dt_, int B, const double* w, const double* lbx, const double* ubx, const double* p,
                               const double* t, const double* z, const int* mode, const double* plant0, const double* plant1,
                               int variant, double* dzeta, double* dt, double* dz, double* state, double* zeta0, double* t0, double* z0,
                               double* zeta1, double* t1, double* z1, double* ls) {
    if ((t == nullptr) != (z == nullptr) || (t == nullptr) != (mode == nullptr) || (!t && (plant0 || plant1))) return 1;
    Rig R(B, B, 1, default_opts(N, dt_), w, lbx, ubx, p);
    R.own_outputs();
    R.init();
    const int nb = (int)((R.nset() + 63) / 64);
    if (t) R.set_rows(t, z, mode);
    if (t || plant0) launch(nb, [&](int blk, int l) { k_ls_plant_body(R.A, (size_t)blk * 64 + l, plant0, 0, t ? 1 : 0); });
    R.eval(R.nw, false);
    R.direction(false);
    launch(nb, [&](int blk, int l) { k_newton_out_body(R.A, (size_t)blk * 64 + l, dzeta, dt, dz, state); });
    if (plant1) launch(nb, [&](int blk, int l) { k_ls_plant_body(R.A, (size_t)blk * 64 + l, plant1, 1, 0); });
    R.trial(variant == 1);
    launch(nb, [&](int blk, int l) { k_ls_out_body(R.A, (size_t)blk * 64 + l, zeta0, t0, z0, zeta1, t1, z1, ls); });
    return 0;
}

// The iteration control of one super-step from a given state (tests/test_iteration_control.py; the bodies of
// bmpc_debug_iteration_control): emu_line_search's sequence with the given tol, max_iter, mu_floor_k and dw0, the iteration-control state planted
// after the rows (k_ctl_plant_body; null = nothing) and copied out after k_step and after the trial body (k_ctl_out_body).
// ric_variant 0: k_ric_body; 1: the speculative pair k_ric_att_body + k_ric_body<RESUME> with three attempts.  The trial body is
// k_trial_spec_body.
extern "C" int emu_iteration_control(int N, double dt_, double tol, int max_iter, double mu_floor_k, double dw0, int B, const double* w, const double* lbx, const double* ubx,
                                     const double* p, const double* t, const double* z, const int* mode, const double* plant0,
                                     const double* plant1, const double* ctl_plant, int ric_variant, double* dzeta, double* dt, double* dz,
                                     double* state, double* zeta0, double* t0, double* z0, double* zeta1, double* t1, double* z1, double* ls,
                                     double* ctl) {
    if (!t || !z || !mode) return 1;
    SolverOpts o = default_opts(N, dt_);
    o.tol = tol; o.max_iter = max_iter; o.mu_floor_k = mu_floor_k; o.dw0 = dw0;
    Rig R(B, B, 1, o, w, lbx, ubx, p);
    R.own_outputs();
    R.init();
    const int nb = (int)((R.nset() + 63) / 64), nbi = (B + 63) / 64;
    R.set_rows(t, z, mode);
    launch(nb, [&](int blk, int l) { k_ls_plant_body(R.A, (size_t)blk * 64 + l, plant0, 0, 1); });
    if (ctl_plant) launch(nbi, [&](int blk, int l) { k_ctl_plant_body(R.A, (size_t)blk * 64 + l, ctl_plant); });
    R.eval(R.nw, false);
    R.direction(ric_variant == 1);
    launch(nb, [&](int blk, int l) { k_newton_out_body(R.A, (size_t)blk * 64 + l, dzeta, dt, dz, state); });
    launch(nbi, [&](int blk, int l) { k_ctl_out_body(R.A, (size_t)blk * 64 + l, ctl, 0); });
    if (plant1) launch(nb, [&](int blk, int l) { k_ls_plant_body(R.A, (size_t)blk * 64 + l, plant1, 1, 0); });
    R.trial(true);
    launch(nb, [&](int blk, int l) { k_ls_out_body(R.A, (size_t)blk * 64 + l, zeta0, t0, z0, zeta1, t1, z1, ls); });
    launch(nbi, [&](int blk, int l) { k_ctl_out_body(R.A, (size_t)blk * 64 + l, ctl, 1); });
    return 0;
}
