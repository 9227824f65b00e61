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

extern "C" int emu_pipe_solve(int N, double dt, double tol, int max_iter, int hess, double hess_switch, double mu_init,
                              double kappa_mu, double theta_mu, double kappa_eps, int B, const double* x0,
                              const double* lbx, const double* ubx, const double* p, double* x, double* g, double* f,
                              int* iters, int* status, double* viol, int verbose, double* lam_g, double* lam_x, int slots,
                              double mu_floor_k, double dw0, double inertia_err, int inertia, int stall_n, int gn_backoff, int slack_reset, double ls_alpha_mem, int trial_repeats) {
    RobotConst rc;
    fill_robot_const(rc);
    PipeArgs A;   // emulation: BMPC_AS1 is empty, host and device views coincide
    A.B = B; A.N = N; A.natt = 0; A.pad0_ = 0;
    A.lam_g = nullptr; A.lam_x = nullptr; A.cont = nullptr;
    A.o = SolverOpts{N, dt, tol, max_iter, hess, hess_switch, mu_init, kappa_mu, theta_mu, kappa_eps, mu_floor_k, dw0, inertia_err, ls_alpha_mem, inertia, stall_n, gn_backoff, slack_reset, trial_repeats};
    A.rc = &rc;
    A.x0 = x0; A.lbx = lbx; A.ubx = ubx; A.p = p;
    A.x = x; A.f = f; A.viol = viol; A.g = g; A.iters = iters; A.status = status;
    const int cap = (slots > 0 && slots < B) ? slots : B;       // pool of `cap` slots: B > cap streams through it
    const char* lay = getenv("BMPC_LAYOUT");
    const int slot_major = lay ? atoi(lay) : 1;
    std::vector<double> work(pipe_workspace_doubles(cap, N, slot_major));
    pipe_carve(A, work.data(), cap, N, slot_major);
    std::vector<InstState> st(cap);
    std::vector<int> l_eval(cap), l_step(cap), l_trial(cap), l_evn(cap), l_trn(cap), l_done(cap), l_admit(cap), l_curv(cap), srcv(cap), cnt(NCNT, 0), tbl(3 * HREC);
    build_scatter_table(tbl.data());
    A.st = st.data();
    A.L.eval = l_eval.data(); A.L.step = l_step.data(); A.L.trial = l_trial.data();
    A.L.eval_next = l_evn.data(); A.L.trial_next = l_trn.data(); A.L.cnt = cnt.data();
    A.L.done = l_done.data(); A.L.admit = l_admit.data(); A.L.curv = l_curv.data(); A.src = srcv.data();
    A.tbl = tbl.data();
    std::vector<double> lds(std::max<size_t>(std::max<size_t>(pair_lds_doubles(N, true), trial_lds_doubles(N, 4)), RIC_LDS_DOUBLES) + 64);
    const int n0 = cap;
    const int nb_inst = (cap + 63) / 64, nw = waves_for(N, cap);
    cnt[0] = n0; cnt[6] = n0; cnt[9] = n0;
    launch(nb_inst, [&](int blk, int l) { k_init_inst_body(A, blk * 64 + l); });
    launch(nw, [&](int blk, int l) { k_init_body(A, blk, l, lds.data()); });
    launch(nb_inst, [&](int blk, int l) { k_init_fin_body(A, blk * 64 + l); });
    k_pool_reset_body(A, false);
    auto retire = [&]() {        // bmpc_pipe_launch_retire
        launch(waves_for(N, cnt[8]), [&](int blk, int l) { k_out_body(A, blk, l, lds.data()); });
        launch((cnt[8] + 63) / 64, [&](int blk, int l) { k_fin_body(A, blk * 64 + l); });
        launch((cnt[8] + 63) / 64, [&](int blk, int l) { k_admit_body(A, blk * 64 + l); });
        launch(waves_for(N, cnt[9]), [&](int blk, int l) { k_init_body(A, blk, l, lds.data()); });
        launch((cnt[9] + 63) / 64, [&](int blk, int l) { k_init_fin_body(A, blk * 64 + l); });
        k_pool_reset_body(A, true);
    };
    int steps = 0;
    for (; steps < 12 * (max_iter + 2) * ((B + cap - 1) / cap + 1); steps++) {
        retire();
        if (cnt[7] >= B) break;
        if (verbose) printf("step %d: n_eval %d n_trial %d finished %d retired %d next row %d\n", steps, cnt[0], cnt[2], cnt[5], cnt[7], cnt[6]);
        launch(waves_for(N, cnt[0]), [&](int blk, int l) { k_points_body(A, blk, l, lds.data()); });
        launch(waves_for(N, cnt[0]), [&](int blk, int l) { k_pose_body(A, blk, l, lds.data()); });
        if (getenv("BMPC_EMU_EVAL_SPLIT") && atoi(getenv("BMPC_EMU_EVAL_SPLIT"))) {      // the tail regime's two-wavefront k_eval on the GPU
            launch(waves_for(N, cnt[0]), [&](int blk, int l) { k_eval_body<2>(A, blk, l, lds.data()); });
            launch(waves_for(N, cnt[0]), [&](int blk, int l) { k_eval_body<1>(A, blk, l, lds.data()); });
        } else
        launch(waves_for(N, cnt[0]), [&](int blk, int l) { k_eval_body<0>(A, blk, l, lds.data()); });
        launch(waves_for(N, cnt[10]), [&](int blk, int l) { k_curv_body(A, blk, l, lds.data()); });
        if (getenv("BMPC_EMU_RIC_SPEC") && atoi(getenv("BMPC_EMU_RIC_SPEC"))) {      // the speculative pair (the deep tail's kernels on the GPU)
            A.natt = 3;
            launch(cnt[0] * A.natt, [&](int blk, int l) { k_ric_att_body<EMU_RIC_NT, false>(*reinterpret_cast<const PipeArgsH*>(&A), blk, l, lds.data()); }, EMU_RIC_NT);
            launch(cnt[0], [&](int blk, int l) { k_ric_body<EMU_RIC_NT, false, true>(*reinterpret_cast<const PipeArgsH*>(&A), blk, l, lds.data()); }, EMU_RIC_NT);
        } else
        launch(cnt[0], [&](int blk, int l) { k_ric_body<EMU_RIC_NT>(*reinterpret_cast<const PipeArgsH*>(&A), blk, l, lds.data()); }, EMU_RIC_NT);
        launch(cnt[1], [&](int blk, int l) { k_fwd_body(A, blk, l, lds.data()); });
        launch(waves_for(N, cnt[1]), [&](int blk, int l) { k_step_body(A, blk, l, lds.data()); });
        if (getenv("BMPC_EMU_TRIAL_SPEC") && atoi(getenv("BMPC_EMU_TRIAL_SPEC")) && slot_major)      // the tail regime's line search on the GPU
            launch(waves_for(N, cnt[2]), [&](int blk, int l) { k_trial_spec_body(A, blk, l, lds.data()); }, 64 * TRIAL_SPEC);
        else
        launch(waves_for(N, cnt[2]), [&](int blk, int l) { k_trial_body_t<EMU_TRIAL_NW>(A, blk, l, lds.data()); }, 64 * EMU_TRIAL_NW);
        k_rotate_body(A);
        std::swap(A.L.eval, A.L.eval_next);
        std::swap(A.L.trial, A.L.trial_next);
    }
    if (lam_g && lam_x) {
        A.lam_g = lam_g; A.lam_x = lam_x;
        launch(nw, [&](int blk, int l) { k_mult_body(A, blk, l, lds.data()); });
        launch(nb_inst, [&](int blk, int l) { k_mult_sweep_body(A, blk * 64 + l); });
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
    RobotConst rc;
    fill_robot_const(rc);
    PipeArgs A;
    A.B = B; A.N = N; A.natt = 0; A.pad0_ = 0;
    A.lam_g = nullptr; A.lam_x = nullptr; A.cont = nullptr;
    A.o = SolverOpts{N, dt, 1e-5, 100, 2, 1.0, 0.1, 0.1, 2.0, 1000.0, 1e4, 1e-4, 1e-2, 0.0, 2, 8, 2, 1, 9};
    A.rc = &rc;
    A.x0 = w; A.lbx = lbx; A.ubx = ubx; A.p = p;
    std::vector<double> xo((size_t)B * (44 * N + 6)), fo(B), vo(B);
    std::vector<int> ito(B), sto(B);
    A.x = xo.data(); A.f = fo.data(); A.viol = vo.data(); A.g = nullptr; A.iters = ito.data(); A.status = sto.data();
    const int cap = B;
    std::vector<double> work(pipe_workspace_doubles(cap, N, 1));
    pipe_carve(A, work.data(), cap, N, 1);
    std::vector<InstState> st(cap);
    std::vector<int> l_eval(cap), l_step(cap), l_trial(cap), l_evn(cap), l_trn(cap), l_done(cap), l_admit(cap), l_curv(cap), srcv(cap), cnt(NCNT, 0), tbl(3 * HREC);
    build_scatter_table(tbl.data());
    A.st = st.data();
    A.L.eval = l_eval.data(); A.L.step = l_step.data(); A.L.trial = l_trial.data();
    A.L.eval_next = l_evn.data(); A.L.trial_next = l_trn.data(); A.L.cnt = cnt.data();
    A.L.done = l_done.data(); A.L.admit = l_admit.data(); A.L.curv = l_curv.data(); A.src = srcv.data();
    A.tbl = tbl.data();
    std::vector<double> lds(std::max<size_t>(std::max<size_t>(pair_lds_doubles(N, true), trial_lds_doubles(N, 4)), RIC_LDS_DOUBLES) + 64);
    const int nb_inst = (cap + 63) / 64, nw = waves_for(N, cap);
    cnt[0] = cap; cnt[6] = cap; cnt[9] = cap;
    launch(nb_inst, [&](int blk, int l) { k_init_inst_body(A, blk * 64 + l); });
    launch(nw, [&](int blk, int l) { k_init_body(A, blk, l, lds.data()); });
    launch(nb_inst, [&](int blk, int l) { k_init_fin_body(A, blk * 64 + l); });
    k_pool_reset_body(A, false);
    const size_t nset = (size_t)B * (N - 1) * NSLOT;
    launch((int)((nset + 63) / 64), [&](int blk, int l) { k_set_rows_body(A, (size_t)blk * 64 + l, t, z); });
    launch(nw, [&](int blk, int l) { k_points_body(A, blk, l, lds.data()); });
    launch(nw, [&](int blk, int l) { k_pose_body(A, blk, l, lds.data()); });
    if (split) {
        launch(nw, [&](int blk, int l) { k_eval_body<2>(A, blk, l, lds.data()); });
        launch(nw, [&](int blk, int l) { k_eval_body<1>(A, blk, l, lds.data()); });
    } else
        launch(nw, [&](int blk, int l) { k_eval_body<0>(A, blk, l, lds.data()); });
    if (cnt[10] != B) return -1;            // every instance is in the curvature list
    launch(waves_for(N, cnt[10]), [&](int blk, int l) { k_curv_body(A, blk, l, lds.data()); });
    launch(B, [&](int b, int lane) {
        k_stage_matrix_body<EMU_RIC_NT>(*reinterpret_cast<const PipeArgsH*>(&A), b, lane, lds.data(), lam_pi, H);
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
    RobotConst rc;
    fill_robot_const(rc);
    PipeArgs A;
    A.B = B; A.N = N; A.natt = 0; A.pad0_ = 0;
    A.lam_g = nullptr; A.lam_x = nullptr; A.cont = nullptr;
    A.o = SolverOpts{N, dt_, 1e-5, 100, 2, 1.0, 0.1, 0.1, 2.0, 1000.0, 1e4, 1e-4, 1e-2, 0.0, 2, 8, 2, 1, 9};
    A.rc = &rc;
    A.x0 = w; A.lbx = lbx; A.ubx = ubx; A.p = p;
    std::vector<double> xo((size_t)B * (44 * N + 6)), fo(B), vo(B);
    std::vector<int> ito(B), sto(B);
    A.x = xo.data(); A.f = fo.data(); A.viol = vo.data(); A.g = nullptr; A.iters = ito.data(); A.status = sto.data();
    const int cap = B;
    std::vector<double> work(pipe_workspace_doubles(cap, N, 1));
    pipe_carve(A, work.data(), cap, N, 1);
    std::vector<InstState> st(cap);
    std::vector<int> l_eval(cap), l_step(cap), l_trial(cap), l_evn(cap), l_trn(cap), l_done(cap), l_admit(cap), l_curv(cap), srcv(cap), cnt(NCNT, 0), tbl(3 * HREC);
    build_scatter_table(tbl.data());
    A.st = st.data();
    A.L.eval = l_eval.data(); A.L.step = l_step.data(); A.L.trial = l_trial.data();
    A.L.eval_next = l_evn.data(); A.L.trial_next = l_trn.data(); A.L.cnt = cnt.data();
    A.L.done = l_done.data(); A.L.admit = l_admit.data(); A.L.curv = l_curv.data(); A.src = srcv.data();
    A.tbl = tbl.data();
    std::vector<double> lds(std::max<size_t>(std::max<size_t>(pair_lds_doubles(N, true), trial_lds_doubles(N, 4)), RIC_LDS_DOUBLES) + 64);
    const int nb_inst = (cap + 63) / 64, nw = waves_for(N, cap);
    cnt[0] = cap; cnt[6] = cap; cnt[9] = cap;
    launch(nb_inst, [&](int blk, int l) { k_init_inst_body(A, blk * 64 + l); });
    launch(nw, [&](int blk, int l) { k_init_body(A, blk, l, lds.data()); });
    launch(nb_inst, [&](int blk, int l) { k_init_fin_body(A, blk * 64 + l); });
    k_pool_reset_body(A, false);
    const size_t nset = (size_t)B * (N - 1) * NSLOT;
    launch((int)((nset + 63) / 64), [&](int blk, int l) { k_set_rows_body(A, (size_t)blk * 64 + l, t, z, mode); });
    launch(nw, [&](int blk, int l) { k_points_body(A, blk, l, lds.data()); });
    launch(nw, [&](int blk, int l) { k_pose_body(A, blk, l, lds.data()); });
    launch(nw, [&](int blk, int l) { k_eval_body<0>(A, blk, l, lds.data()); });
    launch(waves_for(N, cnt[10]), [&](int blk, int l) { k_curv_body(A, blk, l, lds.data()); });
    if (variant == 1) {
        A.natt = 3;
        launch(cnt[0] * A.natt, [&](int blk, int l) { k_ric_att_body<EMU_RIC_NT, false>(*reinterpret_cast<const PipeArgsH*>(&A), blk, l, lds.data()); }, EMU_RIC_NT);
        launch(cnt[0], [&](int blk, int l) { k_ric_body<EMU_RIC_NT, false, true>(*reinterpret_cast<const PipeArgsH*>(&A), blk, l, lds.data()); }, EMU_RIC_NT);
    } else
        launch(cnt[0], [&](int blk, int l) { k_ric_body<EMU_RIC_NT>(*reinterpret_cast<const PipeArgsH*>(&A), blk, l, lds.data()); }, EMU_RIC_NT);
    launch(cnt[1], [&](int blk, int l) { k_fwd_body(A, blk, l, lds.data()); });
    launch(waves_for(N, cnt[1]), [&](int blk, int l) { k_step_body(A, blk, l, lds.data()); });
    launch((int)((nset + 63) / 64), [&](int blk, int l) { k_newton_out_body(A, (size_t)blk * 64 + l, dzeta, dt, dz, state); });
    return 0;
}
