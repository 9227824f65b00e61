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
#include "../../boundplanner_amd/csrc/bmpc_debug_step.hpp"      // (and with it include/boundmpc.h: the record of emu_superstep)

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
// bmpc_default_opts, for emu_superstep
static SolverOpts default_opts(int N, double dt) { return SolverOpts{N, dt, 1e-5, 100, 2, 1.0, 0.1, 0.1, 2.0, 1000.0, 1e4, 1e-4, 1e-2, 0.0, 2, 8, 2, 1, 9}; }

// Everything a run of the kernel bodies needs beside the caller's arrays -- workspace, instance state, lists, counters, scatter table,
// LDS buffer -- with a PipeArgs wired to it, and the launch sequences of bmpc_pipeline.hip (bmpc_pipe_launch_init, launch_eval,
// launch_direction, launch_trial, bmpc_pipe_launch_superstep) as members.  A points into the rig: it is neither copied nor moved.
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
    int nb_slot() const { return (int)(((size_t)A.B * (N - 1) * NSLOT + 63) / 64); }      // grid of one thread per (instance, stage, slot)
    void set_rows(const double* t, const double* z, const int* mode = nullptr) {
        launch(nb_slot(), [&](int blk, int l) { k_set_rows_body(A, (size_t)blk * 64 + l, t, z, mode); });
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
    // bmpc_pipe_launch_superstep, launch by launch in its order (d: the record of bmpc_debug_superstep, checked by the caller), with
    // the variants the GPU selects by batch size given as switches.  false: the stage-matrix path found an instance missing from the
    // curvature list.
    bool superstep(const bmpc_debug_step* d, bool eval_split, bool ric_spec, bool trial_spec) {
        const int nbi = (A.B + 63) / 64, nb = nb_slot();      // grids of one thread per instance / per (instance, stage, slot)
        const bool search = d->ls != nullptr;
        if (d->t) set_rows(d->t, d->z, d->H ? nullptr : d->mode);
        if (search && (d->t || d->plant0)) launch(nb, [&](int blk, int l) { k_ls_plant_body(A, (size_t)blk * 64 + l, d->plant0, 0, d->t ? 1 : 0); });
        if (d->ctl_plant) launch(nbi, [&](int blk, int l) { k_ctl_plant_body(A, (size_t)blk * 64 + l, d->ctl_plant); });
        if (!eval(nw, eval_split, d->H ? A.B : -1)) return false;
        if (d->H) {
            launch(A.B, [&](int b, int l) { k_stage_matrix_body<EMU_RIC_NT>(*reinterpret_cast<const PipeArgsH*>(&A), b, l, lds.data(), d->lam_pi, d->H); }, EMU_RIC_NT);
            return true;
        }
        direction(ric_spec);
        launch(nb, [&](int blk, int l) { k_newton_out_body(A, (size_t)blk * 64 + l, d->dzeta, d->dt, d->dz, d->state); });
        if (d->ctl) launch(nbi, [&](int blk, int l) { k_ctl_out_body(A, (size_t)blk * 64 + l, d->ctl, 0); });
        if (!search) return true;
        if (d->plant1) launch(nb, [&](int blk, int l) { k_ls_plant_body(A, (size_t)blk * 64 + l, d->plant1, 1, 0); });
        trial(trial_spec);
        launch(nb, [&](int blk, int l) { k_ls_out_body(A, (size_t)blk * 64 + l, d->zeta0, d->t0, d->z0, d->zeta1, d->t1, d->z1, d->ls); });
        if (d->ctl) launch(nbi, [&](int blk, int l) { k_ctl_out_body(A, (size_t)blk * 64 + l, d->ctl, 1); });
        return true;
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

// One super-step of the kernel bodies from a planted state (tests/test_hessian_pin.py, test_newton_step.py, test_line_search.py,
// test_iteration_control.py): the sequence of bmpc_debug_superstep (include/boundmpc.h) on the same record, with the same argument
// check.  The slots are initialised by the k_init* bodies from x0 with bmpc_default_opts, of which tol, max_iter, mu_floor_k and dw0
// are given; the rest is Rig::superstep.  Variants: eval_split runs k_eval as the two-wavefront pair <2> + <1> instead of
// k_eval_body<0>; ric_spec the speculative pair k_ric_att_body + k_ric_body<RESUME> with three attempts instead of k_ric_body (the
// kernels bmpc_k_ric / bmpc_k_ric_lat); trial_spec k_trial_spec_body (bmpc_k_trial_spec) instead of k_trial_body (bmpc_k_trial).
// The default trial_repeats: the search ends inside the trial body.  rc 1: the arguments; -1: the curvature list.
struct emu_step_cfg {
    int N, max_iter, eval_split, ric_spec, trial_spec;
    double dt, tol, mu_floor_k, dw0;
};
extern "C" int emu_superstep(const emu_step_cfg* c, int B, const bmpc_debug_step* s) {
    if (!c || bmpc_debug_step_refusal(B, s)) return 1;
    SolverOpts o = default_opts(c->N, c->dt);
    o.tol = c->tol; o.max_iter = c->max_iter; o.mu_floor_k = c->mu_floor_k; o.dw0 = c->dw0;
    Rig R(B, B, 1, o, s->x0, s->lbx, s->ubx, s->p);
    R.own_outputs();
    R.init();
    return R.superstep(s, c->eval_split != 0, c->ric_spec != 0, c->trial_spec != 0) ? 0 : -1;
}
