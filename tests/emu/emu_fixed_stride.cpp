// CPU thread emulation of the pair kernels' two instantiations -- TEST INFRASTRUCTURE ONLY (tests/test_fixed_stride_emu.py).
// The bodies that bmpc_pipeline.hip dispatches per horizon (bmpc_pair_fixed.hpp: k_points, k_pose, k_eval<1>, k_eval<2>, k_curv beside
// them, k_step, k_trial, k_trial_spec) run `steps` super-steps from the cold start, once on the generic view of the argument block
// (PipeArgs) and once on the fixed-horizon view (PipeArgsN<N>: N, NP and the slot strides are constants, the lane's column of an SoA
// array is a base pointer).  The Riccati body, k_fwd and the list rotation are the same code both times.  The caller compares the whole
// workspace and the instance states.  Rig, launch: emu_pipe.cpp.
#include "emu_pipe.cpp"

template <class AT>
static void super_steps(Rig& R, const AT& A, int steps, bool trial_spec, int* bt_max, int* rounds) {
    const int N = R.N;
    double* const lds = R.lds.data();
    for (int s = 0; s < steps; s++) {
        const int n = waves_for(N, R.cnt[0]);
        launch(n, [&](int blk, int l) { k_points_body(A, blk, l, lds); });
        launch(n, [&](int blk, int l) { k_pose_body(A, blk, l, lds); });
        launch(n, [&](int blk, int l) { k_eval_body<2>(A, blk, l, lds); });
        launch(n, [&](int blk, int l) { k_eval_body<1>(A, blk, l, lds); });
        launch(waves_for(N, R.cnt[10]), [&](int blk, int l) { k_curv_body(A, blk, l, lds); });
        const PipeArgsH& AH = *reinterpret_cast<const PipeArgsH*>(&R.A);
        launch(R.cnt[0], [&](int blk, int l) { k_ric_body<EMU_RIC_NT>(AH, blk, l, lds); }, EMU_RIC_NT);
        launch(R.cnt[1], [&](int blk, int l) { k_fwd_body(R.A, blk, l, lds); });
        launch(waves_for(N, R.cnt[1]), [&](int blk, int l) { k_step_body(A, blk, l, lds); });
        if (trial_spec) launch(waves_for(N, R.cnt[2]), [&](int blk, int l) { k_trial_spec_body(A, blk, l, lds); }, 64 * TRIAL_SPEC);
        else launch(waves_for(N, R.cnt[2]), [&](int blk, int l) { k_trial_body_t<1>(A, blk, l, lds); });
        // rejected trials of this super-step's line searches, per instance (bt is reset when the next search starts, in k_step)
        for (int b = 0; b < R.cap; b++) { *bt_max = std::max(*bt_max, R.st[b].bt); *rounds += R.st[b].bt; }
        k_rotate_body(R.A);
        std::swap(R.A.L.eval, R.A.L.eval_next);
        std::swap(R.A.L.trial, R.A.L.trial_next);
    }
}

extern "C" size_t emu_fixed_work_doubles(int N, int B) { return pipe_workspace_doubles(B, N, 1); }
extern "C" size_t emu_fixed_state_bytes(int B) { return (size_t)B * sizeof(InstState); }

// fixed = 0: the generic bodies; 1: the instantiation for N (20 or 30; anything else returns -1).  trial_spec = 1: k_trial_spec_body.
// work [emu_fixed_work_doubles], state [emu_fixed_state_bytes]: the workspace and the instance states after the last super-step;
// bt[0]: the largest number of rejected trials of one line search, bt[1]: rejected trials in all.
extern "C" int emu_fixed_super_steps(int N, double dt, int B, const double* x0, const double* lbx, const double* ubx, const double* p,
                                     int fixed, int steps, int trial_spec, double* work, unsigned char* state, int* bt) {
    Rig R(B, B, 1, default_opts(N, dt), x0, lbx, ubx, p);
    R.own_outputs();
    std::memset((void*)R.st.data(), 0, (size_t)B * sizeof(InstState));      // (padding bytes too: the states are compared as bytes)
    R.init();
    bt[0] = 0; bt[1] = 0;
    if (!fixed) super_steps(R, R.A, steps, trial_spec != 0, bt, bt + 1);
    else if (N == 20) super_steps(R, *reinterpret_cast<const PipeArgsN<20>*>(&R.A), steps, trial_spec != 0, bt, bt + 1);
    else if (N == 30) super_steps(R, *reinterpret_cast<const PipeArgsN<30>*>(&R.A), steps, trial_spec != 0, bt, bt + 1);
    else return -1;
    std::memcpy(work, R.work.data(), R.work.size() * sizeof(double));
    std::memcpy(state, R.st.data(), (size_t)B * sizeof(InstState));
    return 0;
}
