// bmpc_stage_matrix.hpp -- the bodies of the test entry bmpc_debug_superstep (include/boundmpc.h) beside the product's kernels, none
// of which changes; bmpc_pipe_launch_superstep (bmpc_pipeline.hip) and Rig::superstep (tests/emu/emu_pipe.cpp) run them in one
// sequence, one super-step from a planted state:
//   init launch -> k_set_rows_body (t, z written over the ones the init launch left, the first attempt's Hessian mode)
//     -> k_ls_plant_body (line-search state before the evaluation, NaN in the copies the trial writes) -> k_ctl_plant_body
//     (iteration-control state) -> the product's evaluation kernels
//     -> k_stage_matrix_body: the sweep's own load phase (ric_phase_load_impl) per stage, the matrix it leaves in LDS copied out; stop
//        (tests/test_hessian_pin*.py compare it with the reference-derived probes of tests/golden/hess_N*.npz)
//     -> the product's Riccati, forward and row-step kernels -> k_newton_out_body (what they left) -> k_ctl_out_body (what the Riccati
//        kernel's control left of the iteration-control state); stop, or
//     -> k_ls_plant_body (line-search state after k_step) -> the product's trial kernel -> k_ls_out_body (the iterate before and after
//        the search, the line-search state) -> k_ctl_out_body (what ls_decide left).
#pragma once
#include "bmpc_ric_kernel.hpp"

namespace bmpc {
#define RL(x) (lds + (x))

// one thread per (instance row, stage, slot): t, z [B][N-1][NSLOT] in the slot numbering of bmpc_device.hpp (S_*).  mode (per
// instance row, or null = 1 everywhere): the Hessian of the first factorisation attempt -- 0 Gauss-Newton, 1 exact, 2 exact with the
// KKT error of the previous iterate set to 0, the state in which a failed attempt is answered by delta_w and not by the Gauss-Newton
// fallback (k_ric_body: gn_ok).  The row-step array gets a NaN in every slot, so that a reader can tell the slots k_step wrote.
BMPC_INL void k_set_rows_body(const PipeArgs& A, size_t e, GCD t, GCD z, GCI mode = nullptr) {
    const size_t S = (size_t)(A.N - 1);
    if (e >= (size_t)A.B * S * NSLOT) return;
    const int b = (int)(e / (S * NSLOT));                 // slot = row: the pool was filled by the init launch (src[b] = b)
    const int k = (int)((e / NSLOT) % S) + 1, s = (int)(e % NSLOT);
    const int flip = A.st[b].flip;
    const size_t dst = (size_t)s * A.NP + pair_of(A, b, k);
    cur_t(A, flip)[dst] = t[e];
    cur_z(A, flip)[dst] = z[e];
    A.dt[dst] = __builtin_nan("");
    if (k == 1 && s == 0) {
        const int m = mode ? mode[b] : 1;
        A.st[b].hess_mode = m != 0;
        if (m == 2) A.st[b].err_prev = 0.0;
    }
}

// The Newton step (tests/test_newton_step*.py): what one super-step's k_ric / k_fwd / k_step left in the
// workspace, one thread per (instance row, stage, slot).  dzeta [B][N-1][NZ]; dt, dz [B][N-1][NSLOT]: dt = c - t with k_step's
// stored c = t + dt, dz = (mu - z c) / t as StepVisitor::fin and k_trial form it (NaN in the slots k_step did not write);
// state [B][12]: the fields of bmpc_debug_inst_state.
BMPC_INL void k_newton_out_body(const PipeArgs& A, size_t e, GD dzeta, GD dt, GD dz, GD state) {
    const size_t S = (size_t)(A.N - 1);
    if (e >= (size_t)A.B * S * NSLOT) return;
    const int b = (int)(e / (S * NSLOT));
    const int k = (int)((e / NSLOT) % S) + 1, s = (int)(e % NSLOT);
    const size_t row = (size_t)A.src[b], pi = pair_of(A, b, k), dst = (size_t)s * A.NP + pi;
    const int flip = A.st[b].flip;
    const double mu = A.st[b].mu, t = cur_t(A, flip)[dst], z = cur_z(A, flip)[dst], c = A.dt[dst];
    const size_t o = (row * S + (size_t)(k - 1)) * NSLOT + s;
    dt[o] = c - t;
    dz[o] = (mu - z * c) * BMPC_RCP(t);
    if (s < NZ) dzeta[(row * S + (size_t)(k - 1)) * NZ + s] = A.dz[(size_t)s * A.NP + pi];
    if (k == 1 && s == 0) {
        const GST st = A.st + b;
        GD q = state + row * 12;
        q[0] = st->it; q[1] = st->state == ST_DONE ? st->status : -1; q[2] = st->mu; q[3] = st->alpha; q[4] = st->ad; q[5] = st->ap;
        q[6] = st->hreg; q[7] = st->hess_mode; q[8] = st->tries; q[9] = st->bt; q[10] = st->err_prev; q[11] = st->stall;
    }
}

// The line search (tests/test_line_search*.py).  Doubles per instance of the two planted records and of the
// returned line-search state:
//   plant, before the evaluation launches [LS_PLANT0]: f0, th0, ls0, it, filt_mu, nfilt, filt_th[8], filt_phi[8]
//   plant, after k_step                   [LS_PLANT1]: nfilt, filt_th[8], filt_phi[8], theta_max, theta_min
//   state                                 [LS_OUT]:    ap, ad, D, phi0, alpha, bt, f0, th0, ls0, nfilt, filt_th[8], filt_phi[8] (NaN beyond nfilt),
//                                                      theta_max, theta_min, it, flip, hess_mode, state, mu, filt_mu, armijo, 0
constexpr int LS_PLANT0 = 22, LS_PLANT1 = 19, LS_OUT = 36;

// one thread per (instance row, stage, slot).  plant (may be null): the record of `after_step` (0 / 1) per instance row, a NaN
// leaves the field as the product made it.  nan_other: a NaN goes into every slot of the copies of t, z and zeta that are NOT the
// iterate -- the ones k_trial writes the trial point to -- so that a reader can tell what the search wrote.
BMPC_INL void k_ls_plant_body(const PipeArgs& A, size_t e, GCD plant, int after_step, int nan_other) {
    const size_t S = (size_t)(A.N - 1);
    if (e >= (size_t)A.B * S * NSLOT) return;
    const int b = (int)(e / (S * NSLOT));                 // slot = row: the pool was filled by the init launch (src[b] = b)
    const int k = (int)((e / NSLOT) % S) + 1, s = (int)(e % NSLOT);
    const GST st = A.st + b;
    if (nan_other) {
        const int flip = st->flip;
        const size_t dst = (size_t)s * A.NP + pair_of(A, b, k);
        oth_t(A, flip)[dst] = __builtin_nan("");
        oth_z(A, flip)[dst] = __builtin_nan("");
        if (s < NZ) oth_zeta(A, flip)[dst] = __builtin_nan("");
    }
    if (!plant || k != 1 || s != 0) return;
    if (!after_step) {
        GCD q = plant + (size_t)b * LS_PLANT0;
        if (q[0] == q[0]) st->f0 = q[0];
        if (q[1] == q[1]) st->th0 = q[1];
        if (q[2] == q[2]) st->ls0 = q[2];
        if (q[3] == q[3]) st->it = (int)q[3];
        if (q[4] == q[4]) st->filt_mu = q[4];
        if (q[5] == q[5]) st->nfilt = (int)q[5];
        for (int j = 0; j < 8; j++) {
            if (q[6 + j] == q[6 + j]) st->filt_th[j] = q[6 + j];
            if (q[14 + j] == q[14 + j]) st->filt_phi[j] = q[14 + j];
        }
    } else {
        GCD q = plant + (size_t)b * LS_PLANT1;
        if (q[0] == q[0]) st->nfilt = (int)q[0];
        for (int j = 0; j < 8; j++) {
            if (q[1 + j] == q[1 + j]) st->filt_th[j] = q[1 + j];
            if (q[9 + j] == q[9 + j]) st->filt_phi[j] = q[9 + j];
        }
        if (q[17] == q[17]) st->theta_max = q[17];
        if (q[18] == q[18]) st->theta_min = q[18];
    }
}

// one thread per (instance row, stage, slot), after the trial launch: zeta0 / zeta1 [B][N-1][NZ], t0, z0, t1, z1 [B][N-1][NSLOT]
// (kernel slots), ls [B][LS_OUT].  An accepted (or forced) trial has flipped the instance's copies: the iterate before the search is
// the other copy now.  An instance that took no step (finished at entry) returns its iterate as the one before and NaN after.
BMPC_INL void k_ls_out_body(const PipeArgs& A, size_t e, GD zeta0, GD t0, GD z0, GD zeta1, GD t1, GD z1, GD ls) {
    const size_t S = (size_t)(A.N - 1);
    if (e >= (size_t)A.B * S * NSLOT) return;
    const int b = (int)(e / (S * NSLOT));
    const int k = (int)((e / NSLOT) % S) + 1, s = (int)(e % NSLOT);
    const GST st = A.st + b;
    const size_t row = (size_t)A.src[b], src = (size_t)s * A.NP + pair_of(A, b, k);
    const bool moved = st->state != ST_DONE;
    const int now = st->flip, was = moved ? now ^ 1 : now;
    const size_t o = (row * S + (size_t)(k - 1)) * NSLOT + s;
    const double nan = __builtin_nan("");
    t0[o] = cur_t(A, was)[src]; z0[o] = cur_z(A, was)[src];
    t1[o] = moved ? cur_t(A, now)[src] : nan; z1[o] = moved ? cur_z(A, now)[src] : nan;
    if (s < NZ) {
        const size_t oz = (row * S + (size_t)(k - 1)) * NZ + s;
        zeta0[oz] = cur_zeta(A, was)[src];
        zeta1[oz] = moved ? cur_zeta(A, now)[src] : nan;
    }
    if (k == 1 && s == 0) {
        GD q = ls + row * LS_OUT;
        q[0] = st->ap; q[1] = st->ad; q[2] = st->D; q[3] = st->phi0; q[4] = st->alpha; q[5] = st->bt; q[6] = st->f0; q[7] = st->th0;
        q[8] = st->ls0; q[9] = st->nfilt;
        // (entries beyond nfilt are no state: whatever an earlier instance of the slot left there -- returned as NaN)
        for (int j = 0; j < 8; j++) { const bool in = j < st->nfilt; q[10 + j] = in ? st->filt_th[j] : nan; q[18 + j] = in ? st->filt_phi[j] : nan; }
        q[26] = st->theta_max; q[27] = st->theta_min; q[28] = st->it; q[29] = st->flip; q[30] = st->hess_mode; q[31] = st->state;
        q[32] = st->mu; q[33] = st->filt_mu; q[34] = st->armijo; q[35] = 0.0;
    }
}

// The iteration control (tests/test_iteration_control*.py).  Doubles per instance of the planted record and of the
// returned control state:
//   plant, before the evaluation launches [CTL_PLANT]: mu, err_prev, err_best, stall, dw_last, gn_back, gn_skip, it
//   state [CTL_OUT], after the direction launches:     state, status (-1: not finished), mu, hreg, tries, ksel, hess_mode, err_prev,
//                                                      err_best, stall, dw_last, gn_back, gn_skip, it, fk
//                    after the trial launch:           it, hess_mode, gn_skip, state; 0
constexpr int CTL_PLANT = 8, CTL_OUT = 20;

// one thread per instance row, after k_set_rows_body / k_ls_plant_body.  plant [B][CTL_PLANT]: a NaN leaves the field as the init
// launch (and the mode of k_set_rows_body: hess_mode, err_prev = 0 with mode 2) made it.
BMPC_INL void k_ctl_plant_body(const PipeArgs& A, size_t e, GCD plant) {
    if (e >= (size_t)A.B) return;
    const GST st = A.st + e;                              // slot = row: the pool was filled by the init launch (src[b] = b)
    GCD q = plant + e * CTL_PLANT;
    if (q[0] == q[0]) st->mu = q[0];
    if (q[1] == q[1]) st->err_prev = q[1];
    if (q[2] == q[2]) st->err_best = q[2];
    if (q[3] == q[3]) st->stall = (int)q[3];
    if (q[4] == q[4]) st->dw_last = q[4];
    if (q[5] == q[5]) st->gn_back = (int)q[5];
    if (q[6] == q[6]) st->gn_skip = (int)q[6];
    if (q[7] == q[7]) st->it = (int)q[7];
}

// one thread per instance row: ctl [B][CTL_OUT]; after_trial = 0 writes entries 0 .. 14, 1 writes 15 .. 19
BMPC_INL void k_ctl_out_body(const PipeArgs& A, size_t e, GD ctl, int after_trial) {
    if (e >= (size_t)A.B) return;
    const GST st = A.st + e;
    GD q = ctl + (size_t)A.src[e] * CTL_OUT;
    if (!after_trial) {
        q[0] = st->state; q[1] = st->state == ST_DONE ? st->status : -1; q[2] = st->mu; q[3] = st->hreg; q[4] = st->tries; q[5] = st->ksel;
        q[6] = st->hess_mode; q[7] = st->err_prev; q[8] = st->err_best; q[9] = st->stall; q[10] = st->dw_last; q[11] = st->gn_back;
        q[12] = st->gn_skip; q[13] = st->it; q[14] = st->fk;
    } else {
        q[15] = st->it; q[16] = st->hess_mode; q[17] = st->gn_skip; q[18] = st->state; q[19] = 0.0;
    }
}

// NT lanes per instance (one workgroup): lam_pi [B][N][3] (lam_pi[k] multiplies pi_{k-1} + dt w_{k-1} - pi_k; stage k uses
// lam_pi[k+1]); Hout [B][N-1][NZ][NZ], zeta coordinates, row-major.  lds: RIC_LDS_DOUBLES.
template <int NT>
BMPC_INL void k_stage_matrix_body(RicArgs AH, int b, int lane, LDSD* lds, GCD lam_pi, GD Hout) {
    RicArgsRef A = ric_args(AH);
    const int N = A.N;
    if (b >= A.B) return;
    // this lane's scatter-table entries, packed as ric_backward packs them
    constexpr int NF = HREC / NT;
    int tpk[NF];
    const int junk = R_misc + (lane & 31);
    BMPC_UNROLL
    for (int i = 0; i < NF; i++) {
        const int f = lane + NT * i;
        int ps = A.tbl[3 * f], o1 = A.tbl[3 * f + 1], o2 = A.tbl[3 * f + 2];
        if (ps == 0) { o1 = -1; o2 = -1; }
        if (ps == 1 && o2 < 0) o2 = junk;
        tpk[i] = (o1 < 0 ? 8191 : o1) | ((o2 < 0 ? 8191 : o2) << 13) | (ps << 26);
    }
    if (lane == 0) RL(R_park)[12] = 0.0;                  // no inertia correction
    const size_t row = (size_t)A.src[b];
    for (int k = N - 1; k >= 1; k--) {
        if (lane < NX) RL(R_lam)[lane] = (k < N - 1 && lane >= Z_PI && lane < Z_PI + 3) ? lam_pi[(row * N + k + 1) * 3 + (lane - Z_PI)] : 0.0;
        BMPC_SYNC();
        ric_phase_load_impl<NT>(AH, lds, b, lane, k, 1, tpk);
        BMPC_SYNC();
        for (int e = lane; e < NZ * NZ; e += NT) Hout[(row * (N - 1) + (k - 1)) * NZ * NZ + e] = RL(R_W)[(e / NZ) * LDW + e % NZ];
        BMPC_SYNC();
    }
}

#undef RL
}  // namespace bmpc
