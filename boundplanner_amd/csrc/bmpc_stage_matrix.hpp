// bmpc_stage_matrix.hpp -- test entry (bmpc_debug_stage_matrices, tests/emu/emu_pipe.cpp): the stage matrices the Riccati sweep
// factorises, at a given point with given row slacks / multipliers and given adjoint multipliers of the pi dynamics.  Two bodies
// beside the product's kernels, none of which changes: k_set_rows_body writes (t, z) over the ones the init launch left and switches
// the exact Hessian on; after the product's evaluation kernels have run once, k_stage_matrix_body runs the sweep's own load phase
// (ric_phase_load_impl) per stage and copies the matrix it leaves in LDS.  tests/test_hessian_pin*.py compare the result with the
// reference-derived probes of tests/golden/hess_N*.npz.  The second test entry, bmpc_debug_newton_step, shares k_set_rows_body
// and adds k_newton_out_body, which copies out what the product's own Riccati, forward and row-step kernels left.
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

// Test entry bmpc_debug_newton_step (tests/test_newton_step*.py): what one super-step's k_ric / k_fwd / k_step left in the
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
