// k_step and k_pose (bmpc_pair_kernels.hpp) beside the statements they replaced -- TEST INFRASTRUCTURE ONLY
// (tests/test_step_pose_phases.py).  The product bodies run in phases, each phase's results pinned before the next starts, so that
// fewer values are alive at once; k_step_body_one_walk and k_pose_body_stage_point below are the earlier statements, line for line:
// k_step over stage_point and ONE walk_rows<WR_ALL>, k_pose over stage_point.  Both statements run on the same pairs of the same
// workspace and everything they write is handed out twice, to be compared bitwise.
#include <algorithm>
#include "emu_pipe.cpp"       // the rig (workspace, lists, lanes as threads) and the product bodies

namespace bmpc {

// ---- k_pose over stage_point ----
BMPC_KBODY void k_pose_body_stage_point(const PipeArgs& A, int wave, int lane, LDSD* lds_par) {
    const int count = A.L.cnt[0], N = A.N;
    if (wave * ipw_of(N) >= count) return;
    PairMap m = pair_map(A, A.L.eval, count, wave, lane);
    const int k = m.k, n_w = 44 * N + 6;
    const bool term = (k == N - 1);
    const DynC dc = make_dync(A.o.dt);
    GCD lbx = A.lbx + (size_t)A.src[m.b] * n_w;
    PGP pg = stage_params(A, A.L.eval, count, wave, lane, m, lds_par);
    double iw0[3];
    BMPC_UNROLL
    for (int c = 0; c < 3; c++) iw0[c] = lbx[28 * N + (3 + c) * N];
    StagePoint S;
    const int flip = A.st[m.b].flip;
    GCD zc = cur_zeta(A, flip), tc = cur_t(A, flip), zcur = cur_z(A, flip);
    load_zeta(zc, A.NP, m.pi, S.zeta);
    // row data of the pose rows: in flight while the kinematics are evaluated
    RowPre<S_EE, 21> rp_pose;
    rp_pose.load(A, tc, zcur, m.pi);
    const double t_phi = tc[(size_t)S_PHI * A.NP + m.pi], z_phi = zcur[(size_t)S_PHI * A.NP + m.pi];
    stage_point(A, pg, iw0, k, dc, S);
    double g12[12], Hp[21];
    cost_grad12(pg, S.C, term, g12);
    {
        double HvX[21];
        cost_hess(pg, S.C, term, Hp, HvX);
    }
    RowAcc R;
    R.init(&A, m.pi, m.valid, 0.0, tc, zcur);
    // (KKT partial sums of the pose rows only: k_points runs beside this kernel, k_eval combines the two)
    PoseAsm PO;
    PO.R = &R;
    PO.init(Hp, g12);
    walk_pose_rows(pg, N, k, S.y, S.C, PO, rp_pose, t_phi, z_phi);
    {
        RowPre<S_TSET, 21> rp_term;          // one batch of loads per row group, right before the group is walked
        rp_term.load(A, tc, zcur, m.pi);
        walk_pose_rows_term(pg, N, k, S.y, S.C, PO, rp_term);
    }
    if (!m.valid) return;
    const double hdt = 0.5 * dc.dt;
    // generalised forces for the second-order kinematic terms (k_curv)
    if (A.o.hess == 2) {
        GD F = A.part + (size_t)PT_FORCE * A.NP + m.pi;
        BMPC_UNROLL
        for (int a = 0; a < 3; a++) F[(size_t)a * A.NP] = PO.bpz[a];
        BMPC_UNROLL
        for (int a = 0; a < 6; a++) F[(size_t)(3 + a) * A.NP] = g12[6 + a] + (a >= 3 ? hdt * PO.bpz[a] : 0.0);
        // what the Gauss-Newton model of r = sig(phi) e leaves out of the Hessian of sig^2 (|e_r|^2 + |e_p|^2)
        // (casadi_ocp_formulation.py:272-276): 2 sig [ sig'' |e|^2 dphi dphi^T + sig' (ge dphi^T + dphi ge^T) ], ge = De^T e
        GD Sg = A.part + (size_t)PT_SIG * A.NP + m.pi;
        const double c2 = 2 * S.C.sig * S.C.dsig;
        Sg[0] = 2 * S.C.sig * (60.0 * S.C.dsig * (1.0 - 2.0 * S.C.sig)) * S.C.er2ep2;
        BMPC_UNROLL
        for (int a = 0; a < 3; a++) Sg[(size_t)(1 + a) * A.NP] = S.C.dpp[a];
        BMPC_UNROLL
        for (int bb = 0; bb < 6; bb++) {
            double ge = S.C.Der[0][bb] * S.C.er[0] + S.C.Der[1][bb] * S.C.er[1] + S.C.Der[2][bb] * S.C.er[2];
            if (bb < 3) ge += S.C.Dep[0][bb] * S.C.ep[0] + S.C.Dep[1][bb] * S.C.ep[1] + S.C.Dep[2][bb] * S.C.ep[2];
            Sg[(size_t)(4 + bb) * A.NP] = c2 * ge;
        }
    }
    GD Pz = A.part + (size_t)PT_POSE * A.NP + m.pi;
    BMPC_UNROLL
    for (int i = 0; i < 21; i++) Pz[(size_t)(PZ_M6 + i) * A.NP] = PO.M6[i];
    BMPC_UNROLL
    for (int sl = 0; sl < 3; sl++) {
        BMPC_UNROLL
        for (int i = 0; i < 6; i++) Pz[(size_t)(PZ_MS + 6 * sl + i) * A.NP] = PO.mS[sl][i];
        Pz[(size_t)(PZ_SS + sl) * A.NP] = PO.sS[sl];
        Pz[(size_t)(PZ_BS0 + sl) * A.NP] = PO.bS0[sl]; Pz[(size_t)(PZ_BS1 + sl) * A.NP] = PO.bS1[sl]; Pz[(size_t)(PZ_BSZ + sl) * A.NP] = PO.bSz[sl];
    }
    BMPC_UNROLL
    for (int i = 0; i < 6; i++) {
        Pz[(size_t)(PZ_BP0 + i) * A.NP] = PO.bp0[i]; Pz[(size_t)(PZ_BP1 + i) * A.NP] = PO.bp1[i]; Pz[(size_t)(PZ_BPZ + i) * A.NP] = PO.bpz[i];
        Pz[(size_t)(PZ_BV + i) * A.NP] = g12[6 + i];
    }
    Pz[(size_t)(PZ_KKT + 0) * A.NP] = R.cmax; Pz[(size_t)(PZ_KKT + 1) * A.NP] = R.csum; Pz[(size_t)(PZ_KKT + 2) * A.NP] = R.cmin;
    Pz[(size_t)(PZ_KKT + 3) * A.NP] = R.zsum; Pz[(size_t)(PZ_KKT + 4) * A.NP] = R.prim; Pz[(size_t)(PZ_KKT + 5) * A.NP] = R.nrows;
    BMPC_UNROLL
    for (int a = 0; a < 3; a++) Pz[(size_t)(PZ_VANG + a) * A.NP] = S.C.v[3 + a];
}

// ---- k_step over stage_point and one walk over all rows ----
BMPC_KBODY void k_step_body_one_walk(const PipeArgs& A, int wave, int lane, LDSD* lds_par) {
    const int count = A.L.cnt[1], N = A.N;
    if (wave * ipw_of(N) >= count) return;
    PairMap m = pair_map(A, A.L.step, count, wave, lane);
    const int k = m.k, n_w = 44 * N + 6;
    const bool term = (k == N - 1);
    const DynC dc = make_dync(A.o.dt);
    GCD lbx = A.lbx + (size_t)A.src[m.b] * n_w;
    GCD ubx = A.ubx + (size_t)A.src[m.b] * n_w;
    PGP pg = stage_params(A, A.L.step, count, wave, lane, m, lds_par);
    PGP wts = pg + P_W;
    const double mu = A.st[m.b].mu;
    double iw0[3];
    BMPC_UNROLL
    for (int c = 0; c < 3; c++) iw0[c] = lbx[28 * N + (3 + c) * N];
    StagePoint S;
    const int flip = A.st[m.b].flip;
    load_zeta(cur_zeta(A, flip), A.NP, m.pi, S.zeta);
    stage_point(A, pg, iw0, k, dc, S);
    double G[6][7], g12[12];
    kin_G(S.K, S.Jl, S.y + Z_DQ, G);
    cost_grad12(pg, S.C, term, g12);
    double dzt[NZ], dy[NZ];
    load_zeta(A.dz, A.NP, m.pi, dzt);
    nat_all(dzt, dc, dy);
    StepVisitor V;
    V.A = &A; V.pi = m.pi; V.valid = m.valid; V.mu = mu; V.tau = fmax(0.99, 1.0 - mu); V.tc = cur_t(A, flip); V.zc = cur_z(A, flip);
    V.dy = dy; V.dzt = dzt; V.rp = 0.0; V.rdn = 0.0; V.rdd = 1.0; V.dbar = 0.0;
    double dv[6];
    BMPC_UNROLL
    for (int a = 0; a < 6; a++) {
        double s = 0;
        BMPC_UNROLL
        for (int j = 0; j < 7; j++) s += G[a][j] * dy[Z_Q + j] + (a < 3 ? S.Jl[a][j] : S.K.zx[j][a - 3]) * dy[Z_DQ + j];
        dv[a] = s;
    }
    BMPC_UNROLL
    for (int a = 0; a < 3; a++) {
        double s = 0;
        BMPC_UNROLL
        for (int j = 0; j < 7; j++) s += S.Jl[a][j] * dy[Z_Q + j];
        V.dloc[a] = s;
        V.dloc[3 + a] = dy[Z_PI + a] + 0.5 * dc.dt * dv[3 + a];
    }
    point_dirs<0>(S.K, dy + Z_Q, V.dpt);
    // directional derivative of f
    double dphi_f = 0;
    BMPC_UNROLL
    for (int a = 0; a < 6; a++) dphi_f += g12[a] * V.dloc[a] + g12[6 + a] * dv[a];
    BMPC_UNROLL
    for (int j = 2; j <= 4; j++) dphi_f += 2 * wts[6] * S.y[Z_DQ + j] * dy[Z_DQ + j];
    BMPC_UNROLL
    for (int j = 0; j < 7; j++) dphi_f += 2 * wts[7] * S.y[Z_U + j] * dy[Z_U + j];
    dphi_f += 2 * wts[9] * S.y[Z_RS] * dy[Z_RS] + 2 * wts[10] * S.y[Z_DRS] * dy[Z_DRS] +
              2 * wts[9] * S.y[Z_PS] * dy[Z_PS] + 2 * wts[10] * S.y[Z_DPS] * dy[Z_DPS];
    if (term)
        BMPC_UNROLL
        for (int i = 0; i < 6; i++) {
            double gg = 2 * wts[10] * S.y[Z_D + i] + (i != 4 ? 2 * wts[8] * (pg[P_SLACKS0 + i] + S.y[Z_D + i]) : 0.0);
            dphi_f += gg * dy[Z_D + i];
        }
    walk_rows(pg, lbx, ubx, N, k, S.y, S.zeta, S.K, S.C, V);
    if (m.valid) {
        GD P = A.part + m.pi;
        P[PT_DPHIF * A.NP] = dphi_f;
        P[PT_AP * A.NP] = (V.rp > 0) ? V.tau / V.rp : 1.0; P[PT_AD * A.NP] = (V.rdn > 0) ? V.tau / (V.rdn / V.rdd) : 1.0; P[PT_DBAR * A.NP] = V.dbar;
    }
    // the pairs of an instance are lanes of this wavefront: line-search start per instance (a kernel of its own, then part
    // of the streaming row kernel k_rowstep, before the row steps moved in here)
    BMPC_FENCE_SYNC();
    if (m.valid && m.k == 1) ls0_instance(A, m.b);
}

}  // namespace bmpc

// fields of the per-pair partials that k_pose writes: PT_POSE (PZ_END), Fp and Fv of PT_FORCE (Fc is k_points'), PT_SIG
static constexpr int SP_POSE = PZ_END + 9 + 10;
static int sp_pose_field(int i) { return i < PZ_END ? PT_POSE + i : i < PZ_END + 9 ? PT_FORCE + (i - PZ_END) : PT_SIG + (i - PZ_END - 9); }
// what ls0_instance writes per instance
static constexpr int SP_INST = 12;
static const int SP_STEP_PARTS[4] = {PT_DPHIF, PT_AP, PT_AD, PT_DBAR};

extern "C" void emu_step_pose_layout(int* out) {
    out[0] = NSLOT; out[1] = SP_POSE; out[2] = SP_INST; out[3] = S_EE; out[4] = S_COL; out[5] = S_PHI; out[6] = S_END; out[7] = NZ;
}

// B instances at the points w [B][n_w] with row slacks / multipliers t, z [B][N-1][NSLOT] (kernel slots) and the step dzeta
// [B][N-1][NZ]: slots initialised by the k_init* bodies from x0 = w, rows written over them (k_set_rows_body), dzeta written into the
// workspace's dz, every slot in the step list.  which = 0: the product bodies, 1: the earlier statements.  Per call, with NaN in
// everything the bodies are to write beforehand:
//   pose [B][N-1][SP_POSE]      the fields of sp_pose_field
//   rows [B][N-1][NSLOT]        k_step's dt rows (t + dt; NaN where no row is)
//   parts [B][N-1][4]           PT_DPHIF, PT_AP, PT_AD, PT_DBAR
//   inst [B][SP_INST]           ap, ad, D, phi0, theta_max, theta_min, alpha, bt, armijo, state, nfilt, filt_mu
//   trial [B]                   the trial list, sorted (its order is the lanes' arrival order)
extern "C" int emu_step_pose(int N, double dt_, int B, const double* w, const double* lbx, const double* ubx, const double* p,
                             const double* t, const double* z, const double* dzeta, int which, double* pose, double* rows,
                             double* parts, double* inst, int* trial) {
    Rig R(B, B, 1, default_opts(N, dt_), w, lbx, ubx, p);
    R.own_outputs();
    R.init();
    R.set_rows(t, z);
    PipeArgs& A = R.A;
    const size_t S = (size_t)(N - 1);
    const double nan = __builtin_nan("");
    for (int b = 0; b < B; b++)
        for (size_t k = 1; k <= S; k++) {
            const size_t pi = pair_of(A, b, (int)k);
            for (int i = 0; i < NZ; i++) A.dz[(size_t)i * A.NP + pi] = dzeta[((size_t)b * S + (k - 1)) * NZ + i];
            for (int i = 0; i < SP_POSE; i++) A.part[(size_t)sp_pose_field(i) * A.NP + pi] = nan;
            for (int i = 0; i < 4; i++) A.part[(size_t)SP_STEP_PARTS[i] * A.NP + pi] = nan;
            for (int s = 0; s < NSLOT; s++) A.dt[(size_t)s * A.NP + pi] = nan;
        }
    if (R.cnt[0] != B) return 1;
    double* const lds = R.lds.data();
    if (which == 0) launch(R.nw, [&](int blk, int l) { k_pose_body(A, blk, l, lds); });
    else launch(R.nw, [&](int blk, int l) { k_pose_body_stage_point(A, blk, l, lds); });
    for (int b = 0; b < B; b++) {
        A.L.step[b] = b;
        R.st[b].ap = R.st[b].ad = R.st[b].D = R.st[b].phi0 = R.st[b].alpha = nan;
    }
    R.cnt[1] = B; R.cnt[2] = 0;
    if (which == 0) launch(R.nw, [&](int blk, int l) { k_step_body(A, blk, l, lds); });
    else launch(R.nw, [&](int blk, int l) { k_step_body_one_walk(A, blk, l, lds); });
    if (R.cnt[2] != B) return 2;
    for (int b = 0; b < B; b++) {
        if (A.src[b] != b) return 3;
        for (size_t k = 1; k <= S; k++) {
            const size_t pi = pair_of(A, b, (int)k), o = (size_t)b * S + (k - 1);
            for (int i = 0; i < SP_POSE; i++) pose[o * SP_POSE + i] = A.part[(size_t)sp_pose_field(i) * A.NP + pi];
            for (int i = 0; i < 4; i++) parts[o * 4 + i] = A.part[(size_t)SP_STEP_PARTS[i] * A.NP + pi];
            for (int s = 0; s < NSLOT; s++) rows[o * NSLOT + s] = A.dt[(size_t)s * A.NP + pi];
        }
        const InstState& st = R.st[b];
        double* q = inst + (size_t)b * SP_INST;
        q[0] = st.ap; q[1] = st.ad; q[2] = st.D; q[3] = st.phi0; q[4] = st.theta_max; q[5] = st.theta_min; q[6] = st.alpha; q[7] = st.bt;
        q[8] = st.armijo; q[9] = st.state; q[10] = st.nfilt; q[11] = st.filt_mu;
        trial[b] = A.L.trial[b];
    }
    std::sort(trial, trial + B);
    return 0;
}
