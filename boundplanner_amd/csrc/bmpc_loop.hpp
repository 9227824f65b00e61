// bmpc_loop.hpp -- device-resident closed loop: the per-rollout logic of one receding-horizon step
// either side of the NLP solve, one thread per rollout (BASELINE.json configs[4]: thousands of
// rollouts advanced in lock step, nothing but the rollout log crosses PCIe).
//
// Restates (SURVEY.md section 8 rows a9, a11, a12 (sliding window), a13):
//   BoundMPC.step before the solve           /root/reference/bound_planner/BoundMPC/BoundMPC.py:388-589
//   acceptance + compute_return_data         BoundMPC.py:604-676, 678-1040
//   reference_function / error_function      BoundMPC/bound_mpc_functions.py:49-390 (numpy branches)
//   compute_initial_rot_errors, integrate_rotation_reference   bound_mpc_functions.py:16-46
//   compute_orientation_projection_vectors   BoundMPC.py:338-386
//   jac_SO3_inv_left/right, rodrigues_matrix utils/optimization_functions.py:35-104
//   ReferencePath.update / set_point         ReferencePath/ReferencePath.py:160-207
//   integrate_joint (first hat interval)     utils/util_functions.py:55-65, jerk_trajectory_casadi.py:78-175
//   MPCNode.step state advance               BoundMPC/MPCNode.py:106-160
//   obstacle-free collision sets             BoundPlanner/ConvexSetFinder.py:400-421 (+ util_functions.py:121-135)
//   plan-time construction                   ReferencePath.py:12-157, BoundMPC.py:28-336 (loop_install_path)
// The plan-time construction (ReferencePath.__init__, BoundMPC.__init__ / update) has two routes into the state
// vector below: built on the host (boundplanner_amd/reference_path.py, bound_mpc.py) and serialised by
// boundplanner_amd/device_loop.py pack_state, or written on the device by loop_install_path, which restates
// exactly that host code.  Scenes with obstacles are handled on the device as well: the per-step collision
// sets come from a closest-pair pass, one thread per (rollout, collision point, obstacle) (loop_collision_pair), and the greedy
// choice of separating halfspaces per (rollout, collision point) inside loop_prepare -- the scene image, the closest pair and the
// greedy routine are those of bmpc_freespace.hpp, shared with the set kernel (one shared scene, or one scene per rollout).
//
// Written against the platform macros of bmpc_platform_hip.hpp so that tests/emu/emu_loop.cpp can run
// the identical source on the CPU against the reference's closed-loop trace (test infrastructure only).
#pragma once
#include "bmpc_freespace.hpp"

namespace bmpc {

constexpr int LP_NL = 11;        // via points + nr_segs-1 padded copies, at most (8 via points)
constexpr int LP_S = 4;          // nr_segs
constexpr int LP_NMAX = 64;      // horizon bound of the solver
constexpr int LP_LOGW = 24;      // doubles per (step, rollout) log row
// Optional per-(step, selected rollout) record with the content of the reference's trace message (boundmpcmsg/msg/MPCData.msg:1-64):
//   header [16]: iters, status, viol, error_count, n (valid stages), sector, phi_max, split_idxs[5] (before the step), next selector, 0, 0, 0
//   stage i < N [LP_REC_STAGE each; zero beyond n]: p 6, v 6, q 7, dq 7, ddq 7, dddq 7, phi, dphi, e_p 3, de_p 3, e_r 3, de_r 3,
//       e_r_orth1, e_r_par, e_r_orth2 (coordinates along br1, dp_normed, br2), p_ref 6, segment
//   sets [600]: the a_set / b_set / a_set_joints / b_set_joints blocks of the step's parameter vector (casadi_ocp_formulation.py:407-415)
constexpr int LP_REC_HDR = 16, LP_REC_STAGE = 64, LP_REC_SETS = 600;
BMPC_HD int lp_rec_doubles(int N) { return LP_REC_HDR + LP_REC_STAGE * N + LP_REC_SETS; }

// ---- state vector of one rollout (doubles; integers are stored exactly) -------------------------
#define LP_FIELDS(X)                                                                                  \
    X(q, 7) X(dq, 7) X(ddq, 7) X(jerk, 7) X(qf, 7) X(v, 6) X(p_lie, 6)                                \
    X(split, 5) X(sw, 1) X(error_count, 1) X(has_prev, 1) X(slacks0, 6) X(pr_ref, 3) X(iw_ref, 3)     \
    X(phi_current, 1) X(dphi_current, 1) X(phi_max, 1) X(weights, 11)                                 \
    X(dtau, 12) X(dtau_par, 12) X(dtau_o1, 12) X(dtau_o2, 12) /* [seg][c] */                          \
    X(jac_l, 9) X(jac_r, 9) /* row-major */ X(v1, 12) X(v2, 12) X(v3, 12) /* [c][seg] */              \
    X(patch, 1) X(patch_delta, 3) X(accept, 1) X(dead, 1) X(steps, 1)                                 \
    X(rp_sector, 1) X(rp_num_sectors, 1) X(rp_phi_bias, 1) X(rp_phi_max, 1)                           \
    X(rp_p, 33) X(rp_r_tau, 33) X(rp_dr, 33) X(rp_drn, 33) X(rp_iw, 33) X(rp_dp, 33) X(rp_phi, 12)    \
    X(rp_bp1, 33) X(rp_bp2, 33) X(rp_br1, 33) X(rp_br2, 33) X(rp_erb, 66) X(rp_a, 495) X(rp_b, 165)   \
    X(rp_pd, 24) X(rp_r_taud, 12) X(rp_dpd, 24) X(rp_dpdn, 12) /* [c][seg] */ X(rp_phi_switch, 5)

enum LoopField {
#define X(n, c) LF_##n,
    LP_FIELDS(X)
#undef X
        LF_COUNT
};
constexpr int LS_CNT[LF_COUNT] = {
#define X(n, c) c,
    LP_FIELDS(X)
#undef X
};
constexpr int ls_off(int f) {
    int o = 0;
    for (int i = 0; i < f; i++) o += LS_CNT[i];
    return o;
}
#define X(n, c) constexpr int LS_##n = ls_off(LF_##n);
LP_FIELDS(X)
#undef X
constexpr int LS_SIZE = (ls_off(LF_COUNT) + 7) / 8 * 8;

// robot limits and collision-sphere radii (URDF <limit>, RobotModel.py:37-54, BoundMPC.py:171-191): RobotConst

// ---- SO(3) helpers (conventions of scipy.spatial.transform.Rotation, which the reference calls) ----
BMPC_INL void lp_quat_to_mat(const double* q, double* R) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w, xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
    R[0] = x2 - y2 - z2 + w2; R[1] = 2 * (xy - zw);       R[2] = 2 * (xz + yw);
    R[3] = 2 * (xy + zw);     R[4] = -x2 + y2 - z2 + w2;  R[5] = 2 * (yz - xw);
    R[6] = 2 * (xz - yw);     R[7] = 2 * (yz + xw);       R[8] = -x2 - y2 + z2 + w2;
}

BMPC_INL void lp_rotvec_to_mat(const double* v, double* R) {
    const double a = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    double sc;
    if (a <= 1e-3) { const double a2 = a * a; sc = 0.5 - a2 / 48 + a2 * a2 / 3840; }
    else sc = sin(a / 2) / a;
    const double q[4] = {sc * v[0], sc * v[1], sc * v[2], cos(a / 2)};
    lp_quat_to_mat(q, R);
}

BMPC_INL void lp_mat_to_rotvec(const double* M, double* v) {
    const double tr = M[0] + M[4] + M[8];
    const double dec[4] = {M[0], M[4], M[8], tr};
    int ch = 0;
    for (int i = 1; i < 4; i++) if (dec[i] > dec[ch]) ch = i;
    double q[4];
    if (ch != 3) {
        const int i = ch, j = (i + 1) % 3, k = (j + 1) % 3;
        q[i] = 1 - tr + 2 * M[3 * i + i];
        q[j] = M[3 * j + i] + M[3 * i + j];
        q[k] = M[3 * k + i] + M[3 * i + k];
        q[3] = M[3 * k + j] - M[3 * j + k];
    } else {
        q[0] = M[7] - M[5]; q[1] = M[2] - M[6]; q[2] = M[3] - M[1]; q[3] = 1 + tr;
    }
    const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; i++) q[i] /= nq;
    if (q[3] < 0) for (int i = 0; i < 4; i++) q[i] = -q[i];
    const double a = 2 * atan2(sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), q[3]);
    double sc;
    if (a <= 1e-3) { const double a2 = a * a; sc = 2 + a2 / 12 + 7 * a2 * a2 / 2880; }
    else sc = a / sin(a / 2);
    for (int i = 0; i < 3; i++) v[i] = sc * q[i];
}

// extrinsic z-y-x Euler angles (as_euler("zyx")): M = Rx(e2) Ry(e1) Rz(e0)
BMPC_INL void lp_euler_zyx(const double* M, double* e) {
    const double PI = 3.14159265358979323846;
    // M[2] = sin e1, (M[0], M[1]) = cos e1 (cos e0, -sin e0): the middle angle from both keeps its digits next to +-90 deg,
    // where asin(M[2]) loses half of them; below 64 deg asin is good to rounding and stays (the bits of every recorded run)
    e[1] = (fabs(M[2]) < 0.9) ? asin(M[2]) : atan2(M[2], sqrt(M[0] * M[0] + M[1] * M[1]));
    if (fabs(fabs(e[1]) - 0.5 * PI) <= 1e-7) {
        // gimbal lock, scipy's window and convention: the third angle is 0 and the first carries the combined rotation
        // (rows 1, 2 of M are [sin, cos, 0], [-+cos, +-sin, 0] of e0 +- e2); outside the window the two are separate
        e[0] = atan2(M[3], M[4]);
        e[2] = 0.0;
    } else {
        e[0] = atan2(-M[1], M[0]);
        e[2] = atan2(-M[5], M[8]);
    }
    // a half turn comes out as +pi or -pi depending on the SIGN OF A ZERO in M (structural zeros of the padded segments'
    // bases): made deterministic -- +pi -- here and in so3.compute_initial_rot_errors, where the reference's value is a coin flip
    if (fabs(fabs(e[0]) - PI) < 1e-12) e[0] = PI;
    if (fabs(fabs(e[2]) - PI) < 1e-12) e[2] = PI;
}

BMPC_INL void lp_mat3T(const double* A, double* T) {
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) T[3 * i + j] = A[3 * j + i];
}

// jac_SO3_inv_right (sign +1) / left (sign -1); angle = |axis| + 1e-6 (optimization_functions.py:37,54)
BMPC_INL void lp_jac_inv(const double* ax, double sign, double* J) {
    const double a = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]) + 1e-6;
    const double W[9] = {0, -ax[2], ax[1], ax[2], 0, -ax[0], -ax[1], ax[0], 0};
    double W2[9];
    mat3mul(W, W, W2);
    const double coef = 1.0 / (a * a) - (1.0 + cos(a)) / (2.0 * a * sin(a));
    for (int i = 0; i < 9; i++) J[i] = ((i % 4 == 0) ? 1.0 : 0.0) + sign * 0.5 * W[i] + coef * W2[i];
}

// integrate_rotation_reference (bound_mpc_functions.py:16-27)
BMPC_INL void lp_integrate_rot_ref(const double* pr_ref, const double* omega, double phi0, double phi1, double* out) {
    double r0[9], r1[9];
    lp_rotvec_to_mat(pr_ref, r0);
    const double n = sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2]);
    if (n > 1e-4) {
        const double w[3] = {omega[0] / n, omega[1] / n, omega[2] / n}, ph = (phi1 - phi0) * n;
        const double W[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
        double W2[9], Rr[9];
        mat3mul(W, W, W2);
        const double sp = sin(ph), cp = 1.0 - cos(ph);
        for (int i = 0; i < 9; i++) Rr[i] = ((i % 4 == 0) ? 1.0 : 0.0) + sp * W[i] + cp * W2[i];
        mat3mul(Rr, r0, r1);
    } else {
        for (int i = 0; i < 9; i++) r1[i] = r0[i];
    }
    lp_mat_to_rotvec(r1, out);
}

// compute_initial_rot_errors (bound_mpc_functions.py:30-46): e0, e_par, e_orth1, e_orth2
BMPC_INL void lp_initial_rot_errors(const double* pr, const double* pr_ref, const double* dpn, const double* br1,
                                    const double* br2, double* e0, double* epar, double* eo1, double* eo2) {
    double tc[9], td[9], tdT[9], m[9];
    lp_rotvec_to_mat(pr, tc);
    lp_rotvec_to_mat(pr_ref, td);
    lp_mat3T(td, tdT);
    mat3mul(tc, tdT, m);
    lp_mat_to_rotvec(m, e0);
    double r01[9], r01T[9], Rd[9], t1[9], d01[9], eul[3];
    for (int i = 0; i < 3; i++) { r01[3 * i] = br2[i]; r01[3 * i + 1] = dpn[i]; r01[3 * i + 2] = br1[i]; }
    lp_mat3T(r01, r01T);
    lp_rotvec_to_mat(e0, Rd);
    mat3mul(r01T, Rd, t1);
    mat3mul(t1, r01, d01);
    lp_euler_zyx(d01, eul);
    for (int i = 0; i < 3; i++) { epar[i] = eul[1] * dpn[i]; eo1[i] = eul[0] * br1[i]; eo2[i] = eul[2] * br2[i]; }
}

// X = G^{-1} Bt for 3x3 G, by elimination with partial pivoting (numpy.linalg.solve)
BMPC_INL void lp_solve3(const double* G, const double* Bt, double* X) {
    double A[3][6];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { A[i][j] = G[3 * i + j]; A[i][3 + j] = Bt[3 * i + j]; }
    for (int c = 0; c < 3; c++) {
        int piv = c;
        for (int r = c + 1; r < 3; r++) if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
        if (piv != c) for (int j = 0; j < 6; j++) { double t = A[c][j]; A[c][j] = A[piv][j]; A[piv][j] = t; }
        for (int r = c + 1; r < 3; r++) {
            const double f = A[r][c] / A[c][c];
            for (int j = c; j < 6; j++) A[r][j] -= f * A[c][j];
        }
    }
    for (int j = 0; j < 3; j++)
        for (int r = 2; r >= 0; r--) {
            double s = A[r][3 + j];
            for (int c = r + 1; c < 3; c++) s -= A[r][c] * X[3 * c + j];
            X[3 * r + j] = s / A[r][r];
        }
}

// ReferencePath.set_point (ReferencePath.py:160-185)
BMPC_INL void lp_set_point(double* S, int idx) {
    const int j = (int)S[LS_rp_sector] + idx;
    const double* dp = S + LS_rp_dp + 3 * j;
    const double nd = sqrt(dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2]);
    for (int c = 0; c < 3; c++) {
        S[LS_rp_pd + LP_S * c + idx] = S[LS_rp_p + 3 * j + c];
        S[LS_rp_pd + LP_S * (3 + c) + idx] = S[LS_rp_iw + 3 * j + c];
        S[LS_rp_r_taud + LP_S * c + idx] = S[LS_rp_r_tau + 3 * j + c];
        S[LS_rp_dpd + LP_S * c + idx] = dp[c] / nd;
        S[LS_rp_dpd + LP_S * (3 + c) + idx] = S[LS_rp_dr + 3 * j + c];
        S[LS_rp_dpdn + LP_S * c + idx] = S[LS_rp_drn + 3 * j + c];
    }
    double cs = 0;
    for (int i = 0; i <= j + 1; i++) cs += S[LS_rp_phi + i];
    S[LS_rp_phi_switch + idx + 1] = cs + S[LS_rp_phi_bias];
}

// ReferencePath.update (ReferencePath.py:187-207)
BMPC_INL void lp_path_update(double* S, bool sw) {
    if ((int)S[LS_rp_sector] >= (int)S[LS_rp_num_sectors] || !sw) return;
    S[LS_rp_sector] += 1;
    for (int c = 0; c < 6; c++)
        for (int i = 0; i < LP_S - 1; i++) {
            S[LS_rp_pd + LP_S * c + i] = S[LS_rp_pd + LP_S * c + i + 1];
            S[LS_rp_dpd + LP_S * c + i] = S[LS_rp_dpd + LP_S * c + i + 1];
        }
    for (int c = 0; c < 3; c++)
        for (int i = 0; i < LP_S - 1; i++) {
            S[LS_rp_r_taud + LP_S * c + i] = S[LS_rp_r_taud + LP_S * c + i + 1];
            S[LS_rp_dpdn + LP_S * c + i] = S[LS_rp_dpdn + LP_S * c + i + 1];
        }
    for (int i = 0; i < LP_S - 1; i++) S[LS_rp_phi_switch + i] = S[LS_rp_phi_switch + i + 1];
    S[LS_rp_phi_switch + LP_S - 1] = S[LS_rp_phi_switch + LP_S] + S[LS_rp_phi_bias];
    lp_set_point(S, LP_S - 1);
}

// ---- one scene per rollout (bmpc_loop_set_scenes) ----------------------------------------------------
// The obstacles of all scenes lie back to back in `all` (only the obstacles that exist); scene s owns obstacles first[s] ..
// first[s + 1] - 1.  Which scene a rollout looks at is configuration of the loop, not rollout state: scene[r], -1 = no obstacles.
struct LoopSceneTable {
    LoopScene all;        // n_obs = first[n_scenes]
    const int* first;     // [n_scenes + 1]
    const int* scene;     // [R]
    int n_scenes, max_obs;      // max_obs: the largest obstacle count of a scene = the stride of the closest-pair results
};

// the scene rollout r looks at, as the LoopScene the shared-scene code takes (n_obs = 0: obstacle-free collision sets)
BMPC_INL LoopScene loop_scene_of(const LoopSceneTable& t, int r) {
    const int s = t.scene[r];
    if (s < 0) return LoopScene{0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t o = (size_t)t.first[s];
    return LoopScene{t.first[s + 1] - (int)o, t.all.A + 45 * o, t.all.b + LP_ROWS * o, t.all.AAt + LP_ROWS * LP_ROWS * o, t.all.nrows + o,
                     t.all.V + 3 * LP_NV * o, t.all.nv + o, t.all.box + 6 * o, t.all.is_box + o};
}
// where the closest-pair results of rollout r start: blocks of the table's largest obstacle count, filled densely
// ([point][obstacle of the rollout's own scene], the layout loop_prepare reads)
BMPC_INL size_t loop_colres_of(const LoopSceneTable& t, int r) { return (size_t)r * 6 * t.max_obs * LP_CRES; }

// one (rollout, collision point, obstacle) of the closest-pair pass
BMPC_DEV void loop_collision_pair(const RobotConst* rc, const LoopScene& sc, const double* S, int pt, int ob, double* out) {
    Kin k0, kf;
    kin_eval(rc, S + LS_q, k0);
    kin_eval(rc, S + LS_qf, kf);
    loop_closest_pair(sc.A + 45 * ob, sc.b + LP_ROWS * ob, sc.AAt + LP_ROWS * LP_ROWS * ob, sc.nrows[ob],
                      sc.is_box[ob] ? sc.box + 6 * ob : nullptr, k0.pc[pt], kf.pc[pt], out);
}

// ---- before the solve: BoundMPC.step up to the solver call ---------------------------------------
// S: state; prev: previous solution row (read when has_prev); p/lbx/ubx: rows of the solver arguments
// (lbx/ubx hold the constant limits already, only the stage-0 pins are written here).
BMPC_DEV void loop_prepare(const RobotConst* rc, int N, double* S, const double* prev, double* p, double* lbx, double* ubx,
                           const LoopScene* sc = nullptr, const double* colres = nullptr) {
    // MPCNode.step: p_lie = fk(q) (MPCNode.py:118)
    Kin k;
    kin_eval(rc, S + LS_q, k);
    double p0[6];
    for (int c = 0; c < 3; c++) p0[c] = k.pee[c];
    lp_mat_to_rotvec(k.Ree, p0 + 3);
    for (int c = 0; c < 6; c++) S[LS_p_lie + c] = p0[c];

    lp_path_update(S, S[LS_sw] != 0.0);
    S[LS_sw] = 0.0;
    const int sec = (int)S[LS_rp_sector];

    // warm start: previous solution unshifted, with the omega-reversal patch (BoundMPC.py:418-428)
    S[LS_patch] = 0.0;
    if (S[LS_has_prev] != 0.0) {
        double d[3], n2 = 0;
        for (int c = 0; c < 3; c++) { d[c] = p0[3 + c] - prev[28 * N + (3 + c) * N]; n2 += d[c] * d[c]; }
        if (sqrt(n2) > 1.5) {
            S[LS_patch] = 1.0;
            for (int c = 0; c < 3; c++) S[LS_patch_delta + c] = d[c];
        }
    }

    // initial orientation errors per segment (BoundMPC.py:436-462)
    for (int i = 0; i < LP_S; i++) {
        double prs[3], dpn[3];
        for (int c = 0; c < 3; c++) {
            prs[c] = (i == 0) ? S[LS_pr_ref + c] : S[LS_rp_r_taud + LP_S * c + i];
            dpn[c] = S[LS_rp_dpdn + LP_S * c + i];
        }
        lp_initial_rot_errors(p0 + 3, prs, dpn, S + LS_rp_br1 + 3 * (sec + i), S + LS_rp_br2 + 3 * (sec + i),
                              S + LS_dtau + 3 * i, S + LS_dtau_par + 3 * i, S + LS_dtau_o1 + 3 * i, S + LS_dtau_o2 + 3 * i);
    }
    // projection vectors (BoundMPC.py:338-386); one jac_dtau_l/r from segment 0 serves all segments
    lp_jac_inv(S + LS_dtau, +1.0, S + LS_jac_r);
    lp_jac_inv(S + LS_dtau, -1.0, S + LS_jac_l);
    double rinit0[9];
    lp_rotvec_to_mat(S + LS_dtau, rinit0);
    for (int i = 0; i < LP_S; i++) {
        double Ro[9], RoT[9], rest1[9], Rp[9], RpT[9], rest2[9], rv[3], j1[9], j2[9], dpn[3];
        lp_rotvec_to_mat(S + LS_dtau_o1 + 3 * i, Ro);
        lp_mat3T(Ro, RoT);
        mat3mul(rinit0, RoT, rest1);
        lp_rotvec_to_mat(S + LS_dtau_par + 3 * i, Rp);
        lp_mat3T(Rp, RpT);
        mat3mul(rest1, RpT, rest2);
        lp_mat_to_rotvec(rest1, rv);
        lp_jac_inv(rv, +1.0, j1);
        lp_mat_to_rotvec(rest2, rv);
        lp_jac_inv(rv, +1.0, j2);
        for (int c = 0; c < 3; c++) dpn[c] = S[LS_rp_dpdn + LP_S * c + i];
        double g[3], h[3], kk[3];
        mat3vec(S + LS_jac_r, S + LS_rp_br1 + 3 * (sec + i), g);
        mat3vec(j1, dpn, h);
        mat3vec(j2, S + LS_rp_br2 + 3 * (sec + i), kk);
        double Bt[9], G[9], X[9];      // Bt = Bm^T with Bm = [g h k] columns
        for (int c = 0; c < 3; c++) { Bt[c] = g[c]; Bt[3 + c] = h[c]; Bt[6 + c] = kk[c]; }
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) G[3 * a + b] = Bt[3 * a] * Bt[3 * b] + Bt[3 * a + 1] * Bt[3 * b + 1] + Bt[3 * a + 2] * Bt[3 * b + 2];
        lp_solve3(G, Bt, X);
        for (int c = 0; c < 3; c++) {
            S[LS_v1 + LP_S * c + i] = X[c]; S[LS_v2 + LP_S * c + i] = X[3 + c]; S[LS_v3 + LP_S * c + i] = X[6 + c];
        }
    }

    // Q10: w_phi rescale only when phi_max < 1; phi target clamped to phi + 5 (BoundMPC.py:465-478)
    const double phi_max = S[LS_phi_max], phi_cur = S[LS_phi_current];
    double w4 = S[LS_weights + 4];
    if (phi_max < 1 && phi_max > 0.001) w4 *= fmin(1.0 / ((phi_max - phi_cur) * (phi_max - phi_cur)), 2.0);
    const double phi_clamped = fmin(phi_cur + 5.0, phi_max);

    // ---- the 875 parameters in the order of BoundMPC.py:507-542 ----
    for (int i = 0; i < 5; i++) p[P_SPLIT + i] = S[LS_split + i];
    for (int i = 0; i < 6; i++) p[P_SLACKS0 + i] = S[LS_slacks0 + i];
    for (int i = 0; i < 3; i++) p[P_IWREF + i] = S[LS_iw_ref + i];
    for (int i = 0; i < 12; i++) {
        p[P_DTAU + i] = S[LS_dtau + i]; p[P_DTAU_PAR + i] = S[LS_dtau_par + i];
        p[P_DTAU_O1 + i] = S[LS_dtau_o1 + i]; p[P_DTAU_O2 + i] = S[LS_dtau_o2 + i];
        p[P_DPN + i] = S[LS_rp_dpdn + i];
        p[P_V1 + i] = S[LS_v1 + i]; p[P_V2 + i] = S[LS_v2 + i]; p[P_V3 + i] = S[LS_v3 + i];
    }
    p[P_XPHID] = phi_clamped; p[P_XPHID + 1] = 0.0; p[P_XPHID + 2] = 0.0;
    for (int i = 0; i < 5; i++) p[P_PHISW + i] = S[LS_rp_phi_switch + i];
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) { p[P_JACR + 3 * a + b] = S[LS_jac_r + 3 * b + a]; p[P_JACL + 3 * a + b] = S[LS_jac_l + 3 * b + a]; }
    for (int i = 0; i < 24; i++) { p[P_PREF + i] = S[LS_rp_pd + i]; p[P_DPREF + i] = S[LS_rp_dpd + i]; }
    for (int c = 0; c < 3; c++)
        for (int i = 0; i < LP_S; i++) {
            p[P_BP1 + LP_S * c + i] = S[LS_rp_bp1 + 3 * (sec + i) + c]; p[P_BP2 + LP_S * c + i] = S[LS_rp_bp2 + 3 * (sec + i) + c];
            p[P_BR1 + LP_S * c + i] = S[LS_rp_br1 + 3 * (sec + i) + c]; p[P_BR2 + LP_S * c + i] = S[LS_rp_br2 + 3 * (sec + i) + c];
        }
    for (int c = 0; c < 6; c++)
        for (int i = 0; i < LP_S; i++) p[P_ERB + LP_S * c + i] = S[LS_rp_erb + 6 * (sec + i) + c];
    for (int i = 0; i < 11; i++) p[P_W + i] = (i == 4) ? w4 : S[LS_weights + i];
    p[P_PHIMAX] = phi_clamped;
    for (int i = 0; i < 7; i++) p[P_V3 + 12 + i] = 0.0;      // qd (unused desired joint configuration, BoundMPC.py:66)
    for (int i = 0; i < LP_S; i++)
        for (int c = 0; c < 3; c++)
            for (int r = 0; r < LP_ROWS; r++) p[P_ASET + 45 * i + LP_ROWS * c + r] = S[LS_rp_a + 45 * (sec + i) + 3 * r + c];
    for (int r = 0; r < LP_ROWS; r++)
        for (int i = 0; i < LP_S; i++) p[P_BSET + LP_S * r + i] = S[LS_rp_b + LP_ROWS * (sec + i) + r];
    // collision sets: 0.7 m box around each collision point at q0 (ConvexSetFinder.py:400-421), separating halfspaces
    // of the scene's obstacles along the segment to the point's position at qf, everything shrunk by the joint size,
    // padded with (A = 0, b = 10) (BoundMPC.py:480-497, util_functions.py:121-135)
    const bool obst = sc && sc->n_obs > 0;
    Kin kf;
    if (obst) kin_eval(rc, S + LS_qf, kf);
    for (int j = 0; j < 6; j++) {
        double a[LP_ROWS][3], b[LP_ROWS];
        for (int r = 0; r < 6; r++) {
            for (int c = 0; c < 3; c++) a[r][c] = ((r >> 1) == c) ? ((r & 1) ? -1.0 : 1.0) : 0.0;
            b[r] = ((r & 1) ? -k.pc[j][r >> 1] : k.pc[j][r >> 1]) + 0.7;
        }
        int n = 6;
        if (obst) {
            const double* res = colres + LP_CRES * sc->n_obs * j;      // the closest pairs of this point, [obstacle][LP_CRES]
            bool touched;
            n = separating_halfspaces(*sc, [res](int i) { return res + LP_CRES * i; }, res + 6, LP_CRES, k.pc[j], kf.pc[j], LP_ROWS,
                                      &a[0][0], b, n, touched);
            if (n == FS_OVERFLOW) { S[LS_dead] = 2.0; n = LP_ROWS; }       // more rows than max_set_size: the host raises
            if (n == FS_NUMERICAL) { S[LS_dead] = 3.0; n = 6; }            // an obstacle without a closest pair (empty to rounding)
        }
        for (int c = 0; c < 3; c++)
            for (int r = 0; r < LP_ROWS; r++) p[P_ASETJ + 45 * j + LP_ROWS * c + r] = (r < n) ? a[r][c] : 0.0;
        for (int r = 0; r < LP_ROWS; r++) p[P_BSETJ + 6 * r + j] = (r < n) ? b[r] - rc->colsize[j] : 10.0;
    }

    // stage-0 pins (BoundMPC.py:544-580, Q7): x[0:-1:N] = value on the joint-major arrays
    for (int j = 0; j < 7; j++) {
        lbx[j * N] = ubx[j * N] = S[LS_q + j];
        lbx[7 * N + j * N] = ubx[7 * N + j * N] = S[LS_dq + j];
        lbx[14 * N + j * N] = ubx[14 * N + j * N] = S[LS_ddq + j];
        lbx[21 * N + j * N] = ubx[21 * N + j * N] = S[LS_jerk + j];
    }
    for (int j = 0; j < 6; j++) {
        lbx[28 * N + j * N] = ubx[28 * N + j * N] = p0[j];
        lbx[34 * N + j * N] = ubx[34 * N + j * N] = S[LS_v + j];
    }
}

// constant part of the bounds (BoundMPC.py:171-191, 544-589); infinities as +-1e20
BMPC_INL void loop_bound_const(const RobotConst* rc, int N, int i, double* lo, double* hi) {
    double l = 0.0, h = 1e20;
    if (i < 7 * N) { h = rc->q_hi[i / N]; l = rc->q_lo[i / N]; }
    else if (i < 14 * N) { h = rc->dq_max[(i - 7 * N) / N]; l = -h; }
    else if (i < 21 * N) { h = rc->ddq_max; l = -h; }
    else if (i < 28 * N) { h = rc->u_max; l = -h; }
    else if (i < 40 * N) { h = 1e20; l = -1e20; }
    *lo = l; *hi = h;
}

// element i of the start vector: cold start (BoundMPC.py:412-416) or the patched previous solution
BMPC_INL double loop_x0_elem(int N, const double* S, const double* prev, int i) {
    if (S[LS_has_prev] == 0.0) {
        if (i < 7 * N) return S[LS_q + i / N];
        if (i >= 28 * N && i < 34 * N) return S[LS_p_lie + (i - 28 * N) / N];
        return 0.0;
    }
    if (S[LS_patch] != 0.0 && i >= 31 * N && i < 34 * N) {
        const int c = (i - 31 * N) / N, col = (i - 31 * N) - c * N;
        const int src = (col < N - 1) ? col + 1 : N - 1;
        return prev[31 * N + c * N + src] + S[LS_patch_delta + c];
    }
    return prev[i];
}

BMPC_INL int lp_segment(int idx, const double* split, int n_rows) {
    int i = 0;
    for (int j = 0; j < n_rows - 2; j++) if (idx > (int)split[j + 1]) i = j + 1;
    return i;
}

// ---- after the solve: acceptance, compute_return_data, joint integration ---------------------------
// x: the solver's solution row; prev: the stored previous solution row (read only here; the caller copies
// x over it afterwards where S[LS_accept] is set); log: LP_LOGW doubles or null.
BMPC_DEV void loop_finish(const RobotConst* rc, int N, double dt, double* S, const double* x, const double* prev,
                          int status, double viol, int iters, double* log, double* rec = nullptr, const double* par = nullptr) {
    const int n_w = 44 * N + 6;
    S[LS_steps] += 1.0;
    for (int i = 0; i < 6; i++) S[LS_slacks0 + i] += x[n_w - 6 + i];          // Q1
    const bool success = (status == 0) || (viol < 1e-4);                         // Q8
    const double* w = x;
    S[LS_accept] = 0.0;
    if (!success) {
        S[LS_error_count] += 1.0;
        if (S[LS_has_prev] != 0.0) w = prev;
        else S[LS_error_count] = 0.0;
    } else {
        S[LS_error_count] = 0.0;
        S[LS_accept] = 1.0;
        S[LS_has_prev] = 1.0;
    }
    const int ec = (int)S[LS_error_count], n = N - ec;
    if (log) {
        for (int i = 0; i < LP_LOGW; i++) log[i] = 0.0;
        log[0] = (double)iters; log[1] = (double)status; log[2] = viol; log[3] = (double)ec;
    }
    if (rec) {
        const int nr = lp_rec_doubles(N);
        for (int i = 0; i < nr; i++) rec[i] = 0.0;
        rec[0] = (double)iters; rec[1] = (double)status; rec[2] = viol; rec[3] = (double)ec; rec[4] = (double)(n < 0 ? 0 : n);
        rec[5] = S[LS_rp_sector]; rec[6] = S[LS_phi_max];
        for (int i = 0; i < 5; i++) rec[7 + i] = S[LS_split + i];
        if (par) for (int i = 0; i < LP_REC_SETS; i++) rec[LP_REC_HDR + LP_REC_STAGE * N + i] = par[275 + i];
    }
    if (n < 2) { S[LS_dead] = 1.0; if (log) log[4] = 1.0; return; }   // the reference would index past its arrays here

    const int sec = (int)S[LS_rp_sector];
    double split_prev[5], iw_ref_0[3];
    for (int i = 0; i < 5; i++) split_prev[i] = S[LS_split + i];
    for (int c = 0; c < 3; c++) iw_ref_0[c] = S[LS_iw_ref + c];
    const int nxt = ((int)split_prev[1] == N) ? 1 : (((int)split_prev[2] == N) ? 2 : 3);
    if (rec) rec[12] = (double)nxt;

    double opt_phi[LP_NMAX], ers[LP_NMAX][3], ersn[LP_NMAX][3];
    signed char segs[LP_NMAX];
    double opt_dphi1 = 0.0;
    for (int i = 0; i < n; i++) {
        double pp[6], vv[6];
        for (int c = 0; c < 6; c++) { pp[c] = w[28 * N + c * N + ec + i]; vv[c] = w[34 * N + c * N + ec + i]; }
        const int s = lp_segment(i, split_prev, LP_S);
        const double phi_start = S[LS_rp_phi_switch + lp_segment(i, split_prev, LP_S + 1)];
        double pc[6], pn[6], dpd[6], dpn_[6];
        for (int c = 0; c < 6; c++) {
            pc[c] = S[LS_rp_pd + LP_S * c + s]; pn[c] = S[LS_rp_pd + LP_S * c + s + 1];
            dpd[c] = S[LS_rp_dpd + LP_S * c + s]; dpn_[c] = S[LS_rp_dpd + LP_S * c + s + 1];
        }
        double phi_l = 0, phi_next = 0, dphi = 0;
        for (int c = 0; c < 3; c++) { phi_l += (pp[c] - pc[c]) * dpd[c]; phi_next += (pp[c] - pn[c]) * dpn_[c]; dphi += vv[c] * dpd[c]; }
        double pdr[3], pdrn[3], iw0[3], t1[3], t2[3], dl[3], a1[3], a2[3];
        for (int c = 0; c < 3; c++) {
            pdr[c] = dpd[3 + c] * phi_l + pc[3 + c];
            pdrn[c] = dpn_[3 + c] * phi_next + pn[3 + c];
            iw0[c] = (i <= (int)split_prev[1]) ? iw_ref_0[c] : pc[3 + c];
            t1[c] = pp[3 + c] - S[LS_p_lie + 3 + c];
        }
        mat3vec(S + LS_jac_l, t1, dl);
        for (int c = 0; c < 3; c++) { t1[c] = pdr[c] - iw0[c]; t2[c] = pdrn[c] - iw0[c]; }
        mat3vec(S + LS_jac_r, t1, a1);
        mat3vec(S + LS_jac_r, t2, a2);
        // d = e_r - e_init, dn = e_rn - e_initn (evaluated as in the reference: sum first, then subtract)
        double d[3], dn[3];
        for (int c = 0; c < 3; c++) {
            const double ei = S[LS_dtau + 3 * s + c], ein = S[LS_dtau + 3 * nxt + c];
            d[c] = (ei + dl[c] - a1[c]) - ei;
            dn[c] = (ein + dl[c] - a2[c]) - ein;
        }
        const double* br1 = S + LS_rp_br1 + 3 * (sec + s);
        const double* br2 = S + LS_rp_br2 + 3 * (sec + s);
        const double* br1n = S + LS_rp_br1 + 3 * (sec + s + 1);
        const double* br2n = S + LS_rp_br2 + 3 * (sec + s + 1);
        double dv[6] = {0, 0, 0, 0, 0, 0}, dpnv[3], dpnn[3];
        for (int c = 0; c < 3; c++) {
            dpnv[c] = S[LS_rp_dpdn + LP_S * c + s]; dpnn[c] = S[LS_rp_dpdn + LP_S * c + s + 1];
            dv[0] += d[c] * S[LS_v1 + LP_S * c + s]; dv[1] += d[c] * S[LS_v2 + LP_S * c + s]; dv[2] += d[c] * S[LS_v3 + LP_S * c + s];
            dv[3] += dn[c] * S[LS_v1 + LP_S * c + s + 1]; dv[4] += dn[c] * S[LS_v2 + LP_S * c + s + 1]; dv[5] += dn[c] * S[LS_v3 + LP_S * c + s + 1];
        }
        double e[6] = {0, 0, 0, 0, 0, 0};     // orth1, par, orth2, then the next-segment variants
        for (int c = 0; c < 3; c++) {
            e[0] += (S[LS_dtau_o1 + 3 * s + c] + dv[0] * br1[c]) * br1[c];
            e[1] += (S[LS_dtau_par + 3 * s + c] + dv[1] * dpnv[c]) * dpnv[c];
            e[2] += (S[LS_dtau_o2 + 3 * s + c] + dv[2] * br2[c]) * br2[c];
            e[3] += (S[LS_dtau_o1 + 3 * (s + 1) + c] + dv[3] * br1n[c]) * br1n[c];
            e[4] += (S[LS_dtau_par + 3 * (s + 1) + c] + dv[4] * dpnn[c]) * dpnn[c];
            e[5] += (S[LS_dtau_o2 + 3 * (s + 1) + c] + dv[5] * br2n[c]) * br2n[c];
        }
        if (rec) {
            double* q_ = rec + LP_REC_HDR + LP_REC_STAGE * i;
            for (int c = 0; c < 6; c++) { q_[c] = pp[c]; q_[6 + c] = vv[c]; }
            for (int j = 0; j < 7; j++) {
                q_[12 + j] = w[j * N + ec + i]; q_[19 + j] = w[7 * N + j * N + ec + i];
                q_[26 + j] = w[14 * N + j * N + ec + i]; q_[33 + j] = w[21 * N + j * N + ec + i];
            }
            q_[40] = phi_l + phi_start; q_[41] = dphi;
            double lv[3], rv[3], wv[3] = {vv[3], vv[4], vv[5]}, rd[3] = {dpd[3] * dphi, dpd[4] * dphi, dpd[5] * dphi};
            mat3vec(S + LS_jac_l, wv, lv);
            mat3vec(S + LS_jac_r, rd, rv);
            for (int c = 0; c < 3; c++) {
                q_[42 + c] = pp[c] - (pc[c] + dpd[c] * phi_l);             // e_p
                q_[45 + c] = vv[c] - dpd[c] * dphi;                          // de_p
                q_[48 + c] = S[LS_dtau + 3 * s + c] + dl[c] - a1[c];         // e_r
                q_[51 + c] = lv[c] - rv[c];                                  // de_r
                q_[54 + c] = e[c];                                           // e_r_orth1, e_r_par, e_r_orth2
                q_[57 + c] = pc[c] + dpd[c] * phi_l; q_[60 + c] = pdr[c];    // p_ref
            }
            q_[63] = (double)s;
        }
        opt_phi[i] = phi_l + phi_start;
        if (i == 1) opt_dphi1 = dphi;
        for (int c = 0; c < 3; c++) { ers[i][c] = e[c]; ersn[i][c] = e[3 + c]; }
        segs[i] = (signed char)s;
    }

    // rotation reference integrated to the path parameter of stage 1 (BoundMPC.py:894-914)
    {
        const int j = ((int)S[LS_split + 1] == 1) ? 1 : 0;
        double om[3], pr[3];
        for (int c = 0; c < 3; c++) om[c] = S[LS_rp_dpd + LP_S * (3 + c) + j];
        lp_integrate_rot_ref(S + LS_rp_r_tau + 3 * (sec + j), om, S[LS_rp_phi_switch + j], opt_phi[1], pr);
        if (rec) for (int c = 0; c < 3; c++) rec[LP_REC_HDR + 60 + c] = pr[c];      // ref_data["p"][0][3:] = pr_ref (BoundMPC.py:1023)
        for (int c = 0; c < 3; c++) {
            S[LS_pr_ref + c] = pr[c];
            S[LS_iw_ref + c] = S[LS_rp_pd + LP_S * (3 + c) + j] + (opt_phi[1] - S[LS_rp_phi_switch + j]) * om[c];
        }
    }

    // split indices: countdown of a set switch, or detection of a new one (BoundMPC.py:916-1021)
    const double IN_SET = 0.005, ROT_M = 5 * 3.141592653589793 / 180, PHI_M = 0.03;
    bool sw = S[LS_sw] != 0.0;
    for (int i = 1; i < LP_S - 1; i++) {
        if ((int)S[LS_split + i] < N) {
            S[LS_split + i] -= 1.0;
            if ((int)S[LS_split + i] == 0) { sw = true; S[LS_split + i] = N; }
        } else if (ec == 0) {
            const double* a0 = S + LS_rp_a + 45 * (sec + i - 1);
            const double* b0 = S + LS_rp_b + LP_ROWS * (sec + i - 1);
            const double* a1 = S + LS_rp_a + 45 * (sec + i);
            const double* b1 = S + LS_rp_b + LP_ROWS * (sec + i);
            int last_out = -1;
            unsigned long long m_all = 0ull, m_set1 = 0ull;
            for (int kx = 0; kx < n; kx++) {
                const double px = w[28 * N + kx], py = w[29 * N + kx], pz = w[30 * N + kx], ps = w[n_w - 2 * N + kx];
                double d0 = -1e300, d1 = -1e300;
                for (int r = 0; r < LP_ROWS; r++) {
                    d0 = fmax(d0, a0[3 * r] * px + a0[3 * r + 1] * py + a0[3 * r + 2] * pz - b0[r]);
                    d1 = fmax(d1, a1[3 * r] * px + a1[3 * r + 1] * py + a1[3 * r + 2] * pz - b1[r]);
                }
                const bool in0 = d0 < IN_SET + ps, in1 = d1 < IN_SET + ps;
                if (!in1) last_out = kx;
                const int s = segs[kx];
                const double* up = S + LS_rp_erb + 6 * (sec + s);
                const double* upn = S + LS_rp_erb + 6 * (sec + s + 1);
                bool rot = true;
                for (int c = 0; c < 3; c++)
                    rot = rot && (ers[kx][c] < up[c]) && (ers[kx][c] > up[3 + c]) && (ersn[kx][c] < upn[c] + ROT_M) && (ersn[kx][c] > upn[3 + c] - ROT_M);
                const bool dsw = opt_phi[kx] > S[LS_rp_phi_switch + i] - PHI_M;
                if (dsw && in0 && rot) m_all |= 1ull << kx;
                if (in1) m_set1 |= 1ull << kx;
            }
            // only the trailing run of in-set stages counts for the next set
            int idx_new = -1;
            for (int kx = (last_out < 0 ? 0 : last_out); kx < n; kx++)
                if (((m_all >> kx) & 1ull) && ((m_set1 >> kx) & 1ull)) { idx_new = kx; break; }
            const bool not_at_end = sec + (i - 1) < (int)S[LS_rp_num_sectors];
            if (idx_new >= 0 && not_at_end) {
                if ((int)S[LS_split + i] == N) {
                    S[LS_split + i] = idx_new - 1;
                    // move the via point onto the switching position (BoundMPC.py:989-1011)
                    double dp[3], pv[3], corr = 0;
                    for (int c = 0; c < 3; c++) { dp[c] = S[LS_rp_dpd + LP_S * c + i]; pv[c] = S[LS_rp_pd + LP_S * c + i]; }
                    for (int c = 0; c < 3; c++) corr += (w[28 * N + c * N + idx_new] - pv[c]) * dp[c];
                    for (int c = 0; c < 3; c++) {
                        const double nv = pv[c] + corr * dp[c];
                        S[LS_rp_pd + LP_S * c + i] = nv;
                        S[LS_rp_p + 3 * (sec + i) + c] = nv;
                    }
                    S[LS_rp_phi + sec + i + 1] -= corr;
                    for (int q = i + 1; q < LP_S + 1; q++) S[LS_rp_phi_switch + q] -= corr;
                    double cs = 0;
                    for (int q = 0; q <= (int)S[LS_rp_num_sectors] + 1; q++) cs += S[LS_rp_phi + q];
                    S[LS_rp_phi_max] = cs + S[LS_rp_phi_bias];
                    S[LS_phi_max] = S[LS_rp_phi_max];
                }
                if ((int)S[LS_split + i] == 0) sw = true;
            }
        }
    }
    if (sw) {
        for (int i = 1; i < LP_S; i++) S[LS_split + i] = S[LS_split + i + 1];
        S[LS_split + LP_S] = N;
    }
    S[LS_sw] = sw ? 1.0 : 0.0;
    for (int i = 1; i < LP_S; i++)
        if (S[LS_split + i] <= S[LS_split + i - 1]) S[LS_split + i] = fmin((double)N, S[LS_split + i - 1] + 1.0);
    S[LS_phi_current] = opt_phi[1];
    S[LS_dphi_current] = opt_dphi1;

    // integrate_joint over one sampling interval (only the first two jerk hats reach t = dt) with the
    // closed forms of jerk_trajectory_casadi.py:78-175, then MPCNode.step's state advance
    {
        const double h = dt, t = dt;
        Kin k0;
        double J[6][7], G[6][7], vold[6], qn[7], dqn[7], ddqn[7];
        kin_eval(rc, S + LS_q, k0);
        kin_jac(k0, S + LS_dq, J, G, vold);       // v = J(q) dq at the OLD state (util_functions.py:61-62)
        for (int j = 0; j < 7; j++) {
            const double j0 = w[21 * N + j * N + ec], j1 = w[21 * N + j * N + ec + 1];
            double acc = 0, vel = 0, ang = 0;
            acc += -j0 * t * (t - 2 * h) / h / 2;
            vel += -j0 * t * t * (t - 3 * h) / h / 6;
            ang += -j0 * t * t * t * (t - 4 * h) / h / 24;
            acc += j1 * (t * t) / h / 2;
            vel += -j1 * ((0.0 - t) * (0.0 - t) * (0.0 - t)) / h / 6;
            ang += j1 * ((0.0 - t) * (0.0 - t) * (0.0 - t) * (0.0 - t)) / h / 24;
            const double q = S[LS_q + j], dq = S[LS_dq + j], ddq = S[LS_ddq + j];
            qn[j] = ddq * (t * t) / 2 + dq * t + q + ang;
            dqn[j] = ddq * t + dq + vel;
            ddqn[j] = ddq + acc;
        }
        for (int j = 0; j < 7; j++) {
            S[LS_q + j] = qn[j]; S[LS_dq + j] = dqn[j]; S[LS_ddq + j] = ddqn[j];
            S[LS_qf + j] = w[j * N + N - 1];
            S[LS_jerk + j] = w[21 * N + j * N + ec + 1];
        }
        for (int c = 0; c < 6; c++) S[LS_v + c] = vold[c];
        Kin k1;
        kin_eval(rc, qn, k1);
        for (int c = 0; c < 3; c++) S[LS_p_lie + c] = k1.pee[c];
        lp_mat_to_rotvec(k1.Ree, S + LS_p_lie + 3);
    }
    if (rec) rec[6] = S[LS_phi_max];          // after the via-point adaptation of this step
    if (log) {
        log[5] = S[LS_phi_current]; log[6] = S[LS_phi_max]; log[7] = S[LS_split + 1]; log[8] = (double)sec; log[9] = sw ? 1.0 : 0.0;
        for (int c = 0; c < 6; c++) log[10 + c] = S[LS_p_lie + c];
        for (int j = 0; j < 7; j++) log[16 + j] = S[LS_q + j];
    }
}

// ---- installing a reference path: ReferencePath.__init__ + BoundMPC.update / __init__ + pack_state -------------------
// One rollout gets a new via path on the device.  The host code is the specification -- ReferencePath.__init__
// (boundplanner_amd/reference_path.py), BoundMPC.update / __init__ (bound_mpc.py) and pack_state (device_loop.py) -- and the state
// vector afterwards is what pack_state would have written, including what looks accidental there: the padded list entries, the
// in-place normalisation of the dp entries that share an object with entry 0 or 1, the padded dr entries that keep the undivided
// increment, zeros in every field pack_state does not write.  The lists are built in S itself (no local array indexed by a runtime
// value); the record is read where the caller staged it.
constexpr int LP_MAXPTS = 8;     // via points of a path, at most (LP_NL = LP_MAXPTS + LP_S - 1)
enum LoopInstallMode { LP_INSTALL_REPLAN = 0, LP_INSTALL_FRESH = 1 };

BMPC_INL double lp_norm3(const double* a) { return sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }

// orthonormal pair around the unit direction d: b1 = the part of `want` orthogonal to d ([1,1,1] when want is parallel to d),
// b2 = d x b1 (ReferencePath.py:109-150)
BMPC_INL void lp_basis_pair(const double* d, const double* want, double* b1, double* b2) {
    double s = d[0] * want[0] + d[1] * want[1] + d[2] * want[2];
    double b[3] = {want[0] - s * d[0], want[1] - s * d[1], want[2] - s * d[2]};
    if (lp_norm3(b) < 1e-3) {
        s = d[0] + d[1] + d[2];
        for (int c = 0; c < 3; c++) b[c] = 1.0 - s * d[c];
    }
    const double nb = lp_norm3(b);
    for (int c = 0; c < 3; c++) b[c] /= nb;
    const double x[3] = {d[1] * b[2] - d[2] * b[1], d[2] * b[0] - d[0] * b[2], d[0] * b[1] - d[1] * b[0]};
    const double nx = lp_norm3(x);
    for (int c = 0; c < 3; c++) { b1[c] = b[c]; b2[c] = x[c] / nx; }
}

// rows n_real .. n_real + LP_S - 2 of a list of `w` doubles per row: copies of row n_real - 1
BMPC_INL void lp_pad_rows(double* list, int w, int n_real) {
    for (int k = 0; k < LP_S - 1; k++)
        for (int c = 0; c < w; c++) list[w * (n_real + k) + c] = list[w * (n_real - 1) + c];
}

// LP_INSTALL_REPLAN: DeviceLoop.replan -- the record is n_pts in 2..8, p_via [n_pts][3], r_via [n_pts][9] row-major,
//   bp1 / br1 [n_pts-1][3], e_r_bound [n_pts-1][6], a_sets [n_pts-1][15][3], b_sets [n_pts-1][15]; q0 / weights unused.
//   q, dq, ddq, jerk, v, p_lie, slacks0, error_count, has_prev, weights carry over.
// LP_INSTALL_FRESH: BatchMPCNode.__init__ + DeviceLoop.set_rollout for the start configuration q0 [7] with weights [11] -- the
//   rollout at rest on the trivial path [p0, p0]; the record is unused.
BMPC_DEV void loop_install_path(const RobotConst* rc, int N, double* S, int mode, int n_pts, const double* p_via, const double* r_via,
                                const double* bp1, const double* br1, const double* e_r_bound, const double* a_sets, const double* b_sets,
                                const double* q0, const double* weights) {
    const double PI = 3.141592653589793;
    const bool fresh = mode == LP_INSTALL_FRESH;
    if (fresh) {
        for (int j = 0; j < 7; j++) { S[LS_q + j] = q0[j]; S[LS_dq + j] = 0.0; S[LS_ddq + j] = 0.0; S[LS_jerk + j] = 0.0; }
        for (int c = 0; c < 6; c++) { S[LS_v + c] = 0.0; S[LS_slacks0 + c] = 0.0; }
        Kin k;
        kin_eval(rc, S + LS_q, k);
        for (int c = 0; c < 3; c++) S[LS_p_lie + c] = k.pee[c];
        lp_mat_to_rotvec(k.Ree, S + LS_p_lie + 3);
        S[LS_error_count] = 0.0; S[LS_has_prev] = 0.0;
        for (int i = 0; i < 11; i++) S[LS_weights + i] = weights[i];
    } else {
        S[LS_error_count] = (double)(int)S[LS_error_count];       // (the host carries it as an int)
        S[LS_has_prev] = (S[LS_has_prev] != 0.0) ? 1.0 : 0.0;
    }
    for (int j = 0; j < 7; j++) S[LS_qf + j] = S[LS_q + j];
    // what neither mode keeps: pack_state starts from zeros
    for (int i = LS_split; i < LS_error_count; i++) S[i] = 0.0;
    for (int i = LS_pr_ref; i < LS_weights; i++) S[i] = 0.0;
    for (int i = LS_dtau; i < LS_SIZE; i++) S[i] = 0.0;

    const int n = fresh ? 2 : n_pts;
    unsigned same0 = 0u, same1 = 0u;       // bit i: list entry dp[i] is the same host object as dp[0] / dp[1]
    double phi_sum = 0.0;
    if (fresh) {
        for (int i = 0; i < 2 + LP_S - 1; i++)
            for (int c = 0; c < 3; c++) { S[LS_rp_p + 3 * i + c] = S[LS_p_lie + c]; S[LS_rp_r_tau + 3 * i + c] = S[LS_p_lie + 3 + c]; }
        for (int i = 0; i < 1 + LP_S - 1; i++) {      // one segment without length or rotation: the defaults of ReferencePath
            S[LS_rp_drn + 3 * i + 1] = 1.0; S[LS_rp_dp + 3 * i + 1] = 1.0;
            S[LS_rp_bp1 + 3 * i] = 1.0; S[LS_rp_br1 + 3 * i] = 1.0; S[LS_rp_bp2 + 3 * i + 2] = -1.0; S[LS_rp_br2 + 3 * i + 2] = -1.0;
            for (int c = 0; c < 6; c++) S[LS_rp_erb + 6 * i + c] = (c < 3 ? 90.0 : -90.0) * PI / 180.0;
            for (int r = 0; r < LP_ROWS; r++) S[LS_rp_b + LP_ROWS * i + r] = 1.0;
        }
    } else {
        // via points and orientations (ReferencePath.py:43-76); the orientation increments stay undivided for now
        for (int i = 0; i < n; i++) {
            for (int c = 0; c < 3; c++) S[LS_rp_p + 3 * i + c] = p_via[3 * i + c];
            lp_mat_to_rotvec(r_via + 9 * i, S + LS_rp_r_tau + 3 * i);
        }
        double ax[3] = {0.0, 1.0, 0.0};
        for (int i = 1; i < n; i++) {
            double rT[9], m[9], d[3];
            lp_mat3T(r_via + 9 * (i - 1), rT);
            mat3mul(r_via + 9 * i, rT, m);
            lp_mat_to_rotvec(m, d);
            const double nrm = lp_norm3(d);
            if (nrm > 1e-4) {
                const double a[3] = {d[0] / nrm, d[1] / nrm, d[2] / nrm}, s[3] = {ax[0] + a[0], ax[1] + a[1], ax[2] + a[2]};
                const double sg = (lp_norm3(s) < 1e-4) ? -1.0 : 1.0;       // keep the projection axis on reversal
                for (int c = 0; c < 3; c++) ax[c] = sg * a[c];
            }
            for (int c = 0; c < 3; c++) {
                S[LS_rp_dr + 3 * (i - 1) + c] = d[c];
                S[LS_rp_drn + 3 * (i - 1) + c] = ax[c];
                S[LS_rp_iw + 3 * i + c] = S[LS_rp_iw + 3 * (i - 1) + c] + d[c];
            }
        }
        // position increments and arc lengths (ReferencePath.py:78-106).  A segment shorter than 1e-3 IS the entry before it on
        // the host (the same object), the padded entries are the last real one: root = the entry whose object entry i holds
        int root = 0, root1 = 0;
        for (int i = 0; i < n - 1; i++) {
            double d[3] = {p_via[3 * (i + 1)] - p_via[3 * i], p_via[3 * (i + 1) + 1] - p_via[3 * i + 1], p_via[3 * (i + 1) + 2] - p_via[3 * i + 2]};
            double li = lp_norm3(d);
            if (li < 1e-3) {
                for (int c = 0; c < 3; c++) d[c] = (i > 0) ? S[LS_rp_dp + 3 * (i - 1) + c] : (c == 1 ? 1.0 : 0.0);
                li = lp_norm3(S + LS_rp_dr + 3 * i) / PI;        // a pure rotation gets |dr| / pi of path parameter
            } else {
                root = i;
            }
            for (int c = 0; c < 3; c++) S[LS_rp_dp + 3 * i + c] = d[c];
            S[LS_rp_phi + i + 1] = li;
            phi_sum += li;
            if (i == 1) root1 = root;
            if (root == 0) same0 |= 1u << i;
            if (i >= 1 && root == root1) same1 |= 1u << i;
        }
        if (n == 2) root1 = root;            // entry 1 is a padded copy of entry 0
        for (int k = 0; k < LP_S - 1; k++) {
            if (root == 0) same0 |= 1u << (n - 1 + k);
            if (root == root1) same1 |= 1u << (n - 1 + k);
        }
        if (root1 == 0) same1 |= 1u;
        // bases around the position / rotation directions, bounds and sets (ReferencePath.py:109-150, 43-46)
        for (int i = 0; i < n - 1; i++) {
            const double* dp = S + LS_rp_dp + 3 * i;
            const double nd = lp_norm3(dp), dirn[3] = {dp[0] / nd, dp[1] / nd, dp[2] / nd};
            lp_basis_pair(dirn, bp1 + 3 * i, S + LS_rp_bp1 + 3 * i, S + LS_rp_bp2 + 3 * i);
            const double drn[3] = {S[LS_rp_drn + 3 * i], S[LS_rp_drn + 3 * i + 1], S[LS_rp_drn + 3 * i + 2]};
            lp_basis_pair(drn, br1 + 3 * i, S + LS_rp_br1 + 3 * i, S + LS_rp_br2 + 3 * i);
            for (int c = 0; c < 6; c++) S[LS_rp_erb + 6 * i + c] = e_r_bound[6 * i + c];
            for (int c = 0; c < 45; c++) S[LS_rp_a + 45 * i + c] = a_sets[45 * i + c];
            for (int c = 0; c < LP_ROWS; c++) S[LS_rp_b + LP_ROWS * i + c] = b_sets[LP_ROWS * i + c];
        }
        // the nr_segs - 1 padded copies of every list; dr is padded BEFORE the division below, so its copies keep the
        // undivided last increment
        lp_pad_rows(S + LS_rp_p, 3, n); lp_pad_rows(S + LS_rp_r_tau, 3, n); lp_pad_rows(S + LS_rp_iw, 3, n);
        lp_pad_rows(S + LS_rp_dr, 3, n - 1); lp_pad_rows(S + LS_rp_drn, 3, n - 1); lp_pad_rows(S + LS_rp_dp, 3, n - 1);
        lp_pad_rows(S + LS_rp_bp1, 3, n - 1); lp_pad_rows(S + LS_rp_bp2, 3, n - 1); lp_pad_rows(S + LS_rp_br1, 3, n - 1);
        lp_pad_rows(S + LS_rp_br2, 3, n - 1); lp_pad_rows(S + LS_rp_erb, 6, n - 1); lp_pad_rows(S + LS_rp_a, 45, n - 1);
        lp_pad_rows(S + LS_rp_b, LP_ROWS, n - 1);
        // angular velocity per unit path parameter (ReferencePath.py:153-155)
        for (int i = 0; i < n - 1; i++) {
            const double ph = S[LS_rp_phi + i + 1];
            if (ph > 1e-8) for (int c = 0; c < 3; c++) S[LS_rp_dr + 3 * i + c] /= ph;
        }
    }
    for (int k = 0; k < LP_S - 1; k++) S[LS_rp_phi + n + k] = 1.0;
    S[LS_rp_phi_max] = phi_sum; S[LS_phi_max] = phi_sum;
    S[LS_rp_num_sectors] = (double)(n - 2);       // rp_sector = rp_phi_bias = 0, phi_switch[0] = phi_bias
    for (int i = 0; i < LP_S; i++) lp_set_point(S, i);
    S[LS_split] = 0.0;
    for (int i = 1; i <= LP_S; i++) S[LS_split + i] = (double)N;

    if (fresh) {      // BoundMPC.__init__: phi_current = dphi_current = 0, iw_ref = 0
        for (int c = 0; c < 3; c++) S[LS_pr_ref + c] = S[LS_p_lie + 3 + c];
        return;
    }
    // BoundMPC.update normalises dp[0] and dp[1] IN PLACE, after the window was filled: every list entry that is the same object
    // ends up unit length (twice divided when both are one object), the others keep their length
    {
        const double nd = lp_norm3(S + LS_rp_dp);
        for (int i = 0; i < n + LP_S - 2; i++)
            if ((same0 >> i) & 1u) for (int c = 0; c < 3; c++) S[LS_rp_dp + 3 * i + c] /= nd;
    }
    {
        const double nd = lp_norm3(S + LS_rp_dp + 3);
        for (int i = 0; i < n + LP_S - 2; i++)
            if ((same1 >> i) & 1u) for (int c = 0; c < 3; c++) S[LS_rp_dp + 3 * i + c] /= nd;
    }
    double phi_c = 0.0, dphi_c = 0.0;
    for (int c = 0; c < 3; c++) {
        phi_c += (S[LS_p_lie + c] - p_via[c]) * S[LS_rp_dp + c];
        dphi_c += S[LS_v + c] * S[LS_rp_dp + c];
    }
    S[LS_phi_current] = phi_c; S[LS_dphi_current] = dphi_c;
    const double om[3] = {S[LS_rp_dr], S[LS_rp_dr + 1], S[LS_rp_dr + 2]};
    lp_integrate_rot_ref(S + LS_rp_r_tau, om, 0.0, phi_c, S + LS_pr_ref);
    for (int c = 0; c < 3; c++) S[LS_iw_ref + c] = S[LS_rp_pd + LP_S * (3 + c)] + phi_c * S[LS_rp_dpd + LP_S * (3 + c)];
}

// host-side layout lookup for the packer (boundplanner_amd/device_loop.py): offset / count of a state field
inline int loop_field_lookup(const char* name, int* off, int* cnt) {
    static const char* const names[LF_COUNT] = {
#define X(n, c) #n,
        LP_FIELDS(X)
#undef X
    };
    for (int f = 0; f < LF_COUNT; f++) {
        const char *a = names[f], *b = name;
        while (*a && *a == *b) { a++; b++; }
        if (!*a && !*b) { *off = ls_off(f); *cnt = LS_CNT[f]; return 0; }
    }
    return 1;
}

}  // namespace bmpc
