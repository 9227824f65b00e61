// bmpc_ik.hpp -- batched inverse kinematics: the per-lane body of the projected Levenberg-Marquardt solve (bmpc_ik.hip launches it,
// one thread per (instance, seed); tests/emu/emu_ik.cpp compiles the same source for the CPU).
//
// Problem (RobotModel.py:79-144, setup_ik_problem / inverse_kinematics):
//   minimise_q  J(q) = |p_ee(q) - pd|^2 + |M(q) - I|_F^2,   M = R_ee(q) rd^T,   subject to lo <= q <= hi.
// Model ("Batched inverse kinematics"): with the columns c_i = z_i x (p_ee - o_i), z_i of the geometric Jacobian and
// w = vee(M - M^T) = (M21 - M12, M02 - M20, M10 - M01),
//   half gradient    gh_i = c_i . (p_ee - pd) + z_i . w                  (grad J = 2 gh)
//   Gauss-Newton     H_ij = c_i . c_j + 2 z_i . z_j                       (the model J + 2 gh^T s + s^T H s)
// The 12 x 7 residual Jacobian never exists: the rotation residual's columns vec([z_i]x M) have the Gram matrix 2 z_i . z_j.
#pragma once
#include "bmpc_device.hpp"

namespace bmpc {

struct IkOpts { double tol_cost, tol_grad, lambda0; int max_iter; };   // include/boundmpc.h bmpc_ik_opts

constexpr double IK_UNLIMITED = 1e19;     // |limit| at or beyond this: the joint is unlimited (the tables use +-1e20)
constexpr double IK_LAMBDA_MAX = 1e16;    // damping above this without a decrease: stalled (status 2)
constexpr double IK_LAMBDA_MIN = 1e-10;   // floor of the damping: H has rank <= 6, the floor keeps H + lambda D well conditioned
constexpr double IK_PI = 3.141592653589793;

BMPC_INL constexpr int ik_tri(int i, int j) { return i * (i + 1) / 2 + j; }   // packed lower triangle, j <= i
BMPC_INL bool ik_finite(double x) { return __builtin_isfinite(x); }
BMPC_INL double ik_clamp(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }

// Radical inverse of s in base b: coordinate of point s of the Halton sequence (s < 64 here, so at most 6 digits)
BMPC_INL double ik_halton(int s, int b) {
    double f = 1.0, r = 0.0;
    for (int k = 0; k < 6 && s > 0; k++) {
        f /= b;
        r += f * (s % b);
        s /= b;
    }
    return r;
}

// Seed `s` of an instance: seed 0 is q0; seed s >= 1 is lo + h_s (hi - lo) on limited joints and q0 + (2 h_s - 1) pi on unlimited
// ones, h_s = point s of the 7-D Halton sequence with bases 2, 3, 5, 7, 11, 13, 17
BMPC_INL void ik_seed(int s, const double* q0, const double* lo, const double* hi, double* q) {
    const int base[7] = {2, 3, 5, 7, 11, 13, 17};
#pragma unroll
    for (int j = 0; j < 7; j++) {
        if (s == 0) { q[j] = q0[j]; continue; }
        const double h = ik_halton(s, base[j]);
        const bool unlimited = lo[j] <= -IK_UNLIMITED || hi[j] >= IK_UNLIMITED;
        q[j] = unlimited ? q0[j] + (2.0 * h - 1.0) * IK_PI : lo[j] + h * (hi[j] - lo[j]);
    }
}

// End-effector frame of q: the chain of kin_eval (bmpc_device.hpp, same arithmetic in the same order) without the collision points.
// With FULL, also the half gradient gh[7] and the Gauss-Newton matrix H[28] (packed lower); returns J(q).  perr / rerr (non-null):
// |p - pd| and the rotation angle of M, |rotvec(M)| = atan2(|w| / 2, (tr M - 1) / 2).
template <bool FULL>
BMPC_INL double ik_eval(const RobotConst* rc, const double* q, const double* pd, const double* rd, double* H, double* gh,
                        double* perr = nullptr, double* rerr = nullptr) {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0}, Rn[9], tmp[3];
    double o[7][3], z[7][3];
#pragma unroll
    for (int i = 0; i < 7; i++) {
        mat3vec(R, rc->jxyz[i], tmp);
        for (int a = 0; a < 3; a++) t[a] += tmp[a];
        mat3mul(R, rc->jrot[i], Rn);
        for (int a = 0; a < 3; a++) { o[i][a] = t[a]; z[i][a] = Rn[3 * a + 2]; }
        double c, s;
        BMPC_SINCOS(q[i], s, c);
        const double Rz[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
        mat3mul(Rn, Rz, R);
    }
    double p[3], Ree[9], M[9];
    mat3vec(R, rc->ee_xyz, tmp);
    for (int a = 0; a < 3; a++) p[a] = t[a] + tmp[a];
    mat3mul(R, rc->ee_rot, Ree);
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) M[3 * a + b] = Ree[3 * a] * rd[3 * b] + Ree[3 * a + 1] * rd[3 * b + 1] + Ree[3 * a + 2] * rd[3 * b + 2];
    double e[3], f = 0.0;
    for (int a = 0; a < 3; a++) { e[a] = p[a] - pd[a]; f += e[a] * e[a]; }
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) { const double d = M[3 * a + b] - (a == b ? 1.0 : 0.0); f += d * d; }
    const double w[3] = {M[7] - M[5], M[2] - M[6], M[3] - M[1]};
    if (perr) *perr = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    if (rerr) *rerr = atan2(0.5 * sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), 0.5 * (M[0] + M[4] + M[8] - 1.0));
    if (FULL) {
        double cc[7][3];
#pragma unroll
        for (int i = 0; i < 7; i++) {
            double r[3];
            for (int a = 0; a < 3; a++) r[a] = p[a] - o[i][a];
            cross3(z[i], r, cc[i]);
            gh[i] = dot3(cc[i], e) + dot3(z[i], w);
        }
#pragma unroll
        for (int i = 0; i < 7; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) H[ik_tri(i, j)] = dot3(cc[i], cc[j]) + 2.0 * dot3(z[i], z[j]);
    }
    return f;
}

// Damped step of the free joints: (H + lam D) s = -gh on the free set, D = diag(H) (Marquardt's scaling; H_ii >= 2 |z_i|^2 = 2, so
// H + lam D is positive definite for lam > 0 although H has rank <= 6), s = 0 on the fixed joints (mask bit i set: joint i is at a
// bound with the gradient pointing outward).  Cholesky in registers; false when a pivot is not positive (or not finite).
BMPC_INL bool ik_step(const double* H, const double* gh, double lam, int fixed, double* s) {
    double L[28], y[7];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 7; i++) {
        const bool fi = (fixed >> i) & 1;
#pragma unroll
        for (int j = 0; j <= i; j++) {
            const bool fj = (fixed >> j) & 1;
            double a = (fi || fj) ? (i == j ? 1.0 : 0.0) : H[ik_tri(i, j)] * (i == j ? 1.0 + lam : 1.0);
#pragma unroll
            for (int k = 0; k < j; k++) a -= L[ik_tri(i, k)] * L[ik_tri(j, k)];
            if (i == j) {
                ok = ok && a > 0.0 && ik_finite(a);
                L[ik_tri(i, i)] = sqrt(ok ? a : 1.0);
            } else {
                L[ik_tri(i, j)] = a / L[ik_tri(j, j)];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 7; i++) {
        double a = ((fixed >> i) & 1) ? 0.0 : -gh[i];
#pragma unroll
        for (int k = 0; k < i; k++) a -= L[ik_tri(i, k)] * y[k];
        y[i] = a / L[ik_tri(i, i)];
    }
#pragma unroll
    for (int i = 6; i >= 0; i--) {
        double a = y[i];
#pragma unroll
        for (int k = i + 1; k < 7; k++) a -= L[ik_tri(k, i)] * s[k];
        s[i] = ((fixed >> i) & 1) ? 0.0 : a / L[ik_tri(i, i)];
    }
    return ok;
}

// One lane: the projected Levenberg-Marquardt solve from the seed in q (overwritten with the result, inside [lo, hi] exactly unless
// status 3 on entry).  Status: 0 converged (J <= tol_cost, or |P(q - grad J) - q|_inf <= tol_grad), 1 max_iter, 2 stalled (damping
// above IK_LAMBDA_MAX without a decrease), 3 numerical (non-finite input, cost or step).  Every trial -- accepted or rejected --
// counts against max_iter; a pass of the loop either evaluates a trial (and counts it) or re-evaluates the model at q after a
// rejection, so the loop ends after at most 2 max_iter + 1 evaluations whatever the data.  The model is evaluated at ONE place in
// the loop (the trial point's model replaces the current one and is recomputed at q when the trial is rejected): one inlined copy
// of the kinematic chain, and H, gh live once.
BMPC_INL void ik_solve_lane(const RobotConst* rc, const IkOpts& o, const double* pd, const double* rd, const double* lo,
                            const double* hi, double* q, double& cost, int& iters, int& status) {
    bool good = ik_finite(o.lambda0) && o.lambda0 > 0.0;
    for (int a = 0; a < 3; a++) good = good && ik_finite(pd[a]);
    for (int a = 0; a < 9; a++) good = good && ik_finite(rd[a]);
    for (int j = 0; j < 7; j++) good = good && ik_finite(q[j]) && !(lo[j] > hi[j]) && lo[j] == lo[j] && hi[j] == hi[j];
    iters = 0;
    if (!good) { cost = __builtin_nan(""); status = 3; return; }
    double qt[7];                          // the point the next pass evaluates
    for (int j = 0; j < 7; j++) { q[j] = ik_clamp(q[j], lo[j], hi[j]); qt[j] = q[j]; }
    double H[28], gh[7];
    double f = __builtin_inf(), pred = 0.0, lam = o.lambda0, nu = 2.0;
    bool trial = false;
    int it = 0, st = -1;
    while (st < 0) {
        const double fx = ik_eval<true>(rc, qt, pd, rd, H, gh);
        if (!ik_finite(fx)) { st = 3; break; }
        if (trial) {
            trial = false;
            if (pred > 0.0 && fx < f) {                     // accepted: gain ratio -> damping (Nielsen)
                const double rho = (f - fx) / pred, t = 2.0 * rho - 1.0;
                for (int j = 0; j < 7; j++) q[j] = qt[j];
                lam = fmax(lam * fmax(1.0 / 3.0, 1.0 - t * t * t), IK_LAMBDA_MIN);
                nu = 2.0;
            } else {                                        // rejected: more damping, the model at q again
                lam *= nu;
                nu *= 2.0;
                if (lam > IK_LAMBDA_MAX) { st = 2; break; }
                for (int j = 0; j < 7; j++) qt[j] = q[j];
                continue;
            }
        }
        f = fx;
        if (f <= o.tol_cost) { st = 0; break; }
        double pg = 0.0;
        int fixed = 0;
#pragma unroll
        for (int j = 0; j < 7; j++) {
            pg = fmax(pg, fabs(ik_clamp(q[j] - 2.0 * gh[j], lo[j], hi[j]) - q[j]));
            if ((q[j] <= lo[j] && gh[j] > 0.0) || (q[j] >= hi[j] && gh[j] < 0.0)) fixed |= 1 << j;
        }
        if (pg <= o.tol_grad) { st = 0; break; }
        if (it >= o.max_iter) { st = 1; break; }
        it++;
        double s[7];
        if (!ik_step(H, gh, lam, fixed, s)) {               // (H + lam D is positive definite for lam > 0: rounding only)
            lam *= nu;
            nu *= 2.0;
            if (lam > IK_LAMBDA_MAX) { st = 2; break; }
            continue;                                       // qt == q: the pass re-evaluates the model at q
        }
        // clamped trial and the decrease the model predicts for it: -(2 gh . ds + ds^T H ds), ds = qt - q
        double lin = 0.0, quad = 0.0;
#pragma unroll
        for (int j = 0; j < 7; j++) { qt[j] = ik_clamp(q[j] + s[j], lo[j], hi[j]); s[j] = qt[j] - q[j]; }
#pragma unroll
        for (int i = 0; i < 7; i++) {
            lin += gh[i] * s[i];
            double hs = 0.0;
#pragma unroll
            for (int j = 0; j < 7; j++) hs += H[j <= i ? ik_tri(i, j) : ik_tri(j, i)] * s[j];
            quad += s[i] * hs;
        }
        pred = -(2.0 * lin + quad);
        if (!ik_finite(pred)) { st = 3; break; }
        trial = true;
    }
    cost = f;
    iters = it;
    status = st;
}

// Order of the seeds of an instance: (status != 0, J, seed index), lexicographic, a NaN cost last.  A total order: every reduction
// tree picks the same winner.
BMPC_INL bool ik_better(int st_a, double f_a, int s_a, int st_b, double f_b, int s_b) {
    const int ba = st_a != 0, bb = st_b != 0;
    if (ba != bb) return ba < bb;
    const double ka = f_a == f_a ? f_a : __builtin_inf(), kb = f_b == f_b ? f_b : __builtin_inf();
    if (ka != kb) return ka < kb;
    return s_a < s_b;
}

// outputs of instance b from its best seed s (ik_better); every output but q_out may be null; the errors are evaluated at q again
BMPC_INL void ik_store(const RobotConst* rc, long b, int s, const double* q, double cost, int iters, int status, const double* pd,
                       const double* rd, double* q_out, double* cost_out, double* perr_out, double* rerr_out, int* iters_out,
                       int* status_out, int* seed_out) {
    for (int j = 0; j < 7; j++) q_out[b * 7 + j] = q[j];
    if (cost_out) cost_out[b] = cost;
    if (iters_out) iters_out[b] = iters;
    if (status_out) status_out[b] = status;
    if (seed_out) seed_out[b] = s;
    if (perr_out || rerr_out) {
        double pe, re;
        ik_eval<false>(rc, q, pd, rd, nullptr, nullptr, &pe, &re);
        if (perr_out) perr_out[b] = pe;
        if (rerr_out) rerr_out[b] = re;
    }
}

}  // namespace bmpc
