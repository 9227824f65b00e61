// bmpc_sets.hpp -- batched convex free-space sets: the per-lane body of the IRIS-style set growth of the plan phase (bmpc_sets.hip
// launches it, one thread per seed; tests/emu/emu_sets.cpp compiles the same source for the CPU).
//
// Restates the host finder (boundplanner_amd/convex_set_finder.py, planner_opt.py):
//   find_set_around_point        alternate polyhedron growth and a maximum-volume inscribed ellipsoid (MVIE), at most SETS_MAX_ROUNDS
//   compute_polyhedron / _projs  nearest obstacle first, distances in the metric of the current ellipsoid, obstacles behind a chosen
//                                halfspace dropped
//   find_set_collision_avoidance the segment variant (closest pairs and the greedy halfspaces: bmpc_freespace.hpp, shared with the
//                                device loop), with its free-centre MVIE
//   planner_opt.mvie             log-barrier Newton method in the parameterisation of the reference's SOCP
//
// Storage: the obstacle rows and vertices are read from global memory (the same for every lane: cached); the
// rows of the set being grown live in the lane's output rows A [SETS_ROWS][3], b [SETS_ROWS]; the per-obstacle distances of a round
// live in `dist` with stride `ds` (LDS in the kernel).  No array here is indexed by a runtime value, so nothing goes to scratch.
#pragma once
#include "bmpc_freespace.hpp"

namespace bmpc {

constexpr int SETS_ROWS = 20;        // rows per set: the 6 workspace rows plus 14 halfspaces (ConvexSetFinder.py:126-128)
constexpr int SETS_MAXOBS = 32;      // obstacles per scene
constexpr int SETS_OROWS = LP_ROWS;  // rows per obstacle (LoopScene layout: [15][3], [15], AAt [15][15])
constexpr int SETS_NV = LP_NV;       // vertices per obstacle
constexpr int SETS_MAX_ROUNDS = 5;   // ConvexSetFinder.max_iter

// status values (include/boundmpc.h bmpc_convex_sets)
constexpr int SETS_OK = 0, SETS_VIOLATES = 1, SETS_TOO_MANY_ROWS = 2, SETS_NO_INTERIOR = 3, SETS_NUMERICAL = 4;

struct SetScene {
    LoopScene obs;        // the obstacles; AAt is set in segment mode only (its closest pairs), box / is_box never: no box shortcut here
    double e_min[3], e_max[3];
    // in the argument order of bmpc_convex_sets
    SetScene(int n_obs, const double* A, const double* b, const int* nrows, const double* V, const int* nv, const double* AAt,
             const double (&lo)[3], const double (&hi)[3])
        : obs{n_obs, A, b, AAt, nrows, V, nv, nullptr, nullptr}, e_min{lo[0], lo[1], lo[2]}, e_max{hi[0], hi[1], hi[2]} {}
};

BMPC_INL constexpr int sp_tri(int i, int j) { return i * (i + 1) / 2 + j; }   // packed lower triangle, j <= i
BMPC_INL bool sp_finite(double x) { return __builtin_isfinite(x); }

// ------------------------------------------------------------------------------------------------------------------------------
// small dense algebra
// ------------------------------------------------------------------------------------------------------------------------------
BMPC_INL double sp_det3(const double* M) {
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

BMPC_INL double sp_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
BMPC_INL void sp_cross(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

// inverse of a 3x3 matrix through the adjugate; returns the determinant
BMPC_INL double sp_inv3(const double* M, double* Mi) {
    const double d = sp_det3(M);
    Mi[0] = (M[4] * M[8] - M[5] * M[7]) / d; Mi[1] = (M[2] * M[7] - M[1] * M[8]) / d; Mi[2] = (M[1] * M[5] - M[2] * M[4]) / d;
    Mi[3] = (M[5] * M[6] - M[3] * M[8]) / d; Mi[4] = (M[0] * M[8] - M[2] * M[6]) / d; Mi[5] = (M[2] * M[3] - M[0] * M[5]) / d;
    Mi[6] = (M[3] * M[7] - M[4] * M[6]) / d; Mi[7] = (M[1] * M[6] - M[0] * M[7]) / d; Mi[8] = (M[0] * M[4] - M[1] * M[3]) / d;
    return d;
}

// smallest eigenvalue of a symmetric 3x3 matrix (closed form, trigonometric)
BMPC_INL double sp_min_eig_sym3(const double* M) {
    const double p1 = M[1] * M[1] + M[2] * M[2] + M[5] * M[5];
    const double q = (M[0] + M[4] + M[8]) / 3.0;
    if (p1 == 0.0) return fmin(M[0], fmin(M[4], M[8]));
    const double p2 = (M[0] - q) * (M[0] - q) + (M[4] - q) * (M[4] - q) + (M[8] - q) * (M[8] - q) + 2.0 * p1;
    const double p = sqrt(p2 / 6.0);
    double Bm[9];
    for (int i = 0; i < 9; i++) Bm[i] = (M[i] - (i % 4 == 0 ? q : 0.0)) / p;
    const double r = fmin(fmax(sp_det3(Bm) / 2.0, -1.0), 1.0);
    const double phi = acos(r) / 3.0;
    return q + 2.0 * p * cos(phi + 2.0 * 3.141592653589793 / 3.0);
}

// Solve H x = -g for a symmetric positive definite H (packed lower, N x N) by Cholesky; false when a pivot is not positive
template <int N>
BMPC_INL bool sp_newton_dir(const double* H, const double* g, double* dx) {
    double L[N * (N + 1) / 2], y[N];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < N; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) {
            double a = H[sp_tri(i, j)];
#pragma unroll
            for (int k = 0; k < j; k++) a -= L[sp_tri(i, k)] * L[sp_tri(j, k)];
            if (i == j) {
                ok = ok && a > 0.0 && sp_finite(a);
                L[sp_tri(i, i)] = sqrt(ok ? a : 1.0);
            } else {
                L[sp_tri(i, j)] = a / L[sp_tri(j, j)];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
        double a = -g[i];
#pragma unroll
        for (int k = 0; k < i; k++) a -= L[sp_tri(i, k)] * y[k];
        y[i] = a / L[sp_tri(i, i)];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double a = y[i];
#pragma unroll
        for (int k = i + 1; k < N; k++) a -= L[sp_tri(k, i)] * dx[k];
        dx[i] = a / L[sp_tri(i, i)];
    }
    return ok;
}

// ------------------------------------------------------------------------------------------------------------------------------
// ellipsoid-metric projection (compute_set_projs + planner_opt.project_polytope)
// ------------------------------------------------------------------------------------------------------------------------------
// Row r of obstacle o in the coordinates u of x = p0 + E u (E symmetric), scaled to unit length: a' = E a / |E a|,
// b' = (b - a.p0) / |E a|.  False for a zero row (project_polytope drops it).
BMPC_INL bool sp_urow(const SetScene& sc, int o, int r, const double* E, const double* p0, double* ap, double& bp) {
    const double* a = sc.obs.A + 3 * (SETS_OROWS * o + r);
    const double a0 = a[0], a1 = a[1], a2 = a[2];
    // a^T E (E symmetric: the row of A @ E)
    ap[0] = a0 * E[0] + a1 * E[3] + a2 * E[6];
    ap[1] = a0 * E[1] + a1 * E[4] + a2 * E[7];
    ap[2] = a0 * E[2] + a1 * E[5] + a2 * E[8];
    bp = sc.obs.b[SETS_OROWS * o + r] - (a0 * p0[0] + a1 * p0[1] + a2 * p0[2]);
    const double n = sqrt(ap[0] * ap[0] + ap[1] * ap[1] + ap[2] * ap[2]);
    if (!(n > 0.0)) return false;
    ap[0] /= n; ap[1] /= n; ap[2] /= n; bp /= n;
    return true;
}

// is u feasible for every (non-zero) row of obstacle o: a'.u - b' <= tol
BMPC_INL bool sp_ufeas(const SetScene& sc, int o, const double* E, const double* p0, const double* u, double tol) {
    const int nr = sc.obs.nrows[o];
    for (int r = 0; r < nr; r++) {
        double ap[3], bp;
        if (!sp_urow(sc, o, r, E, p0, ap, bp)) continue;
        if (ap[0] * u[0] + ap[1] * u[1] + ap[2] * u[2] - bp > tol) return false;
    }
    return true;
}

// Exact projection of u = 0 onto {u: a'_r . u <= b'_r} (obstacle o seen from p0 through E): the KKT points of the active sets of
// size 1, then 2, then 3 (unit rows), each solved on the rows themselves by Cramer's rule with one step of refinement (the Gram matrix has
// the square of their condition); the nearest feasible one of the smallest size that has one.  The tolerances of feasibility and
// of the multipliers' signs are project_polytope's 1e-10, relative to max(1, |u|): in the first round the rows are scaled by 1e-4 and
// |u| reaches 1e4, where an absolute 1e-10 is below the rounding of a'.u.
// Returns the point p0 + E u in world coordinates; false when no KKT point exists (an empty obstacle).
BMPC_INL bool sp_project(const SetScene& sc, int o, const double* E, const double* p0, double* pt) {
    const int nr = sc.obs.nrows[o];
    double u[3] = {0.0, 0.0, 0.0};
    bool inside = true;
    for (int r = 0; r < nr && inside; r++) {
        double ap[3], bp;
        if (sp_urow(sc, o, r, E, p0, ap, bp) && -bp > 0.0) inside = false;
    }
    bool found = inside;
    // k = 1: u = b'_i a'_i with multiplier -b'_i / |a'_i|^2
    if (!found) {
        double bd = __builtin_inf();
        for (int i = 0; i < nr; i++) {
            double a[3], bi;
            if (!sp_urow(sc, o, i, E, p0, a, bi)) continue;
            const double g = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
            if (!(fabs(g) > 1e-14)) continue;
            const double lam = -bi / g;
            const double tol = 1e-10 * fmax(1.0, fabs(lam) * sqrt(g));
            if (lam < -tol) continue;
            const double x[3] = {-lam * a[0], -lam * a[1], -lam * a[2]};
            if (!sp_ufeas(sc, o, E, p0, x, tol)) continue;
            const double d = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
            if (d < bd) { bd = d; u[0] = x[0]; u[1] = x[1]; u[2] = x[2]; found = true; }
        }
    }
    // k = 2
    if (!found) {
        double bd = __builtin_inf();
        for (int i = 0; i < nr; i++) {
            double a[3], bi;
            if (!sp_urow(sc, o, i, E, p0, a, bi)) continue;
            for (int j = i + 1; j < nr; j++) {
                double c[3], bj;
                if (!sp_urow(sc, o, j, E, p0, c, bj)) continue;
                // the point of the edge a.x = bi, c.x = bj nearest to 0: x = (bi c x e + bj e x a) / |e|^2 along the edge's
                // direction e = a x c, and x = -l1 a - l2 c
                double e[3], ce[3], ea[3];
                sp_cross(a, c, e);
                const double ee = sp_dot(e, e);                                  // the Gram determinant of the unit rows
                if (!(ee > 1e-14)) continue;
                sp_cross(c, e, ce);
                sp_cross(e, a, ea);
                double x[3];
                for (int q = 0; q < 3; q++) x[q] = (bi * ce[q] + bj * ea[q]) / ee;
                // (a candidate whose multipliers are negative beyond any rounding is left before the refinement: most are)
                if (fmin(-sp_dot(x, ce), -sp_dot(x, ea)) / ee < -1e-6 * fmax(1.0, sqrt(sp_dot(x, x)))) continue;
                {                                                                // one step of refinement
                    const double ri = bi - sp_dot(a, x), rj = bj - sp_dot(c, x);
                    for (int q = 0; q < 3; q++) x[q] += (ri * ce[q] + rj * ea[q]) / ee;
                }
                const double l1 = -sp_dot(x, ce) / ee, l2 = -sp_dot(x, ea) / ee;
                const double tol = 1e-10 * fmax(1.0, sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]));
                if (l1 < -tol || l2 < -tol) continue;
                if (!sp_ufeas(sc, o, E, p0, x, tol)) continue;
                const double d = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
                if (d < bd) { bd = d; u[0] = x[0]; u[1] = x[1]; u[2] = x[2]; found = true; }
            }
        }
    }
    // k = 3
    if (!found) {
        double bd = __builtin_inf();
        for (int i = 0; i < nr; i++) {
            double a[3], bi;
            if (!sp_urow(sc, o, i, E, p0, a, bi)) continue;
            for (int j = i + 1; j < nr; j++) {
                double c[3], bj;
                if (!sp_urow(sc, o, j, E, p0, c, bj)) continue;
                for (int k = j + 1; k < nr; k++) {
                    double e[3], bk;
                    if (!sp_urow(sc, o, k, E, p0, e, bk)) continue;
                    // the vertex a.x = bi, c.x = bj, e.x = bk by Cramer's rule on the rows themselves (the Gram matrix has the
                    // square of their condition): x = (bi c x e + bj e x a + bk a x c) / det, and x = -l0 a - l1 c - l2 e
                    double ce[3], ea[3], ac[3];
                    sp_cross(c, e, ce);
                    sp_cross(e, a, ea);
                    sp_cross(a, c, ac);
                    const double det = sp_dot(a, ce);
                    if (!(det * det > 1e-14)) continue;                          // det^2: the Gram determinant of the unit rows
                    double x[3];
                    for (int q = 0; q < 3; q++) x[q] = (bi * ce[q] + bj * ea[q] + bk * ac[q]) / det;
                    if (fmin(-sp_dot(x, ce) / det, fmin(-sp_dot(x, ea) / det, -sp_dot(x, ac) / det)) < -1e-6 * fmax(1.0, sqrt(sp_dot(x, x))))
                        continue;                                                // (as above: left before the refinement)
                    {                                                            // one step of refinement
                        const double ri = bi - sp_dot(a, x), rj = bj - sp_dot(c, x), rk = bk - sp_dot(e, x);
                        for (int q = 0; q < 3; q++) x[q] += (ri * ce[q] + rj * ea[q] + rk * ac[q]) / det;
                    }
                    const double l[3] = {-sp_dot(x, ce) / det, -sp_dot(x, ea) / det, -sp_dot(x, ac) / det};
                    const double tol = 1e-10 * fmax(1.0, sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]));
                    if (l[0] < -tol || l[1] < -tol || l[2] < -tol) continue;
                    if (!sp_ufeas(sc, o, E, p0, x, tol)) continue;
                    const double d = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
                    if (d < bd) { bd = d; u[0] = x[0]; u[1] = x[1]; u[2] = x[2]; found = true; }
                }
            }
        }
    }
    for (int q = 0; q < 3; q++) pt[q] = E[3 * q] * u[0] + E[3 * q + 1] * u[1] + E[3 * q + 2] * u[2] + p0[q];
    return found;
}

// ------------------------------------------------------------------------------------------------------------------------------
// the set under construction: rows in A [SETS_ROWS][3], b [SETS_ROWS] (the lane's output rows)
// ------------------------------------------------------------------------------------------------------------------------------
BMPC_INL void sp_init_rows(const SetScene& sc, double* A, double* b) {      // init_halfspaces: +x, -x, +y, -y, +z, -z
    for (int i = 0; i < 3; i++) {
        for (int c = 0; c < 3; c++) { A[3 * (2 * i) + c] = c == i ? 1.0 : 0.0; A[3 * (2 * i + 1) + c] = c == i ? -1.0 : 0.0; }
        b[2 * i] = sc.e_max[i];
        b[2 * i + 1] = -sc.e_min[i];
    }
}

// compute_polyhedron: the rows of one round around p (E = q_inv, Qe = q_ellipse); returns the row count or a negative status
BMPC_INL int sp_polyhedron(const SetScene& sc, const double* E, const double* Qe, const double* p, double* dist, int ds, double* A, double* b) {
    sp_init_rows(sc, A, b);
    unsigned remain = 0;
    for (int i = 0; i < sc.obs.n_obs; i++) {
        double pt[3];
        if (!sp_project(sc, i, E, p, pt)) return -SETS_NUMERICAL;
        const double d[3] = {pt[0] - p[0], pt[1] - p[1], pt[2] - p[2]};
        double s = 0.0;
        for (int r = 0; r < 3; r++) {
            const double v = Qe[3 * r] * d[0] + Qe[3 * r + 1] * d[1] + Qe[3 * r + 2] * d[2];
            s += v * v;
        }
        dist[i * ds] = sqrt(s);
        remain |= 1u << i;
    }
    // Q2 = Qe Qe^T
    double Q2[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Q2[3 * r + c] = Qe[3 * r] * Qe[3 * c] + Qe[3 * r + 1] * Qe[3 * c + 1] + Qe[3 * r + 2] * Qe[3 * c + 2];
    int n = 6;
    while (remain) {
        const int idx = sp_nearest(sc.obs.n_obs, remain, dist, ds);
        if (dist[idx * ds] < 0.99) return -SETS_VIOLATES;        // the host raises "Ellipse violates constraints"
        double cp[3];
        sp_project(sc, idx, E, p, cp);                            // the same projection again (deterministic)
        const double d[3] = {cp[0] - p[0], cp[1] - p[1], cp[2] - p[2]};
        double a[3];
        for (int r = 0; r < 3; r++) a[r] = 2.0 * (Q2[3 * r] * d[0] + Q2[3 * r + 1] * d[1] + Q2[3 * r + 2] * d[2]);
        double bh = a[0] * cp[0] + a[1] * cp[1] + a[2] * cp[2];
        const double na = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        for (int r = 0; r < 3; r++) a[r] /= na;
        bh /= na;
        remain = sp_drop_behind(sc.obs, remain & ~(1u << idx), a, bh);
        if (n >= SETS_ROWS) return -SETS_TOO_MANY_ROWS;
        for (int c = 0; c < 3; c++) A[3 * n + c] = a[c];
        b[n] = bh;
        n++;
    }
    return n;
}

// ------------------------------------------------------------------------------------------------------------------------------
// MVIE (planner_opt.mvie): x = (L00, L10, L11, L20, L21, L22[, c]); row i: s = d_i - a_i.c (d_i = b_i - a_i.c0 with a fixed centre),
// v = L^T a_i, psi = s^2 - |v|^2;  minimise -t (L00 / 4 + L11 / 2 + L22 / 4 in logs) - sum log psi, t = 1, 8, 64, ... until
// 2 m / t < 1e-10 -- the same central path, Newton tolerances and backtracking as the host, so both end at the same point.
// ------------------------------------------------------------------------------------------------------------------------------
template <int NXV>
BMPC_INL void sp_mvie_row(const double* a, double d, const double* x, double& s, double* v) {
    s = d;
    if constexpr (NXV == 9) s -= a[0] * x[6] + a[1] * x[7] + a[2] * x[8];
    v[0] = a[0] * x[0] + a[1] * x[1] + a[2] * x[3];
    v[1] = a[1] * x[2] + a[2] * x[4];
    v[2] = a[2] * x[5];
}

// barrier value; +inf outside the domain
template <int NXV>
BMPC_INL double sp_mvie_value(const double* A, const double* b, int m, const double* c0, const double* x, double t) {
    if (!(x[0] > 0.0) || !(x[2] > 0.0) || !(x[5] > 0.0)) return __builtin_inf();
    double f = -t * (0.25 * log(x[0]) + 0.5 * log(x[2]) + 0.25 * log(x[5]));
    for (int i = 0; i < m; i++) {
        const double a[3] = {A[3 * i], A[3 * i + 1], A[3 * i + 2]};
        const double d = NXV == 9 ? b[i] : b[i] - (a[0] * c0[0] + a[1] * c0[1] + a[2] * c0[2]);
        double s, v[3];
        sp_mvie_row<NXV>(a, d, x, s, v);
        const double psi = s * s - (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (!(s > 0.0) || !(psi > 0.0)) return __builtin_inf();
        f -= log(psi);
    }
    return f;
}

// x: start (strictly feasible) in, optimum out.  Returns false on a numerical failure; newton += Newton steps taken.
template <int NXV>
BMPC_INL bool sp_mvie_newton(const double* A, const double* b, int m, const double* c0, double* x, int& newton) {
    double t = 1.0;
    for (int outer = 0; outer < 60; outer++) {
        for (int it = 0; it < 60; it++) {
            double g[NXV], H[NXV * (NXV + 1) / 2];
#pragma unroll
            for (int k = 0; k < NXV; k++) g[k] = 0.0;
#pragma unroll
            for (int k = 0; k < NXV * (NXV + 1) / 2; k++) H[k] = 0.0;
            for (int i = 0; i < m; i++) {
                const double a[3] = {A[3 * i], A[3 * i + 1], A[3 * i + 2]};
                const double d = NXV == 9 ? b[i] : b[i] - (a[0] * c0[0] + a[1] * c0[1] + a[2] * c0[2]);
                double s, v[3];
                sp_mvie_row<NXV>(a, d, x, s, v);
                const double psi = s * s - (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                // M (3 x NXV): v = M x;  cv: ds/dx
                double M[3][NXV], cv[NXV];
#pragma unroll
                for (int k = 0; k < NXV; k++) { M[0][k] = M[1][k] = M[2][k] = 0.0; cv[k] = 0.0; }
                M[0][0] = a[0]; M[0][1] = a[1]; M[0][3] = a[2];
                M[1][2] = a[1]; M[1][4] = a[2];
                M[2][5] = a[2];
                if constexpr (NXV == 9) { cv[6] = -a[0]; cv[7] = -a[1]; cv[8] = -a[2]; }
                // gpsi = 2 s cv - 2 M^T v;  g -= gpsi / psi;  H += gg^T / psi^2 - (2 cv cv^T - 2 M^T M) / psi
                double gp[NXV];
#pragma unroll
                for (int k = 0; k < NXV; k++) gp[k] = (2.0 * s * cv[k] - 2.0 * (M[0][k] * v[0] + M[1][k] * v[1] + M[2][k] * v[2])) / psi;
#pragma unroll
                for (int k = 0; k < NXV; k++) g[k] -= gp[k];
#pragma unroll
                for (int k = 0; k < NXV; k++)
#pragma unroll
                    for (int l = 0; l <= k; l++)
                        H[sp_tri(k, l)] += gp[k] * gp[l] -
                                           (2.0 * cv[k] * cv[l] - 2.0 * (M[0][k] * M[0][l] + M[1][k] * M[1][l] + M[2][k] * M[2][l])) / psi;
            }
            g[0] -= t * 0.25 / x[0]; g[2] -= t * 0.5 / x[2]; g[5] -= t * 0.25 / x[5];
            H[sp_tri(0, 0)] += t * 0.25 / (x[0] * x[0]);
            H[sp_tri(2, 2)] += t * 0.5 / (x[2] * x[2]);
            H[sp_tri(5, 5)] += t * 0.25 / (x[5] * x[5]);
            double dx[NXV];
            if (!sp_newton_dir<NXV>(H, g, dx)) {
                // H is positive definite, but in a set 1 mm thick its condition reaches 1e16 and a pivot may round to <= 0: once
                // more with the diagonal raised by 1e-12 of its largest entry (a descent direction still; the line search decides)
                double hmax = 0.0;
#pragma unroll
                for (int k = 0; k < NXV; k++) hmax = fmax(hmax, H[sp_tri(k, k)]);
#pragma unroll
                for (int k = 0; k < NXV; k++) H[sp_tri(k, k)] += 1e-12 * hmax;
                if (!sp_newton_dir<NXV>(H, g, dx)) return false;
            }
            double dec = 0.0;
#pragma unroll
            for (int k = 0; k < NXV; k++) dec -= g[k] * dx[k];
            if (!sp_finite(dec)) return false;
            newton++;
            if (dec < 1e-22 * fmax(1.0, t)) break;
            double al = 1.0;
            const double f0 = sp_mvie_value<NXV>(A, b, m, c0, x, t);
            for (;;) {
                double xt[NXV];
#pragma unroll
                for (int k = 0; k < NXV; k++) xt[k] = x[k] + al * dx[k];
                if (!(sp_mvie_value<NXV>(A, b, m, c0, xt, t) > f0 - 1e-4 * al * dec && al > 1e-14)) break;
                al *= 0.5;
            }
#pragma unroll
            for (int k = 0; k < NXV; k++) x[k] = x[k] + al * dx[k];
            if (dec < 1e-18 * fmax(1.0, t)) break;
        }
        if (2.0 * m / t < 1e-10) break;
        t *= 8.0;
    }
    return true;
}

// A strictly interior point of {A x <= b} (unit rows) for the free-centre start: the Chebyshev problem max r s.t. a_i.x + r <= b_i
// by a log-barrier Newton method on (x, r) from xs with r = min slack - 1, t = 1, 8, ... until m / t < 1e-3 and r >= m / t: an approximate
// Chebyshev centre (the host starts at the exact one from an LP; any strictly interior start leads to the same optimum).  c: the point; returns its radius min_i (b_i - a_i.c) / |a_i| (<= 0: none).
BMPC_INL double sp_interior(const double* A, const double* b, int m, const double* xs, double* c, int& newton) {
    double z[4] = {xs[0], xs[1], xs[2], 0.0};
    double smin = __builtin_inf();
    for (int i = 0; i < m; i++) smin = fmin(smin, b[i] - (A[3 * i] * z[0] + A[3 * i + 1] * z[1] + A[3 * i + 2] * z[2]));
    z[3] = smin - 1.0;
    auto value = [&](const double* zz, double t) {
        double f = -t * zz[3];
        for (int i = 0; i < m; i++) {
            const double s = b[i] - (A[3 * i] * zz[0] + A[3 * i + 1] * zz[1] + A[3 * i + 2] * zz[2]) - zz[3];
            if (!(s > 0.0)) return (double)__builtin_inf();
            f -= log(s);
        }
        return f;
    };
    // on the central path r(t) >= r* - m / t: the path is followed until m / t < 1e-3 AND r >= m / t, i.e. r >= r* / 2 (a set whose
    // inradius r* is below 1e-3 would otherwise be left with r < 0 and be reported as having no interior)
    // -- and left as soon as r + m / t <= 0, which proves r* <= 0: an empty set costs no more stages than it takes to see that
    for (double t = 1.0; m / t >= 1e-3 || (!(z[3] >= m / t) && z[3] + m / t > 0.0 && t < 1e15); t *= 8.0) {
        for (int it = 0; it < 50; it++) {
            double g[4] = {0.0, 0.0, 0.0, -t}, H[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int i = 0; i < m; i++) {
                const double w[4] = {A[3 * i], A[3 * i + 1], A[3 * i + 2], 1.0};
                const double s = b[i] - (w[0] * z[0] + w[1] * z[1] + w[2] * z[2]) - z[3];
#pragma unroll
                for (int k = 0; k < 4; k++) g[k] += w[k] / s;
#pragma unroll
                for (int k = 0; k < 4; k++)
#pragma unroll
                    for (int l = 0; l <= k; l++) H[sp_tri(k, l)] += w[k] * w[l] / (s * s);
            }
            double dz[4];
            if (!sp_newton_dir<4>(H, g, dz)) break;
            const double dec = -(g[0] * dz[0] + g[1] * dz[1] + g[2] * dz[2] + g[3] * dz[3]);
            newton++;
            if (!(dec > 1e-12)) break;
            const double f0 = value(z, t);
            double al = 1.0;
            for (;;) {
                const double zt[4] = {z[0] + al * dz[0], z[1] + al * dz[1], z[2] + al * dz[2], z[3] + al * dz[3]};
                if (!(value(zt, t) > f0 - 1e-4 * al * dec) || al <= 1e-14) break;
                al *= 0.5;
            }
            if (al <= 1e-14) break;
#pragma unroll
            for (int k = 0; k < 4; k++) z[k] += al * dz[k];
        }
    }
    c[0] = z[0]; c[1] = z[1]; c[2] = z[2];
    double r = __builtin_inf();
    for (int i = 0; i < m; i++) {
        const double* a = A + 3 * i;
        r = fmin(r, (b[i] - (a[0] * c[0] + a[1] * c[1] + a[2] * c[2])) / sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]));
    }
    if (!(r > 0.0)) {               // the search failed: a start that was strictly interior itself is not lost
        double rs = __builtin_inf();
        for (int i = 0; i < m; i++) {
            const double* a = A + 3 * i;
            rs = fmin(rs, (b[i] - (a[0] * xs[0] + a[1] * xs[1] + a[2] * xs[2])) / sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]));
        }
        if (rs > 0.0) { c[0] = xs[0]; c[1] = xs[1]; c[2] = xs[2]; r = rs; }
    }
    return r;
}

// MVIE of the set's rows.  fixed: centre c (in / out); free: start from an approximate Chebyshev centre found from c.  Out:
// q = L L^T, c.  Returns a status.
BMPC_INL int sp_mvie(const double* A, const double* b, int m, bool fixed, double* c, double* q, int& newton) {
    double r0;
    double c0[3] = {c[0], c[1], c[2]};
    if (fixed) {
        r0 = __builtin_inf();
        for (int i = 0; i < m; i++) {
            const double* a = A + 3 * i;
            r0 = fmin(r0, (b[i] - (a[0] * c0[0] + a[1] * c0[1] + a[2] * c0[2])) / sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]));
        }
    } else {
        r0 = sp_interior(A, b, m, c, c0, newton);
    }
    if (!(r0 > 0.0) || !sp_finite(r0)) return SETS_NO_INTERIOR;
    double x[9] = {0.5 * r0, 0.0, 0.5 * r0, 0.0, 0.0, 0.5 * r0, c0[0], c0[1], c0[2]};
    const bool ok = fixed ? sp_mvie_newton<6>(A, b, m, c0, x, newton) : sp_mvie_newton<9>(A, b, m, c0, x, newton);
    if (!ok) return SETS_NUMERICAL;
    const double L[9] = {x[0], 0.0, 0.0, x[1], x[2], 0.0, x[3], x[4], x[5]};
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) q[3 * r + k] = L[3 * r] * L[3 * k] + L[3 * r + 1] * L[3 * k + 1] + L[3 * r + 2] * L[3 * k + 2];
    if (!fixed) { c[0] = x[6]; c[1] = x[7]; c[2] = x[8]; }
    for (int k = 0; k < 9; k++) if (!sp_finite(q[k])) return SETS_NUMERICAL;
    return SETS_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// one lane
// ------------------------------------------------------------------------------------------------------------------------------
struct SetResult { int nrows, rounds, newton, collision, status; };

// find_set_around_point(p, fixed_mid, optimize): rows in A / b, q_ellipse qe [9], centre c [3]
BMPC_INL SetResult sets_point_lane(const SetScene& sc, const double* p, bool fixed_mid, bool optimize, double* dist, int ds, double* A,
                                   double* b, double* qe, double* c) {
    SetResult res{0, 0, 0, 0, SETS_OK};
    double E[9] = {1e-4, 0, 0, 0, 1e-4, 0, 0, 0, 1e-4}, Qe[9] = {1e4, 0, 0, 0, 1e4, 0, 0, 0, 1e4};
    double ps[3] = {p[0], p[1], p[2]};
    for (int k = 0; k < 9; k++) qe[k] = Qe[k];
    for (int k = 0; k < 3; k++) c[k] = ps[k];
    if (!sp_finite(p[0]) || !sp_finite(p[1]) || !sp_finite(p[2])) { res.status = SETS_NUMERICAL; return res; }
    double det_old = 1.0, det = 100.0;
    int n = 0;
    while (fabs(det - det_old) / det_old > 0.01) {
        if (res.rounds >= SETS_MAX_ROUNDS) break;
        res.rounds++;
        n = sp_polyhedron(sc, E, Qe, ps, dist, ds, A, b);
        if (n < 0) { res.status = -n; return res; }
        res.nrows = n;
        if (!optimize) return res;
        det_old = det;
        const int st = sp_mvie(A, b, n, fixed_mid, ps, E, res.newton);
        if (st != SETS_OK) { res.status = st; return res; }
        det = 1.0 / sp_inv3(E, Qe);
        if (sp_min_eig_sym3(E) < 1e-3) break;       // the ellipsoid collapsed (fixed centre on a face)
    }
    if (fixed_mid) {
        const int st = sp_mvie(A, b, n, false, ps, E, res.newton);
        if (st != SETS_OK) { res.status = st; return res; }
        sp_inv3(E, Qe);
    }
    for (int k = 0; k < 9; k++) qe[k] = Qe[k];
    for (int k = 0; k < 3; k++) c[k] = ps[k];
    return res;
}

// find_set_collision_avoidance(p0, p1, compute_ellipsoid=True)
BMPC_INL SetResult sets_segment_lane(const SetScene& sc, const double* p0, const double* p1, double* dist, int ds, double* A, double* b,
                                     double* qe, double* c) {
    SetResult res{0, 1, 0, 0, SETS_OK};
    for (int k = 0; k < 9; k++) qe[k] = 0.0;
    for (int k = 0; k < 3; k++) c[k] = 0.5 * (p0[k] + p1[k]);
    for (int k = 0; k < 3; k++)
        if (!sp_finite(p0[k]) || !sp_finite(p1[k])) { res.status = SETS_NUMERICAL; return res; }
    sp_init_rows(sc, A, b);
    const LoopScene& ob = sc.obs;
    double cp[LP_CRES];
    auto pair = [&](int i) -> const double* {       // computed again when its obstacle is chosen (deterministic), not stored
        loop_closest_pair(ob.A + 3 * SETS_OROWS * i, ob.b + SETS_OROWS * i, ob.AAt + SETS_OROWS * SETS_OROWS * i, ob.nrows[i], nullptr, p0, p1, cp);
        return cp;
    };
    for (int i = 0; i < ob.n_obs; i++) dist[i * ds] = pair(i)[6];
    bool touched;
    const int n = separating_halfspaces(ob, pair, dist, ds, p0, p1, SETS_ROWS, A, b, 6, touched);
    res.collision = touched;
    if (n == FS_OVERFLOW) { res.status = SETS_TOO_MANY_ROWS; return res; }
    if (n == FS_NUMERICAL) { res.status = SETS_NUMERICAL; return res; }
    res.nrows = n;
    double q[9];
    const int st = sp_mvie(A, b, n, false, c, q, res.newton);
    if (st != SETS_OK) { res.status = st; return res; }
    sp_inv3(q, qe);
    return res;
}

// row i of A A^T of obstacle o (SetScene::AAt: the segment mode's projections), zero past the obstacle's rows
BMPC_INL void sets_aat_row(const double* A, const int* nrows, int o, int i, double* AAt) {
    const double* a = A + 3 * SETS_OROWS * o;
    for (int j = 0; j < SETS_OROWS; j++) {
        double v = 0.0;
        if (i < nrows[o] && j < nrows[o]) v = a[3 * i] * a[3 * j] + a[3 * i + 1] * a[3 * j + 1] + a[3 * i + 2] * a[3 * j + 2];
        AAt[SETS_OROWS * SETS_OROWS * o + SETS_OROWS * i + j] = v;
    }
}

}  // namespace bmpc
