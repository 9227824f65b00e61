// The curvature block of k_curv (curvature_emit, bmpc_pair_kernels.hpp) beside the formulation it replaced -- TEST INFRASTRUCTURE ONLY
// (tests/test_curvature_contraction.py).  curvature_emit_loop below is that earlier formulation, statement for statement -- the sum
// over j inside every (a, bq) entry, all 28 entries in one nest -- with the scalar type as a template parameter, so that the same
// text evaluates in double (what the kernel used to compute) and in long double (the value both are measured against).
#include <cmath>
#include <cstdlib>
#define BMPC_ATOMIC_INC(ptr) __atomic_fetch_add((ptr), 1, __ATOMIC_RELAXED)
#include "emu_platform.hpp"

#include "../../boundplanner_amd/csrc/bmpc_pair_kernels.hpp"
#include "../../boundplanner_amd/csrc/bmpc_robot.hpp"

using namespace bmpc;

template <class T> static inline void cross3t(const T* a, const T* b, T* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
template <class T> static inline T dot3t(const T* a, const T* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// KinT, Jl and the forces in the scalar type T (converted from the doubles the kernel has: they are the block's inputs, exact here)
template <class T> struct KinTT { T o[7][3], zx[7][3], pee[3], pl4[3]; };

template <class T> struct Capture {
    T* out; int f;
    void put(T v) { out[f++] = v; }
};

template <class T>
static void curvature_emit_loop(const KinTT<T>& K, const T Jl[3][7], const T* dq, const T* Fp, const T* Fv,
                                const T Fc[6][3], const T* sa, const T* sbq, const T* sbdq, T sc1, Capture<T>& E) {
    const int njc[6] = {2, 3, 4, 5, 6, 4};
    // q x q block: third derivatives of the kinematics contracted with forces and dq -- symmetric in (a, bq), so the upper
    // triangle is computed and both halves are emitted from it
    T tri[28];
    for (int a = 0; a < 7; a++)
        for (int bq = a; bq < 7; bq++) {
            const int m = a < bq ? a : bq, M = a < bq ? bq : a;
            T cM[3] = {Jl[0][M], Jl[1][M], Jl[2][M]}, zc[3];
            cross3t(K.zx[m], cM, zc);
            T acc = dot3t(Fp, zc);
            for (int c = 0; c < 6; c++)
                if (M < njc[c]) {
                    const T* pc = (c < 5) ? K.o[c + 2] : K.pl4;
                    T r[3] = {pc[0] - K.o[M][0], pc[1] - K.o[M][1], pc[2] - K.o[M][2]}, cc[3];
                    cross3t(K.zx[M], r, cc);
                    cross3t(K.zx[m], cc, zc);
                    acc += dot3t(Fc[c], zc);
                }
            for (int j = 0; j < 7; j++) {
                const int m1 = a < j ? a : j, M1 = a < j ? j : a;
                T c1[3] = {Jl[0][M1], Jl[1][M1], Jl[2][M1]};
                T t1[3] = {0, 0, 0}, t2[3], dzm[3], dcM[3];
                if (bq < m1) { cross3t(K.zx[bq], K.zx[m1], dzm); cross3t(dzm, c1, t1); }
                const int m2 = bq < M1 ? bq : M1, M2 = bq < M1 ? M1 : bq;
                T c2[3] = {Jl[0][M2], Jl[1][M2], Jl[2][M2]};
                cross3t(K.zx[m2], c2, dcM);
                cross3t(K.zx[m1], dcM, t2);
                T lin = Fv[0] * (t1[0] + t2[0]) + Fv[1] * (t1[1] + t2[1]) + Fv[2] * (t1[2] + t2[2]);
                T ang = 0;
                if (a < j) {
                    T u1[3] = {0, 0, 0}, u2[3] = {0, 0, 0}, tmp[3];
                    if (bq < a) { cross3t(K.zx[bq], K.zx[a], tmp); cross3t(tmp, K.zx[j], u1); }
                    if (bq < j) { cross3t(K.zx[bq], K.zx[j], tmp); cross3t(K.zx[a], tmp, u2); }
                    ang = Fv[3] * (u1[0] + u2[0]) + Fv[4] * (u1[1] + u2[1]) + Fv[5] * (u1[2] + u2[2]);
                }
                acc += dq[j] * (lin + ang);
            }
            tri[sym7(a, bq)] = acc + (sc1 * sa[a] * sa[bq] + sbq[a] * sa[bq] + sa[a] * sbq[bq]);
        }
    for (int a = 0; a < 7; a++)
        for (int bq = 0; bq < 7; bq++) E.put(tri[sym7(a, bq)]);
    for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++) {
            const int m = i < j ? i : j, M = i < j ? j : i;
            T cM[3] = {Jl[0][M], Jl[1][M], Jl[2][M]}, zc[3];
            cross3t(K.zx[m], cM, zc);
            T acc = dot3t(Fv, zc);
            if (i < j) { T zz[3]; cross3t(K.zx[i], K.zx[j], zz); acc += dot3t(Fv + 3, zz); }
            E.put(acc + sa[i] * sbdq[j]);
        }
}

template <class T>
static void run_loop(const KinT& K, const double Jl[3][7], const double* dq, const double* Fp, const double* Fv, const double* Fc,
                     const double* sa, const double* sbq, const double* sbdq, double sc1, T* out) {
    KinTT<T> KT;
    T JT[3][7], dqT[7], FpT[3], FvT[6], FcT[6][3], saT[7], sbqT[7], sbdqT[7];
    for (int i = 0; i < 7; i++)
        for (int a = 0; a < 3; a++) { KT.o[i][a] = K.o[i][a]; KT.zx[i][a] = K.zx[i][a]; JT[a][i] = Jl[a][i]; }
    for (int a = 0; a < 3; a++) { KT.pee[a] = K.pee[a]; KT.pl4[a] = K.pl4[a]; FpT[a] = Fp[a]; }
    for (int a = 0; a < 6; a++) FvT[a] = Fv[a];
    for (int c = 0; c < 6; c++)
        for (int a = 0; a < 3; a++) FcT[c][a] = Fc[3 * c + a];
    for (int i = 0; i < 7; i++) { dqT[i] = dq[i]; saT[i] = sa[i]; sbqT[i] = sbq[i]; sbdqT[i] = sbdq[i]; }
    Capture<T> E{out, 0};
    curvature_emit_loop<T>(KT, JT, dqT, FpT, FvT, FcT, saT, sbqT, sbdqT, (T)sc1, E);
}

// n samples: q, dq, sa, sbq, sbdq [n][7], Fp [n][3], Fv [n][6], Fc [n][18], sc1 [n].  Per sample and per block (0: q x q, 1: q x dq):
// err_new / err_old [n][2] = max |entry - long double value| of curvature_emit / of the loop formulation in double, scale [n][2] =
// max |long double value|; out_new / out_old [n][98] the two sets of entries themselves.
extern "C" int emu_curv_compare(int n, const double* q, const double* dq, const double* Fp, const double* Fv, const double* Fc,
                                const double* sa, const double* sbq, const double* sbdq, const double* sc1, double* err_new,
                                double* err_old, double* scale, double* out_new, double* out_old) {
    RobotConst rc;
    fill_robot_const(rc);
    for (int s = 0; s < n; s++) {
        KinT K;
        double Jl[3][7], Fc63[6][3];
        kin_chain(&rc, q + 7 * s, K);
        kin_jlin(K, Jl);
        for (int c = 0; c < 6; c++)
            for (int a = 0; a < 3; a++) Fc63[c][a] = Fc[18 * s + 3 * c + a];
        double* on = out_new + 98 * s;
        double* oo = out_old + 98 * s;
        long double ref[98];
        Capture<double> E{on, 0};
        curvature_emit(K, Jl, dq + 7 * s, Fp + 3 * s, Fv + 6 * s, Fc63, sa + 7 * s, sbq + 7 * s, sbdq + 7 * s, sc1[s], E);
        if (E.f != 98) return 1;
        run_loop<double>(K, Jl, dq + 7 * s, Fp + 3 * s, Fv + 6 * s, Fc + 18 * s, sa + 7 * s, sbq + 7 * s, sbdq + 7 * s, sc1[s], oo);
        run_loop<long double>(K, Jl, dq + 7 * s, Fp + 3 * s, Fv + 6 * s, Fc + 18 * s, sa + 7 * s, sbq + 7 * s, sbdq + 7 * s, sc1[s], ref);
        for (int blk = 0; blk < 2; blk++) {
            long double en = 0, eo = 0, sc = 0;
            for (int i = 49 * blk; i < 49 * (blk + 1); i++) {
                en = std::fmax(en, std::fabs((long double)on[i] - ref[i]));
                eo = std::fmax(eo, std::fabs((long double)oo[i] - ref[i]));
                sc = std::fmax(sc, std::fabs(ref[i]));
            }
            err_new[2 * s + blk] = (double)en; err_old[2 * s + blk] = (double)eo; scale[2 * s + blk] = (double)sc;
        }
    }
    return 0;
}
