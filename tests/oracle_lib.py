"""ctypes access to the CPU oracle (oracle/libbmpc_oracle.so) -- TEST INFRASTRUCTURE ONLY.
Imported by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg; never by the
product package."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "oracle", "libbmpc_oracle.so")
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)


class Opts(ctypes.Structure):
    _fields_ = [("N", ctypes.c_int), ("dt", ctypes.c_double), ("tol", ctypes.c_double),
                ("max_iter", ctypes.c_int), ("verbose", ctypes.c_int), ("hess", ctypes.c_int), ("mu_strategy", ctypes.c_int), ("hess_switch", ctypes.c_double), ("mu_init", ctypes.c_double), ("kappa_mu", ctypes.c_double), ("theta_mu", ctypes.c_double), ("kappa_eps", ctypes.c_double),
                ("inertia", ctypes.c_int), ("dw0", ctypes.c_double), ("inertia_err", ctypes.c_double), ("stall_n", ctypes.c_int),
                ("gn_backoff", ctypes.c_int), ("slack_reset", ctypes.c_int), ("ls_alpha_mem", ctypes.c_double), ("mu_floor_k", ctypes.c_double),
                ("soc", ctypes.c_int), ("soc_after", ctypes.c_int), ("pi_shoot", ctypes.c_int)]


def _P(a):
    return a.ctypes.data_as(_dp)


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
        _lib = ctypes.CDLL(LIB)
        _lib.bmpc_oracle_eval.restype = ctypes.c_int
        _lib.bmpc_oracle_solve.restype = ctypes.c_int
    return _lib


def set_robot(table=None):
    """table: boundplanner_amd.robots table (dict) or None for the iiwa14 -- process-wide."""
    if table is None:
        lib().bmpc_oracle_set_robot(None, None, None, None, None)
        return
    a = lambda k: np.ascontiguousarray(table[k], float)
    xyz, rpy, ee, eer, l4 = a("joint_xyz"), a("joint_rpy"), a("ee_xyz"), a("ee_rpy"), a("link4_col_xyz")
    lib().bmpc_oracle_set_robot(_P(xyz), _P(rpy), _P(ee), _P(eer), _P(l4))


def fk_batch(q, dq=None):
    q = np.ascontiguousarray(q, float).reshape(-1, 7)
    dq = np.zeros_like(q) if dq is None else np.ascontiguousarray(dq, float).reshape(-1, 7)
    B = q.shape[0]
    out = dict(ee_pos=np.zeros((B, 3)), ee_rot=np.zeros((B, 3, 3)), col_pts=np.zeros((B, 6, 3)),
               jac=np.zeros((B, 6, 7)), dvdq=np.zeros((B, 6, 7)))
    L = lib()
    for b in range(B):
        L.bmpc_oracle_fk(_P(q[b]), _P(dq[b]), _P(out["ee_pos"][b]), _P(out["ee_rot"][b]),
                         _P(out["col_pts"][b]), _P(out["jac"][b]), _P(out["dvdq"][b]))
    return out


def nlp_eval(N, w, p, dt=0.1, jac=True):
    n_w, n_g = 44 * N + 6, 147 * (N - 1) + 21
    w = np.ascontiguousarray(w, float); p = np.ascontiguousarray(p, float)
    f = ctypes.c_double()
    g = np.zeros(n_g); gr = np.zeros(n_w)
    J = np.zeros((n_g, n_w)) if jac else None
    rc = lib().bmpc_oracle_eval(N, ctypes.c_double(dt), _P(w), _P(p), ctypes.byref(f), _P(g), _P(gr),
                                _P(J) if jac else None)
    assert rc == 0
    return f.value, g, gr, J


def gbounds(N):
    n_g = 147 * (N - 1) + 21
    lb = np.zeros(n_g); ub = np.zeros(n_g)
    lib().bmpc_oracle_gbounds(N, _P(lb), _P(ub))
    return lb, ub


def solve(N, x0, lbx, ubx, p, dt=0.1, tol=1e-5, max_iter=100, verbose=0, hess=2, mu_strategy=1, hess_switch=1.0, mu_init=0.1, kappa_mu=0.1, theta_mu=2.0, kappa_eps=1000.0, inertia=2, dw0=1e-4, inertia_err=1e-2, stall_n=8, mu_floor_k=1e4, gn_backoff=2, slack_reset=1, ls_alpha_mem=0.0, soc=0, soc_after=0, pi_shoot=0):
    n_w, n_g = 44 * N + 6, 147 * (N - 1) + 21
    o = Opts(N, dt, tol, max_iter, verbose, hess, mu_strategy, hess_switch, mu_init, kappa_mu, theta_mu, kappa_eps, inertia, dw0, inertia_err, stall_n, gn_backoff, slack_reset, ls_alpha_mem, mu_floor_k, soc, soc_after, pi_shoot)
    lbx = np.where(np.isinf(lbx), -1e20, lbx); ubx = np.where(np.isinf(ubx), 1e20, ubx)
    x0, lbx, ubx, p = (np.ascontiguousarray(a, float) for a in (x0, lbx, ubx, p))
    x = np.zeros(n_w); g = np.zeros(n_g); lg = np.zeros(n_g); lx = np.zeros(n_w)
    f = ctypes.c_double(); it = ctypes.c_int(); st = ctypes.c_int(); viol = ctypes.c_double()
    lib().bmpc_oracle_solve(ctypes.byref(o), _P(x0), _P(lbx), _P(ubx), _P(p), _P(x), _P(g), _P(lg), _P(lx),
                            ctypes.byref(f), ctypes.byref(it), ctypes.byref(st), ctypes.byref(viol))
    return dict(x=x, g=g, lam_g=lg, lam_x=lx, f=f.value, iters=it.value, status=st.value, viol=viol.value)


def solve_batch(N, x0, lbx, ubx, p, dt=0.1, tol=1e-5, max_iter=100, nthreads=0, hess=2, mu_strategy=1, hess_switch=1.0, mu_init=0.1, kappa_mu=0.1, theta_mu=2.0, kappa_eps=1000.0, inertia=2, dw0=1e-4, inertia_err=1e-2, stall_n=8, mu_floor_k=1e4, gn_backoff=2, slack_reset=1, ls_alpha_mem=0.0, soc=0, soc_after=0, pi_shoot=0):
    B = x0.shape[0]
    o = Opts(N, dt, tol, max_iter, 0, hess, mu_strategy, hess_switch, mu_init, kappa_mu, theta_mu, kappa_eps, inertia, dw0, inertia_err, stall_n, gn_backoff, slack_reset, ls_alpha_mem, mu_floor_k, soc, soc_after, pi_shoot)
    lbx = np.where(np.isinf(lbx), -1e20, lbx); ubx = np.where(np.isinf(ubx), 1e20, ubx)
    x0, lbx, ubx, p = (np.ascontiguousarray(a, float) for a in (x0, lbx, ubx, p))
    x = np.zeros_like(x0); f = np.zeros(B); viol = np.zeros(B)
    it = np.zeros(B, np.int32); st = np.zeros(B, np.int32)
    lib().bmpc_oracle_solve_batch(ctypes.byref(o), B, _P(x0), _P(lbx), _P(ubx), _P(p), _P(x), _P(f),
                                  it.ctypes.data_as(_ip), st.ctypes.data_as(_ip), _P(viol), nthreads)
    return dict(x=x, f=f, iters=it, status=st, viol=viol)


INFO_FIELDS = ("iters", "status", "mu", "alpha", "alpha_dual", "alpha_ftb", "delta_w", "hess_next", "retries", "backtracks", "err_prev", "stall")


def solve_batch_info(N, x0, lbx, ubx, p, nthreads=0, **kw):
    """solve_batch + info [B][12]: the decisions of the last iteration of every solve (bmpc_oracle_solve_batch_info)."""
    B = x0.shape[0]
    d = dict(dt=0.1, tol=1e-5, max_iter=100, hess=2, mu_strategy=1, hess_switch=1.0, mu_init=0.1, kappa_mu=0.1, theta_mu=2.0, kappa_eps=1000.0,
             inertia=2, dw0=1e-4, inertia_err=1e-2, stall_n=8, mu_floor_k=1e4, gn_backoff=2, slack_reset=1, ls_alpha_mem=0.0, soc=0, soc_after=0, pi_shoot=0)
    d.update(kw)
    o = Opts(N, d["dt"], d["tol"], d["max_iter"], 0, d["hess"], d["mu_strategy"], d["hess_switch"], d["mu_init"], d["kappa_mu"], d["theta_mu"],
             d["kappa_eps"], d["inertia"], d["dw0"], d["inertia_err"], d["stall_n"], d["gn_backoff"], d["slack_reset"], d["ls_alpha_mem"],
             d["mu_floor_k"], d["soc"], d["soc_after"], d["pi_shoot"])
    lbx = np.where(np.isinf(lbx), -1e20, lbx); ubx = np.where(np.isinf(ubx), 1e20, ubx)
    x0, lbx, ubx, p = (np.ascontiguousarray(a, float) for a in (x0, lbx, ubx, p))
    x = np.zeros_like(x0); f = np.zeros(B); viol = np.zeros(B); info = np.zeros((B, 12))
    it = np.zeros(B, np.int32); st = np.zeros(B, np.int32)
    lib().bmpc_oracle_solve_batch_info(ctypes.byref(o), B, _P(x0), _P(lbx), _P(ubx), _P(p), _P(x), _P(f),
                                       it.ctypes.data_as(_ip), st.ctypes.data_as(_ip), _P(viol), _P(info), nthreads)
    return dict(x=x, f=f, iters=it, status=st, viol=viol, info=info)


MAXROWS = 216


def _opts(N, dt):
    return Opts(N, dt, 1e-5, 100, 0, 1, 1, 1.0, 0.1, 0.1, 2.0, 1000.0, 2, 1e-4, 1e-2, 8, 2, 1, 0.0, 1e4, 0, 0, 0)


def _boxes(lbx, ubx):
    return np.where(np.isinf(lbx), -1e20, lbx), np.where(np.isinf(ubx), 1e20, ubx)


def stage_rows(N, w, lbx, ubx, p, dt=0.1):
    """The rows the oracle builds per stage k = 1 .. N-1 at w (bmpc_oracle_stage_rows): nrows [N-1], meta [N-1][216][6] =
    (gidx, gsign, xidx, kind, i0, i1), coef [N-1][216][2]."""
    lbx, ubx = _boxes(lbx, ubx)
    w, lbx, ubx, p = (np.ascontiguousarray(a, float) for a in (w, lbx, ubx, p))
    nrows = np.zeros(N - 1, np.int32); meta = np.full((N - 1, MAXROWS, 6), -1, np.int32); coef = np.zeros((N - 1, MAXROWS, 2))
    o = _opts(N, dt)
    rc = lib().bmpc_oracle_stage_rows(ctypes.byref(o), _P(w), _P(lbx), _P(ubx), _P(p), nrows.ctypes.data_as(_ip),
                                      meta.ctypes.data_as(_ip), _P(coef))
    assert rc == MAXROWS
    return nrows, meta, coef


def stage_matrices(N, w, lbx, ubx, p, t, z, lam_pi, dt=0.1):
    """Stage matrices H [N-1][41][41] (zeta coordinates, exact Hessian) at w for given row (t, z) [N-1][216] and adjoint
    multipliers of the pi dynamics lam_pi [N][3] (bmpc_oracle_stage_matrices)."""
    lbx, ubx = _boxes(lbx, ubx)
    w, lbx, ubx, p, t, z, lam_pi = (np.ascontiguousarray(a, float) for a in (w, lbx, ubx, p, t, z, lam_pi))
    assert t.shape == z.shape == (N - 1, MAXROWS) and lam_pi.shape == (N, 3)
    H = np.zeros((N - 1, 41, 41))
    o = _opts(N, dt)
    rc = lib().bmpc_oracle_stage_matrices(ctypes.byref(o), _P(w), _P(lbx), _P(ubx), _P(p), _P(t), _P(z), _P(lam_pi), _P(H))
    assert rc == 0
    return H


def newton_system(N, w, lbx, ubx, p, t, z, hess_mode, mu, dw=0.0, dt=0.1, step=True):
    """The linear system of one interior-point iteration at w for given row (t, z) [N-1][216], Hessian mode and barrier parameter
    (bmpc_oracle_newton_system): dict of H [N-1][41][41] (no delta_w), g, gdual [N-1][41], A [N-1][32][32], B [N-1][32][9],
    r [N-1][32], r0 [24], lam [N][32], nrows [N-1], h [N-1][216], a [N-1][216][41]; with step: dzeta [N-1][41], the oracle's own
    Riccati step with delta_w = dw (None when its recursion met a block that is not positive definite)."""
    lbx, ubx = _boxes(lbx, ubx)
    w, lbx, ubx, p, t, z = (np.ascontiguousarray(a, float) for a in (w, lbx, ubx, p, t, z))
    assert t.shape == z.shape == (N - 1, MAXROWS)
    S = N - 1
    d = dict(H=np.zeros((S, 41, 41)), g=np.zeros((S, 41)), gdual=np.zeros((S, 41)), A=np.zeros((S, 32, 32)), B=np.zeros((S, 32, 9)),
             r=np.zeros((S, 32)), r0=np.zeros(24), lam=np.zeros((N, 32)), nrows=np.zeros(S, np.int32), h=np.zeros((S, MAXROWS)),
             a=np.zeros((S, MAXROWS, 41)))
    dz = np.zeros((S, 41))
    o = _opts(N, dt)
    f = lib().bmpc_oracle_newton_system
    f.restype = ctypes.c_int
    rc = f(ctypes.byref(o), _P(w), _P(lbx), _P(ubx), _P(p), _P(t), _P(z), int(hess_mode), ctypes.c_double(mu), ctypes.c_double(dw),
           _P(d["H"]), _P(d["g"]), _P(d["gdual"]), _P(d["A"]), _P(d["B"]), _P(d["r"]), _P(d["r0"]), _P(d["lam"]),
           d["nrows"].ctypes.data_as(_ip), _P(d["h"]), _P(d["a"]), _P(dz) if step else None)
    assert rc in (0, 1)
    d["dzeta"] = dz if (step and rc == 0) else None
    return d


def trial_point(N, lbx, ubx, p, zeta0, dzeta, t0, c, alpha, dt=0.1):
    """The oracle's own trial point (bmpc_oracle_trial_point): (t1 [N-1][216], f1, th1, ls1) for the iterate zeta0 [N-1][41] with
    slacks t0 [N-1][216] (oracle row order), the step dzeta and c = t0 + dt, and the step length alpha."""
    lbx, ubx = _boxes(lbx, ubx)
    lbx, ubx, p, zeta0, dzeta, t0, c = (np.ascontiguousarray(a, float) for a in (lbx, ubx, p, zeta0, dzeta, t0, c))
    assert zeta0.shape == dzeta.shape == (N - 1, 41) and t0.shape == c.shape == (N - 1, MAXROWS)
    t1 = np.zeros((N - 1, MAXROWS))
    f1, th1, ls1 = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    o = _opts(N, dt)
    rc = lib().bmpc_oracle_trial_point(ctypes.byref(o), _P(lbx), _P(ubx), _P(p), _P(zeta0), _P(dzeta), _P(t0), _P(c), ctypes.c_double(alpha),
                                       _P(t1), ctypes.byref(f1), ctypes.byref(th1), ctypes.byref(ls1))
    assert rc == 0
    return t1, f1.value, th1.value, ls1.value


KKT_FIELDS = ("dual", "prim", "cmax", "cmin", "zsum", "lamsum", "nrows", "sd", "sc", "err", "status", "mu_new")


def kkt_control(N, w, lbx, ubx, p, t, z, mu, it, dt=0.1, tol=1e-5, max_iter=100, mu_floor_k=1e4):
    """The KKT error and the iteration control of the oracle's solve loop at w for given row (t, z) [N-1][216], barrier parameter
    and iteration counter (bmpc_oracle_kkt_control): dict of KKT_FIELDS (status -1: the iteration goes on, with mu_new)."""
    lbx, ubx = _boxes(lbx, ubx)
    w, lbx, ubx, p, t, z = (np.ascontiguousarray(a, float) for a in (w, lbx, ubx, p, t, z))
    assert t.shape == z.shape == (N - 1, MAXROWS)
    o = _opts(N, dt)
    o.tol, o.max_iter, o.mu_floor_k = tol, max_iter, mu_floor_k
    out = np.zeros(12)
    rc = lib().bmpc_oracle_kkt_control(ctypes.byref(o), _P(w), _P(lbx), _P(ubx), _P(p), _P(t), _P(z), ctypes.c_double(mu), int(it), _P(out))
    assert rc == 0
    d = dict(zip(KKT_FIELDS, (float(v) for v in out)))
    d["status"], d["nrows"] = int(out[10]), int(out[6])
    return d


def debug_hess(N, w, lbx, ubx, p, k, zval, lamval, dt=0.1):
    """(analytic, finite-difference) Lagrangian Hessian of stage k without barrier terms (bmpc_oracle_debug_hess)."""
    lbx, ubx = _boxes(lbx, ubx)
    w, lbx, ubx, p = (np.ascontiguousarray(a, float) for a in (w, lbx, ubx, p))
    Ha, Hf = np.zeros((41, 41)), np.zeros((41, 41))
    o = _opts(N, dt)
    lib().bmpc_oracle_debug_hess(ctypes.byref(o), _P(w), _P(lbx), _P(ubx), _P(p), k, ctypes.c_double(zval), ctypes.c_double(lamval),
                                 _P(Ha), _P(Hf))
    return Ha, Hf
