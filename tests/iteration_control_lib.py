"""Step-level pin: the KKT error and the iteration control of one interior-point iteration -- TEST INFRASTRUCTURE.

What is checked: what decides whether there is another iteration and with which Hessian, barrier parameter and delta_w -- the scaled
KKT error, the termination test, the barrier update, the stall bookkeeping, the sequence of factorisation attempts
(ric_kkt_and_barrier, ric_note_err, ric_attempt_next, ric_finish, the partial sums of k_eval, k_ric_att + k_ric_sel) and the Hessian
choice at the end of ls_decide.  This file holds no adjoint recursion and no code from the kernels or the oracle.

Continuous quantities, from the kernel's OWN returned zeta0, t0, z0 (np.longdouble sums):
  * prim = max(|h_i + t_i|, |r_k|, |r0|), cmax / cmin = max / min t_i z_i, zsum = sum z_i, nrows: h from line_search_lib.rows_h (the
    pinned g and the box of w through the row table), r_k and r0 from line_search_lib.defects / x1fix_of;
  * dual = max |Z^T gdual| over the 8 free entries of x_1 and the 9 controls of every stage, Z built densely by forward propagation
    through A_k, B_k; lamsum = the 1-norm of the solution of lam_k - A_k^T lam_{k+1} = gdual_k[:32] (np.linalg.solve on the
    block-bidiagonal matrix).  gdual_k = grad_zeta_k [f(w(zeta)) + sum z_i h_i(w(zeta))] and the pi rows of A_k, B_k are the oracle's
    (bmpc_oracle_newton_system), HELD by first_order_check to Richardson-extrapolated central differences of the pinned f, rows_h
    and defects along w_of_zeta within 10 x the difference's own error estimate + 1e-9 x the sum of the absolute terms (the rule of
    the D and Hessian pins); outside the pi rows A, B are newton_step_lib.dynamics_constant_part(dt), asserted;
  * neq = 32 (N - 2) + 24, sd = max(100, (lamsum + zsum) / (neq + nrows)) / 100, sc = max(100, zsum / nrows) / 100,
    err = max(dual / sd, prim, cmax / sc).
Each is measured relative to the sum of the absolute values of the terms of the entry that decides it.

The rule (replay), written from Waechter & Biegler, Math. Prog. 106 (2006): the scaled error E_0 of eq. (5) with s_max = 100, the
barrier test E_mu <= kappa_eps mu of eq. (6) and the update mu <- max(tol / 10, min(kappa_mu mu, mu^theta_mu)) of eq. (7), the
inertia correction of Algorithm IC.  This project's deviations, read off the code (oracle/bmpc_solve.c, bmpc_ric_kernel.hpp,
ls_decide):
  * s_d uses the adjoint multipliers of the dynamics in zeta coordinates;
  * convergence needs err <= tol AND dual <= 1, prim <= 1e-4, cmax <= 1e-4, and is tested before the iteration limit;
  * the first test of the barrier loop is two-sided, max(|cmax - mu|, |cmin - mu|) / sc; later ones use max(cmax - mu, 0) / sc;
  * a decrease is floored: max(mu_new, min(E_mu / mu_floor_k, 0.1)), and the loop breaks (mu restored) when that is no decrease;
  * mu >= tol / 10 (mu_new is compared exactly, except where it went through pow(mu, theta_mu): POW_ULPS);
  * stall bookkeeping: err < 0.9 err_best resets the counter and records err, anything else counts up;
  * a failed exact attempt is answered by Gauss-Newton while the PREVIOUS iterate's error > inertia_err and its stall counter <
    stall_n (gn_ok), by delta_w otherwise;
  * ladder: dw0, then x 100 without history; max(1e-20, dw_last / 3), then x 8 with it; dead (status 3) after 14 tries or above 1e20;
  * gn_back is 1, 2, ... up to gn_backoff after a fallback (gn_skip = gn_back), reset by an exact step that goes through at once;
    dw_last is updated only when the accepted attempt carries a delta_w;
  * after the search: the exact Hessian is wanted when err < hess_switch or stall >= stall_n (the values just recorded), and held off
    with a decrement while gn_skip > 0.
Which attempt succeeds is decided independently: attempt j succeeds iff Z^T Hf_j Z (newton_step_lib.full_hessians, Dense.M) is
positive definite by eigvalsh; a smallest eigenvalue within 1e-9 x the largest is undecidable.  Every comparison of the rule against a
threshold is replayed on the reference's values; one whose margin lies below the bound of the quantity compared is undecidable, and at
most MAX_LEFT_OUT of a case's instances may be left out for that.
What is NOT compared: for the profiles of NO_ATTEMPTS (exact solutions "x" and "d", whose barrier terms make every attempt undecidable
by that rule) delta_w, tries, gn_back, gn_skip, dw_last and hess_mode after the search; they are compared up to the stall bookkeeping
(status, err, mu, stall, err_best), which is what their classes -- termination and the barrier loop -- need.  Profile "b" runs with the
slacks of the Newton pin's rows raised to T_MIN_B at the same t z, so that its attempts are decidable and every field is compared.
"""
import numpy as np

import hessian_pin_lib as HP
import line_search_lib as L
import newton_step_lib as NS

LD = np.longdouble
EPS = float(np.finfo(float).eps)
NX, NU, NZ = 32, 9, 41
PIR = slice(21, 24)
OPTS = dict(tol=1e-5, max_iter=100, hess_switch=1.0, inertia_err=1e-2, stall_n=8, gn_backoff=2, mu_floor_k=1e4, dw0=1e-4,
            kappa_eps=1000.0, kappa_mu=0.1, theta_mu=2.0, mu_init=0.1)
RIC_NATT = 5                       # attempts k_ric_att speculates on at most (bmpc_pipeline.hpp; three under the emulation)
PLANT = ("mu", "err_prev", "err_best", "stall", "dw_last", "gn_back", "gn_skip", "it")
CTL = {n: i for i, n in enumerate(("state", "status", "mu", "delta_w", "tries", "ksel", "hess_mode", "err_prev", "err_best", "stall", "dw_last",
                                   "gn_back", "gn_skip", "it", "fk", "it_after", "hess_mode_after", "gn_skip_after", "state_after"))}
CONTROL = [i for n, i in CTL.items() if n != "ksel"]      # (ksel: which copy of the gains the forward sweep reads, not a control field)
INIT = dict(mu=0.1, err_prev=1e300, err_best=1e300, stall=0, dw_last=0.0, gn_back=0, gn_skip=0, it=0)
ST_DONE = 3
MAX_LEFT_OUT = NS.MAX_LEFT_OUT
FACTOR = 32.0
MARGIN = L.MARGIN
EIG_REL = 1e-9
# mu^theta_mu is pow(): within 1 ulp of the true power on the device (the documented bound of HIP's double-precision pow), within
# 1 ulp in the reference's libm; a barrier parameter that went through it is compared to 2 ulps, every other one exactly
POW_ULPS = 2.0
ZT_MAX = 3e4                       # largest barrier term z / t of profile "s"
T_MIN_B = 1e-5                     # smallest slack of profile "b" here (1e-8 in the Newton pin)


# ---------------------------------------------------------------- inputs
def slots_of(N, rows):
    nrows, meta, coef = rows
    slot = np.full((N - 1, HP.MAXROWS), -1, int)
    for k in range(1, N):
        for r in range(nrows[k - 1]):
            s = HP.slot_of_row(N, k, meta[k - 1, r], HP.ORACLE_Y_NAMES)
            slot[k - 1, r] = s + (1 if 0 <= meta[k - 1, r, 2] < 28 * N and coef[k - 1, r, 0] < 0 else 0)
    return slot


def make_solved_batch(N, B, seed, O, exact, c_small=1e-9, heavy=False):
    """points at and near solutions, with consistent rows: the solution of a tight oracle solve (tol 1e-8) -- profile "x" (exact): as it
    is, rows t = max(-h, 5e-7); profile "s": perturbed by 1e-6, 1e-4, 1e-2 x seeded normal noise (instance i % 3), t = max(-h, 2e-3) --
    and not below z / ZT_MAX -- with z = the solve's returned lam_g / lam_x through the row table (the side of a bound the multiplier's
    sign names), and not below c / t, c = c_small ("x": the barrier parameter the solve ended with) x a seeded log-normal(0.5) ("s").
    The floors of "s" keep the barrier terms z / t below ZT_MAX: the smallest
    eigenvalue of the reduced Hessian at a solution is the objective's smallest weight, 2e-4, and an attempt is decidable only above
    1e-9 x the largest.  "x" therefore runs only under settings in which every instance ends at the KKT test.  Same dict as
    newton_step_lib.make_batch; mode 1 (exact Hessian).  heavy (profile "d"): "x" with 100 added to the multipliers of the (up to) three
    rows of every instance whose slack is smallest, capped at 0.9e-4 / t: t z and prim stay below 1e-4 while dual rises far above 1."""
    floor = 5e-7 if exact else 2e-3
    from boundplanner_amd import scenes
    b = scenes.make_batch(B, N, seed, O.fk_batch, randomize_sets=True)
    rng = np.random.default_rng(seed + 1)
    x0 = np.zeros_like(b["x0"])
    st0 = np.arange(40) * N
    S = N - 1
    T, Z, TS, ZS = (np.zeros((B, S, n)) for n in (HP.MAXROWS, HP.MAXROWS, HP.NSLOT, HP.NSLOT))
    slot = np.full((B, S, HP.MAXROWS), -1, int)
    rows_all, status = [], []
    for i in range(B):
        sol = O.solve(N, b["x0"][i], b["lbx"][i], b["ubx"][i], b["p"][i], tol=1e-8, max_iter=300)
        status.append(sol["status"])
        x0[i] = sol["x"] + (0.0 if exact else (1e-6, 1e-4, 1e-2)[i % 3]) * rng.normal(size=x0.shape[1])
        if not exact and i % 6 == 3:        # one joint's acceleration shifted at every stage: a defect of the pinned part of x_1 alone
            x0[i, 2 * 7 * N + 2 * N + np.arange(1, N)] += 0.3
        if not exact and i % 6 == 4:        # ... at the last stage alone: a defect of the dynamics
            x0[i, 2 * 7 * N + 2 * N + N - 1] += 0.3
        x0[i, st0] = b["lbx"][i, st0]
        rows = O.stage_rows(N, x0[i], b["lbx"][i], b["ubx"][i], b["p"][i])
        rows_all.append(rows)
        one = np.ones((S, HP.MAXROWS))
        h = O.newton_system(N, x0[i], b["lbx"][i], b["ubx"][i], b["p"][i], one, one, 0, 0.1, step=False)["h"]
        live = np.arange(HP.MAXROWS)[None, :] < rows[0][:, None]
        G, X, _ = L.row_table(N, rows)
        zl = np.zeros((S, HP.MAXROWS))
        zl[G[:, 0], G[:, 1]] = np.maximum(G[:, 3] * sol["lam_g"][G[:, 2]], 0.0)
        zl[X[:, 0], X[:, 1]] = np.maximum(np.where(X[:, 3] > 0, 1.0, -1.0) * sol["lam_x"][X[:, 4]], 0.0)
        T[i] = np.where(live, np.maximum(-h, floor if exact else np.maximum(floor, zl / ZT_MAX)), 0.0)
        c = c_small * (1.0 if exact else np.exp(0.5 * rng.normal(size=h.shape)))
        Z[i] = np.where(live, np.maximum(zl, c / np.where(live, T[i], 1.0)), 0.0)
        if heavy:
            flat = np.argsort(np.where(live, T[i], np.inf), axis=None, kind="stable")[:3]
            ks, rs = np.unravel_index(flat, T[i].shape)
            Z[i][ks, rs] = np.minimum(Z[i][ks, rs] + 100.0, 0.9e-4 / T[i][ks, rs])
        TS[i], ZS[i] = HP.slot_arrays(N, rows, T[i], Z[i], HP.ORACLE_Y_NAMES)
        slot[i] = slots_of(N, rows)
    return dict(x0=x0, lbx=b["lbx"], ubx=b["ubx"], p=b["p"], T=T, Z=Z, TS=TS, ZS=ZS, rows=rows_all, slot=slot, mode=np.ones(B, np.int32),
                N=N, B=B, solve_status=np.array(status))


def make_batch(N, B, seed, profile, O):
    """the profiles of newton_step_lib.make_batch; "s", "x", "d" (make_solved_batch); "b" with the
    slacks raised to T_MIN_B at the same t z (z / t <= 1e4 instead of 1e10: the attempts stay decidable); "h": profile (a) with heavy multipliers -- z x 10^(1 + i % 4)
    on the even instances i, z = 3e3 (1 + i % 4) on every box row of the odd ones, slacks as they are: zsum / nrows and the adjoint multipliers beyond 100 without a badly conditioned barrier term"""
    if profile in "sxd":
        return make_solved_batch(N, B, seed, O, profile != "s", heavy=profile == "d")
    bt = NS.make_batch(N, B, seed, "a" if profile == "h" else profile)
    if profile == "b":      # the late-iteration rows of the Newton pin with the slacks not below T_MIN_B at the same products t z
        for i in range(B):
            told = bt["T"][i].copy()
            bt["T"][i] = np.where(told > 0, np.maximum(told, T_MIN_B), told)
            bt["Z"][i] = np.where(told > 0, bt["Z"][i] * told / np.where(told > 0, bt["T"][i], 1.0), bt["Z"][i])
            bt["TS"][i], bt["ZS"][i] = HP.slot_arrays(N, bt["rows"][i], bt["T"][i], bt["Z"][i], HP.ORACLE_Y_NAMES)
    if profile == "h":
        for i in range(B):
            if i % 2:           # both sides of every box alike: the multipliers' gradients cancel, zsum is the larger share of s_d
                X = L.row_table(N, bt["rows"][i])[1]
                bt["Z"][i][X[:, 0], X[:, 1]] = 3e3 * (1 + i % 4)
            else:
                bt["Z"][i] *= 10.0 ** (1 + i % 4)
            bt["TS"][i], bt["ZS"][i] = HP.slot_arrays(N, bt["rows"][i], bt["T"][i], bt["Z"][i], HP.ORACLE_Y_NAMES)
    return bt


# ---------------------------------------------------------------- continuous quantities
def dense_Z(A, B, S):
    """Z_k [S][41][nv] in extended precision: dzeta_k = Z_k v, v = (8 free entries of dx_1, 9 controls per stage), by forward
    propagation of dx_{k+1} = A_k dx_k + B_k dw_k"""
    nv = 8 + NU * S
    Zx = np.zeros((NX, nv), LD)
    Zx[24:32, :8] = np.eye(8)
    out = []
    for k in range(S):
        Zk = np.zeros((NZ, nv), LD)
        Zk[:NX] = Zx
        Zk[NX:, 8 + NU * k:8 + NU * (k + 1)] = np.eye(NU)
        out.append(Zk)
        if k < S - 1:
            Zx = A[k] @ Zx + B[k] @ Zk[NX:]
    return out


def quantities(bt, i, out, sysd, O, gb, dt=0.1):
    """the reference's continuous quantities of instance i at the kernel's returned iterate: dict of values, of the sums of the
    absolute terms of the deciding entries ("s_" keys) and of what decided them"""
    N, S = bt["N"], bt["N"] - 1
    lbx, ubx = bt["lbx"][i], bt["ubx"][i]
    zeta = np.asarray(out["zeta0"][i], LD)
    w, y, om = L.w_of_zeta(N, zeta, lbx, O, dt)
    g = O.nlp_eval(N, w, bt["p"][i], dt, jac=False)[1]
    tables = bt.setdefault("row_tables", {})
    if i not in tables:
        tables[i] = L.row_table(N, bt["rows"][i])
    h = L.rows_h(N, tables[i], w, y, g, gb[0], gb[1], lbx, ubx)
    live = bt["slot"][i] >= 0
    t, z = np.asarray(L.gather(bt, i, out["t0"][i]), LD), np.asarray(L.gather(bt, i, out["z0"][i]), LD)
    q = {}
    # primal infeasibility: rows, defects, the pinned part of x_1
    r, r0, _ = L.defects(N, zeta, om, lbx, dt)
    A0, B0 = (np.asarray(a, LD) for a in NS.dynamics_constant_part(dt))
    sr = np.abs(zeta[:-1, :NX]) @ np.abs(A0).T + np.abs(zeta[:-1, NX:]) @ np.abs(B0).T + np.abs(zeta[1:, :NX])
    sr[:, PIR] = np.abs(zeta[:-1, PIR]) + dt * np.abs(np.asarray(om[:-1], LD)) + np.abs(zeta[1:, PIR])
    sr0 = np.abs(L.x1fix_of(N, lbx, dt)) + np.abs(zeta[0, :24])
    cand = [("row", np.where(live, np.abs(h + t), 0).ravel(), np.where(live, np.abs(h) + np.abs(t), 0).ravel()),
            ("defect", np.abs(r).ravel(), sr.ravel()), ("r0", np.abs(r0), sr0)]
    q["prim"], q["s_prim"], q["prim_by"] = max(((float(v.max()), float(s[int(np.argmax(v))]), n) for n, v, s in cand if v.size), key=lambda e: e[0])
    q["prim_parts"] = {n: float(v.max()) if v.size else 0.0 for n, v, s in cand}
    c = np.where(live, t * z, 0)
    q["cmax"], q["cmin"] = float(c.max()), float(np.where(live, c, np.inf).min())
    q["zsum"], q["nrows"] = float(np.where(live, z, 0).sum()), int(live.sum())
    # dual infeasibility and the adjoint multipliers' 1-norm, from the (held) first-order pieces
    A, B, gd = (np.asarray(sysd[k], LD) for k in ("A", "B", "gdual"))
    Zs = dense_Z(A, B, S)
    dv = sum(Zs[k].T @ gd[k] for k in range(S))
    sv = sum(np.abs(Zs[k]).T @ np.abs(gd[k]) for k in range(S))
    j = int(np.argmax(np.abs(dv)))
    q["dual"], q["s_dual"], q["dual_by"] = float(abs(dv[j])), float(sv[j]), ("x1" if j < 8 else "u")
    q["dual_x1"], q["dual_u"] = float(np.abs(dv[:8]).max()), float(np.abs(dv[8:]).max())
    M = np.eye(NX * S)
    for k in range(S - 1):
        M[NX * k:NX * (k + 1), NX * (k + 1):NX * (k + 2)] = -sysd["A"][k].T
    q["lamsum"] = float(np.abs(np.linalg.solve(M, sysd["gdual"][:, :NX].ravel())).sum())
    q["neq"] = NX * (N - 2) + 24
    q["sd"] = max(100.0, (q["lamsum"] + q["zsum"]) / (q["neq"] + q["nrows"])) / 100.0
    q["sc"] = max(100.0, q["zsum"] / q["nrows"]) / 100.0
    terms = dict(dual=(q["dual"] / q["sd"], q["s_dual"] / q["sd"]), prim=(q["prim"], q["s_prim"]), compl=(q["cmax"] / q["sc"], q["cmax"] / q["sc"]))
    q["err_by"] = max(terms, key=lambda n: terms[n][0])
    q["err"], q["s_err"] = terms[q["err_by"]]
    return q


# ---------------------------------------------------------------- first-order pieces against differences (CPU, oracle only)
def _richardson(fun, eps):
    d1 = (fun(eps) - fun(-eps)) / (2 * eps)
    d2 = (fun(eps / 2) - fun(-eps / 2)) / eps
    return (4 * d2 - d1) / 3, np.abs(d2 - d1) / 3


def _stage_into_w(N, w, k, yk, zeta_k, O, dt):
    """w with stage k + 1 (row k of zeta) replaced by the natural coordinates yk: the assignments of line_search_lib.w_of_zeta for
    one stage"""
    w = w.copy()
    S, kk = N - 1, k + 1
    yd = np.asarray(yk, float)
    for blk, name in enumerate(("q", "dq", "ddq", "u")):
        for j in range(7):
            w[blk * 7 * N + j * N + kk] = yd[L.YI[f"{name}{j}"]]
    fk = O.fk_batch(yd[None, :7], yd[None, 7:14])
    v = fk["jac"][0] @ yd[7:14]
    for c in range(3):
        w[28 * N + c * N + kk] = fk["ee_pos"][0, c]
        w[28 * N + (3 + c) * N + kk] = yd[L.YI[f"pi{c}"]] + 0.5 * dt * v[3 + c]
    for c in range(6):
        w[34 * N + c * N + kk] = v[c]
        if k == S - 1:
            w[40 * N + c] = yd[L.YI[f"d{c}"]]
    for m, name in enumerate(("rs", "drs", "ps", "dps")):
        w[(40 + m) * N + 6 + kk] = yd[L.YI[name]]
    if k == 0:
        w[40 * N + 6], w[42 * N + 6] = float(zeta_k[L.Z_RS]), float(zeta_k[L.Z_PS])
    return w


def first_order_check(bt, i, zeta0, sysd, O, gb, dt=0.1, eps=1e-3):
    """worst ratio to the tolerance of (gdual, the pi rows of A and B) of the oracle against Richardson-extrapolated central
    differences of the pinned f, rows_h and the kinematics of w_of_zeta; tolerance 10 x the difference's error estimate + 1e-9 x
    the sum of the absolute terms.  The rows' and the kinematics' parts are differenced for all stages at once (stage k's rows and
    omega_k depend on zeta_k alone -- asserted through the result), f stage by stage."""
    N, S = bt["N"], bt["N"] - 1
    lbx, ubx, p = bt["lbx"][i], bt["ubx"][i], bt["p"][i]
    z0 = np.asarray(zeta0, LD)
    T = np.asarray(HP.build_T(L.YN, dt), LD)
    tables = bt.setdefault("row_tables", {})
    if i not in tables:
        tables[i] = L.row_table(N, bt["rows"][i])
    live = bt["slot"][i] >= 0
    zmul = np.where(live, np.asarray(bt["Z"][i], LD), 0)
    w0, y0, _ = L.w_of_zeta(N, z0, lbx, O, dt)
    f0, g0 = O.nlp_eval(N, w0, p, dt, jac=False)[:2]
    hscale = max(1.0, float(np.abs(np.where(live, L.rows_h(N, tables[i], w0, y0, g0, gb[0], gb[1], lbx, ubx), 0)).max()))

    def rows_and_omega(e, j):
        zz = z0.copy(); zz[:, j] += LD(e)
        w, y, om = L.w_of_zeta(N, zz, lbx, O, dt)
        h = L.rows_h(N, tables[i], w, y, O.nlp_eval(N, w, p, dt, jac=False)[1], gb[0], gb[1], lbx, ubx)
        return np.concatenate([np.where(live, h, 0), np.asarray(om, LD)], axis=1)          # [S][216 + 3]

    def f_stage(e, k, j):
        zk = z0[k].copy(); zk[j] += LD(e)
        return O.nlp_eval(N, _stage_into_w(N, w0, k, T @ zk, zk, O, dt), p, dt, jac=False)[0]

    worst = dict(gdual=0.0, AB=0.0)
    for j in range(NZ):
        d, e = _richardson(lambda s: rows_and_omega(s, j), eps)
        dh, eh, dom, eom = d[:, :HP.MAXROWS], e[:, :HP.MAXROWS], d[:, HP.MAXROWS:], e[:, HP.MAXROWS:]
        for k in range(S):
            df, ef = _richardson(lambda s: f_stage(s, k, j), eps)
            ef = float(ef) + 4 * EPS * abs(f0) / eps
            ref = df + (zmul[k] * dh[k]).sum()
            terms = abs(df) + float((zmul[k] * np.abs(dh[k])).sum())
            est = ef + float((zmul[k] * (eh[k] + 4 * EPS * hscale / eps)).sum())
            worst["gdual"] = max(worst["gdual"], float(abs(sysd["gdual"][k, j] - ref)) / (10 * est + 1e-9 * terms + 1e-300))
            if k < S - 1:           # d(pi_k + dt omega_k - pi_{k+1}) / d zeta_k[j]
                own = 1.0 if 21 <= j < 24 else 0.0
                for a in range(3):
                    ref = (own if j == 21 + a else 0.0) + dt * dom[k, a]
                    got = sysd["A"][k][21 + a, j] if j < NX else sysd["B"][k][21 + a, j - NX]
                    tol = 10 * dt * (float(eom[k, a]) + 4 * EPS * 10.0 / eps) + 1e-9 * (abs(ref) + own)
                    worst["AB"] = max(worst["AB"], float(abs(got - ref)) / tol)
    return worst


# ---------------------------------------------------------------- the rule (docstring)
class Cmp:
    """comparisons that know whether they are decidable"""

    def __init__(self):
        self.ok, self.notes = True, []

    def le(self, a, b, tol, what=""):
        if abs(a - b) <= tol:
            self.ok = False
            self.notes.append((what, a, b, tol))
        return a <= b

    def lt(self, a, b, tol, what=""):
        self.le(a, b, tol, what)
        return a < b


def replay(q, st, mode, o, rel, pd_of, attempts=True, notes=None):
    """the iteration control on the reference's quantities q from the state st (PLANT fields) and first-attempt Hessian mode:
    dict of what the kernels must leave, the classes reached, decidable (attempts = False: up to the stall bookkeeping only).  rel: relative bound of the continuous quantities;
    pd_of(hess_mode, dw) -> (positive definite, decidable) of attempt's reduced Hessian."""
    C, cls = Cmp(), set()
    if notes is not None:
        C.notes = notes
    e_dual, e_prim, e_cmax, e_cmin, e_err = rel * q["s_dual"], rel * q["s_prim"], rel * q["cmax"], rel * q["cmin"], rel * q["s_err"]
    sd, sc, tol = q["sd"], q["sc"], o["tol"]
    dsc, csc = q["dual"] / sd, q["cmax"] / sc
    cls.add("err_" + (q["err_by"] if q["err_by"] != "prim" else "prim_" + q["prim_by"]))
    if q["err_by"] == "dual" and q["dual_by"] == "x1" and q["dual_x1"] / sd - e_dual / sd > max(q["dual_u"] / sd, q["prim"], q["cmax"] / sc):
        cls.add("err_dual_x1")          # err is the dual residual of a free entry of x_1, and no control's would give the same
    if sd > 1:
        cls.add("sd_lam" if q["lamsum"] > q["zsum"] else "sd_z")
    if sc > 1:
        cls.add("sc")
    R = dict(status=-1, mu=st["mu"], err=q["err"], e_err=e_err, mu_tol=0.0)
    small = C.le(q["err"], tol, e_err, "err <= tol")
    if small:
        tests = (("dual", C.le(q["dual"], 1.0, e_dual)), ("prim", C.le(q["prim"], 1e-4, e_prim)), ("cmax", C.le(q["cmax"], 1e-4, e_cmax)))
        bad = [n for n, ok in tests if not ok]
        if not bad:
            R["status"] = 0
            cls.add("converged_at_limit" if st["it"] >= o["max_iter"] else "converged")
            return R, cls, C.ok
        cls.add("refused_" + bad[0])
        if bad == ["dual"]:
            cls.add("refused_dual_alone")       # (nothing but dual <= 1 keeps the instance from status 0)
    if st["it"] >= o["max_iter"]:
        R["status"] = 1
        cls.add("limit")
        return R, cls, C.ok
    # barrier update
    mu = st["mu"]
    e_emu = max(e_dual / sd, e_prim, max(e_cmax, e_cmin) / sc)
    two = max(abs(q["cmax"] - mu), abs(q["cmin"] - mu)) / sc
    emu = max(dsc, q["prim"], two)
    first, ndec, mu_tol, floored_at, pow_used = True, 0, 0.0, None, False
    while mu > tol / 10.0 and C.le(emu, o["kappa_eps"] * mu, e_emu, "barrier test"):
        before = mu
        k_, t_ = o["kappa_mu"] * mu, mu ** o["theta_mu"]
        new = max(tol / 10.0, min(k_, t_))
        how = "mu_tol10" if new == tol / 10.0 and min(k_, t_) < tol / 10.0 else ("mu_kappa" if k_ <= t_ else "mu_theta")
        ftol = e_emu / o["mu_floor_k"]
        fl = emu / o["mu_floor_k"]
        if C.le(0.1, fl, ftol, "floor cap"):        # the cap: an exact constant from here on
            fl, ftol = 0.1, 0.0
        m2 = max(new, fl)
        if m2 != new:
            C.lt(new, fl, ftol, "floor")
        if m2 != new:
            # the rule: m2 >= mu_before restores mu and ends the loop.  A floor that decided the previous pass and has not moved since
            # (emu decided by a term without mu) IS mu_before on every side, and so is the cap 0.1: equal by construction then, not
            # by rounding; any other floor is compared within its bound
            if floored_at == emu or ftol == 0.0:
                broke = before <= m2
            else:
                broke = C.le(before, m2, ftol, "floor break")
            if broke:
                cls.add("mu_floor_break")
                break
        if how == "mu_theta" or pow_used:
            pow_used = True
        if m2 != new:
            how, mu_tol, floored_at = "mu_floor", ftol, emu
            if first and emu == two and abs(q["cmin"] - mu) > abs(q["cmax"] - mu) and two > max(dsc, q["prim"], max(q["cmax"] - mu, 0.0) / sc):
                cls.add("mu_cmin")
        else:
            mu_tol = POW_ULPS * EPS * m2 if pow_used else 0.0
        mu, ndec, first, last_how = m2, ndec + 1, False, how
        cls.add(how)
        emu = max(dsc, q["prim"], max(q["cmax"] - mu, 0.0) / sc)
    if ndec == 0:
        cls.add("mu_same")
    elif ndec == 1:
        cls.add("mu_one_" + last_how[3:])       # one decrease, and what set its value: mu_one_kappa / _theta / _tol10 / _floor
    else:
        cls.add("mu_multi")
    R["mu"], R["mu_tol"] = mu, mu_tol
    # stall bookkeeping (on the error just computed); gn_ok on the previous iterate's
    gn_ok = st["err_prev"] > o["inertia_err"] and st["stall"] < o["stall_n"]
    if C.lt(q["err"], 0.9 * st["err_best"], e_err, "stall"):
        R["stall"], R["improved"] = 0, True
        cls.add("stall_reset")
    else:
        R["stall"], R["improved"] = st["stall"] + 1, False
        cls.add("stall_edge" if q["err"] < st["err_best"] else "stall_count")      # (edge: an improvement, by less than a tenth)
    if not attempts:
        R.update(partial=True, it_after=st["it"] + 1)
        return R, cls, C.ok
    # factorisation attempts
    hm, dw, tries, fell, dead = int(mode != 0), 0.0, 0, False, False
    dwl = st["dw_last"]
    while True:
        pd, dec = pd_of(hm, dw)
        if not dec:
            C.ok = False
            C.notes.append(("attempt", hm, dw, 0.0))
        if pd:
            break
        if hm and gn_ok:
            hm, tries, fell = 0, tries + 1, True
            cls.add("gn_allowed")
        else:
            if hm:
                cls.add("gn_refused_err" if not st["err_prev"] > o["inertia_err"] else "gn_refused_stall")
            if dw == 0.0:
                dw = o["dw0"] if dwl == 0.0 else max(1e-20, dwl / 3.0)
            else:
                dw *= 100.0 if dwl == 0.0 else 8.0
                cls.add("dw_x100" if dwl == 0.0 else "dw_x8")
            tries += 1
            if tries > 14 or dw > 1e20:
                dead = True
                break
    if dead:
        R["status"] = 3
        cls.add("dead")
        return R, cls, C.ok
    R.update(tries=tries, delta_w=dw, dw_last=dw if dw > 0 else dwl)
    if tries == 0:
        cls.add("first_attempt")
    if tries > RIC_NATT - 1:
        cls.add("beyond_natt")
    if dw > 0:
        ntry = tries - int(fell)
        cls.add(("dw_hist_" if dwl else "dw_try_") + ("1" if ntry == 1 else "2" if ntry == 2 else "3p"))
    elif dwl:
        cls.add("dw_last_kept")
    gb, gs = st["gn_back"], st["gn_skip"]
    if fell and o["gn_backoff"] > 0:
        new = (2 * gb if 2 * gb < o["gn_backoff"] else o["gn_backoff"]) if gb else 1
        cls.add("gn_back_kept" if new == gb else f"gn_back_{gb}_{new}")
        gb = gs = new
    elif tries == 0 and mode != 0:
        if gb:
            cls.add("gn_back_reset")
        gb = 0
    R.update(gn_back=gb, gn_skip=gs)
    # after the search
    by_err = C.lt(q["err"], o["hess_switch"], e_err, "hess_switch")
    by_stall = R["stall"] >= o["stall_n"]
    want = int(by_err or by_stall)
    if want and o["gn_backoff"] > 0 and gs > 0:
        want, gs = 0, gs - 1
        cls.add("hess_held")
    elif want:
        cls.add("hess_by_err" if by_err else "hess_by_stall")
    else:
        cls.add("hess_off")
    R.update(hess_mode_after=want, gn_skip_after=gs, it_after=st["it"] + 1)
    return R, cls, C.ok


# ---------------------------------------------------------------- one instance, one case
def attempts_oracle(bt, i, out, O, mu, dt=0.1):
    """(systems of both Hessian modes, pd_of) for instance i: pd_of(hess_mode, dw) by eigvalsh of Z^T Hf Z"""
    N = bt["N"]
    t, z = L.gather(bt, i, out["t0"][i]), L.gather(bt, i, out["z0"][i])
    sys_ = {}
    T = HP.build_T(HP.ORACLE_Y_NAMES, dt)
    TT = T.T @ T
    cache = {}

    def system(hm):
        if hm not in sys_:
            sys_[hm] = O.newton_system(N, bt["x0"][i], bt["lbx"][i], bt["ubx"][i], bt["p"][i], t, z, hm, mu, 0.0, dt, step=False)
        return sys_[hm]

    def pd_of(hm, dw):
        if hm not in cache:
            sd = system(hm)
            M0 = NS.Dense(sd, NS.full_hessians(sd, 0.0, dt)).M
            H1 = np.broadcast_to(TT, sd["H"].shape).copy()
            cache[hm] = (M0, NS.Dense(sd, H1).M)
        if (hm, dw) not in cache:
            M0, M1 = cache[hm]
            ev = np.linalg.eigvalsh(M0 + dw * M1)
            cache[hm, dw] = bool(ev[0] > 0), bool(abs(ev[0]) > EIG_REL * abs(ev[-1]))
        return cache[hm, dw]

    return system, pd_of


def state_of(plant_row, mode):
    st = dict(INIT)
    if mode == 2:
        st["err_prev"] = 0.0
    for n, v in zip(PLANT, plant_row):
        if v == v:
            st[n] = type(INIT[n])(v)
    return st


def measure(bt, i, profile, out, plant_row, o, O, gb, rel, with_oracle=True):
    """every figure of the pin for instance i: the reference's quantities, the replayed rule, the kernel's agreement with both"""
    mode = int(bt["mode"][i])
    st = state_of(plant_row, mode)
    # the reference's pieces depend on the iterate alone: computed once per instance and shared by the settings and runs of a case
    key = (out["zeta0"][i].tobytes(), out["t0"][i].tobytes(), out["z0"][i].tobytes())
    cache = bt.setdefault("ref_cache", {})
    if i not in cache or cache[i][0] != key:
        system, pd_of = attempts_oracle(bt, i, out, O, st["mu"])
        cache[i] = [key, system, pd_of, None]
    _, system, pd_of, q = cache[i]
    sysd = system(int(mode != 0))
    A0, B0 = NS.dynamics_constant_part(0.1)
    keep = np.ones(NX, bool); keep[PIR] = False
    for k in range(bt["N"] - 2):
        assert np.abs(sysd["A"][k][keep] - A0[keep]).max() <= 1e-15 and np.abs(sysd["B"][k][keep] - B0[keep]).max() <= 1e-15, "oracle A, B differ from the jerk integrator outside the pi rows"
    if q is None:
        q = cache[i][3] = quantities(bt, i, out, sysd, O, gb)
    notes = []
    R, cls, decidable = replay(q, st, mode, o, rel, pd_of, profile not in NO_ATTEMPTS, notes)
    ctl = out["ctl"][i]
    g = lambda n: ctl[CTL[n]]
    m = dict(q=q, R=R, classes=cls, decidable=decidable, st=st, bad=[], notes=notes)
    bad = m["bad"]
    kstatus = int(g("status"))
    if kstatus != R["status"] and not (R.get("partial") and kstatus == 3):
        bad.append(f"status {kstatus} != {R['status']}")
    m["err"] = None
    if kstatus == -1 and R["status"] == -1:
        m["err"] = abs(g("err_prev") - q["err"]) / q["s_err"]
        if not abs(g("mu") - R["mu"]) <= R["mu_tol"]:
            bad.append(f"mu {g('mu')!r} != {R['mu']!r}")
        for n in ("stall", "it_after") if R.get("partial") else ("delta_w", "tries", "stall", "gn_back", "gn_skip", "dw_last", "it_after", "hess_mode_after", "gn_skip_after"):
            if g(n) != R[n]:
                bad.append(f"{n} {g(n)!r} != {R[n]!r}")
        want_best = g("err_prev") if R["improved"] else st["err_best"]
        if g("err_best") != want_best:
            bad.append(f"err_best {g('err_best')!r} != {want_best!r}")
        if g("state_after") != 0 or g("it") != st["it"]:
            bad.append("state / it after the iteration")
    elif kstatus >= 0 and (g("state") != ST_DONE or g("state_after") != ST_DONE or g("it_after") != st["it"]):
        bad.append("a finished instance was touched")
    if with_oracle:
        ok = O.kkt_control(bt["N"], bt["x0"][i], bt["lbx"][i], bt["ubx"][i], bt["p"][i], L.gather(bt, i, out["t0"][i]), L.gather(bt, i, out["z0"][i]),
                           st["mu"], st["it"], tol=o["tol"], max_iter=o["max_iter"], mu_floor_k=o["mu_floor_k"])
        m["o_err"] = abs(ok["err"] - q["err"]) / q["s_err"]
        m["o_parts"] = {n: abs(ok[n] - q[n]) / (q.get("s_" + n, abs(q[n])) + 1e-300) for n in ("dual", "prim", "cmax", "cmin", "zsum", "lamsum", "sd", "sc")}
        want_status = R["status"] if R["status"] != 3 else -1
        m["o_bad"] = [] if (ok["status"] == want_status and ok["nrows"] == q["nrows"] and (want_status >= 0 or abs(ok["mu_new"] - R["mu"]) <= R["mu_tol"])) else \
            [f"oracle status {ok['status']} mu_new {ok['mu_new']!r} against {want_status}, {R['mu']!r}"]
    return m


# ---------------------------------------------------------------- cases, schedules, bounds
# (N, B, profile, seed): the shapes of newton_step_lib.CASES -- N = 3 no interior stage (neq = 24 + 32), 4, 6, N = 20 with B = 67
# (three instances per wavefront of the pair kernels, a ragged last one), N = 64 (the 63 partial sums ric_load_kkt_sums stages) --
# with the profiles of the Newton pin and profile "s" (make_solved_batch)
CASES = ((3, 5, "a", 7003), (3, 5, "s", 7303), (3, 5, "x", 7303), (4, 5, "b", 7104), (4, 5, "s", 7304), (4, 5, "h", 7504), (6, 12, "b", 7106),
         (6, 12, "c", 7206), (6, 12, "s", 7306), (6, 12, "x", 7306), (20, 67, "a", 7020), (20, 12, "c", 7220), (20, 12, "h", 7520), (64, 3, "a", 7064),
         (64, 3, "s", 7364), (64, 3, "x", 7364), (64, 3, "h", 7564), (6, 6, "d", 7306))
THROUGHPUT_CASE = (6, 32, "c", 7406)      # the problems of the batch that runs bmpc_k_ric on the GPU (repeated there to fill the batch)
ALL_CASES = CASES + (THROUGHPUT_CASE,)
# the cases whose first-order pieces are held to differences (one per shape and profile family; every instance)
FD_CASES = ((3, 5, "a", 7003), (4, 5, "s", 7304), (6, 4, "c", 7206), (20, 2, "h", 7520))
nan = float("nan")


def P(**kw):
    return [kw.get(n, nan) for n in PLANT]


# planted states in the order of the instances (rotated by the case's position), per setting = the handle's (tol, max_iter)
SCHEDULE = (P(), P(mu=1e-2, err_prev=0.5), P(mu=1e-3, err_best=1e-30, stall=3, err_prev=0.5), P(mu=1e-4, err_best=1e-30, stall=7, err_prev=2.0),
            P(mu=1e-5, stall=8, err_prev=0.5), P(mu=1e-6, err_prev=5e-3), P(dw_last=1e-3, err_prev=5e-3, mu=3e-2, it=5), P(dw_last=1e-19, err_prev=5e-3),
            P(gn_back=1, gn_skip=1, err_prev=0.5), P(gn_back=2, err_prev=0.5, mu=1e-2), P(gn_skip=2, err_prev=0.5, mu=1e-3), P(mu=3e-2, it=5, dw_last=0.5, err_prev=0.5),
            P(dw_last=1e-10, err_prev=5e-3))
SETTINGS = {"default": dict(tol=1e-5, max_iter=100, sched=SCHEDULE),
            "tight": dict(tol=1e-9, max_iter=100, sched=(P(mu=1e-5), P(mu=3e-5, err_prev=0.5), P(mu=1e-7), P(mu=1e-9), P(mu=1e-10), P(mu=1e-4, err_prev=0.5))),
            "limit": dict(tol=1e-5, max_iter=4, sched=(P(it=4), P(it=3), P(it=4, mu=1e-6), P(it=5))),
            "loose": dict(tol=1e-2, max_iter=100, sched=(P(mu=1e-3), P(mu=1e-2), P(mu=1e-4))),
            "unit": dict(tol=1.0, max_iter=100, sched=(P(mu=1e-3), P(mu=1e-2, err_prev=0.5), P(mu=1e-1))),
            "loose_limit": dict(tol=1e-2, max_iter=4, sched=(P(it=4), P(it=5, mu=1e-6))),
            "tight_x": dict(tol=1e-9, max_iter=100, sched=(P(mu=9e-5), P(mu=8e-5, err_prev=0.5))),
            "stall_edge": dict(tol=1e-5, max_iter=100, sched=(P(err_best=-0.95, stall=2, err_prev=0.5), P(err_best=-0.85, stall=2, err_prev=0.5))),
            "huge": dict(tol=1e4, max_iter=100, sched=(P(), P(mu=1e-2, err_prev=0.5))),
            "dw1": dict(tol=1e-5, max_iter=100, dw0=1.0, sched=(P(err_prev=5e-3), P(err_prev=5e-3, mu=1e-2))),
            "floor": dict(tol=1e-5, max_iter=100, mu_floor_k=100.0, sched=(P(mu=1e-1), P(mu=1e-2), P(mu=1e-3), P(mu=1e-4), P(mu=1e-5), P(mu=3e-3)))}
# the settings beside "default" run at the small shapes only
def SETTINGS_OF(N, profile):
    if profile == "x":
        return ("loose", "loose_limit", "tight_x")
    if profile == "d":
        return ("huge",)
    if N > 6:
        return ("default",)
    small = ("default", "tight", "limit", "loose", "unit", "floor", "stall_edge")
    if profile == "c":
        small += ("dw1",)
    return small


def plant_for(setting, case_index, B, bt=None):
    """planted records [B][8] of a setting.  A negative err_best -c stands for (the reference's err of the instance) / c, from the
    cache an earlier setting's check of the same batch left in bt: planted relative to err, with a margin of 5 %"""
    sched = SETTINGS[setting]["sched"]
    P_ = np.array([sched[(i + 5 * case_index) % len(sched)] for i in range(B)], float)
    for i in np.nonzero(P_[:, 2] < 0)[0]:
        ref = (bt or {}).get("ref_cache", {}).get(i)
        assert ref is not None and ref[3] is not None, f"setting {setting!r} plants err_best relative to the reference's err: check_case must have run on this batch under another setting first"
        P_[i, 2] = ref[3]["err"] / -P_[i, 2]
    return P_


def opts_of(setting):
    return dict(OPTS, **{k: v for k, v in SETTINGS[setting].items() if k != "sched"})


# profiles whose factorisation attempts are not replayed: the barrier terms z / t of exact solutions reach 1e8 against a smallest
# eigenvalue of 2e-4 and less, so that every attempt is undecidable by the rule of the docstring; their instances are
# compared up to the stall bookkeeping (status, err, mu, stall, err_best)
NO_ATTEMPTS = ("x", "d")
# worst relative error of the ORACLE's own err (bmpc_oracle_kkt_control) against the reference over all cases and settings, per
# profile, relative to the sum of the absolute terms of the deciding entry, measured on the CPU and rounded up; the kernels -- emulated
# and on the GPU -- get 32 x these (two FP64 implementations of one recursion that differ in summation order and contraction)
ORACLE_WORST = {"a": 5e-16, "b": 3e-16, "c": 3e-16, "s": 2e-16, "h": 3e-15,
                "d": 1e-16, "x": EPS}     # measured 0: complementarity -- one product -- decides at the exact solutions; one rounding stands in for it
assert all(FACTOR * v <= 1e-9 for v in ORACLE_WORST.values()), "a profile cannot tell a wrong kernel from rounding"


def check_case(bt, profile, out, plant, o, O, label, with_oracle=True):
    """all assertions of one run of one case; prints the worst ratios; returns (per-instance figures, classes reached by decidable
    instances)"""
    NS.check_longdouble()
    B = bt["B"]
    gb = O.gbounds(bt["N"])
    rel = FACTOR * ORACLE_WORST[profile]
    ms = [measure(bt, i, profile, out, plant[i], o, O, gb, rel, with_oracle) for i in range(B)]
    dec = [m for m in ms if m["decidable"]]
    errs = [m["err"] for m in ms if m["err"] is not None]
    oerrs = [m["o_err"] for m in ms] if with_oracle else []
    print(f"{label}: kernel err / bound {max(errs, default=0.0) / rel:.2g} ({len(errs)} stepped); oracle err {max(oerrs, default=0.0):.2g}; "
          f"statuses {sorted(set(int(m['R']['status']) for m in ms))}; left out {B - len(dec)}", flush=True)
    assert B - len(dec) <= MAX_LEFT_OUT * B, f"{label}: {B - len(dec)} of {B} instances with an undecidable comparison"
    if with_oracle:
        assert max(oerrs) <= ORACLE_WORST[profile], f"{label}: the oracle's own err {max(oerrs):.3g} > its recorded worst {ORACLE_WORST[profile]:.3g}"
        obad = [(i, m["o_bad"]) for i, m in enumerate(ms) if m["decidable"] and m["o_bad"]]
        assert not obad, f"{label}: the oracle decides differently from the rule: {obad}"
    assert max(errs, default=0.0) <= rel, f"{label}: err {max(errs):.3g} > {rel:.3g}"
    bad = [(i, m["bad"]) for i, m in enumerate(ms) if m["decidable"] and m["bad"]]
    assert not bad, f"{label}: the control differs from the replayed rule: {bad}"
    return ms, set().union(*(m["classes"] for m in dec)) if dec else set()


# ---------------------------------------------------------------- classes
# every class the pin must reach over the cases -- which term decides err and the scalings; termination; the barrier loop; the stall
# bookkeeping and the fallback's permission; the factorisation attempts; the Hessian choice after the search:
#   err_dual (err_dual_x1: by a free entry of x_1 alone) / err_prim_row / err_prim_defect / err_prim_r0 / err_compl   the deciding term of err (prim: by a row, a defect r_k, r0)
#   sd_lam / sd_z / sc            s_d > 1 with lamsum / zsum the larger share; s_c > 1
#   converged / refused_dual_alone (err <= tol, prim and cmax <= 1e-4: dual <= 1 alone refuses) / refused_prim / refused_cmax /
#   limit / converged_at_limit
#   mu_same / mu_one_kappa / mu_one_theta (ONE decrease, by kappa_mu / by the power) / mu_kappa / mu_theta / mu_multi / mu_tol10 / mu_floor / mu_floor_break / mu_cmin
#   stall_reset / stall_count / stall_edge (0.9 err_best <= err < err_best: counts) / gn_allowed / gn_refused_err / gn_refused_stall
#   first_attempt / gn_back_0_1 / gn_back_1_2 / gn_back_kept / gn_back_reset / dw_try_1 / dw_try_2 / dw_try_3p (no history) /
#   dw_hist_1 / dw_hist_3p + dw_x8 (dw_last / 3, then x 8) / beyond_natt (more tries than k_ric_att speculates on) / dead /
#   dw_last_kept (no delta_w in the accepted attempt: dw_last stays)
#   hess_by_err / hess_by_stall / hess_held (gn_skip > 0: held off, decremented)
CLASSES = ("err_dual", "err_dual_x1", "err_prim_row", "err_prim_defect", "err_prim_r0", "err_compl", "sd_lam", "sd_z", "sc",
           "converged", "refused_dual_alone", "refused_prim", "refused_cmax", "limit", "converged_at_limit",
           "mu_same", "mu_one_kappa", "mu_one_theta", "mu_kappa", "mu_theta", "mu_multi", "mu_tol10", "mu_floor", "mu_floor_break", "mu_cmin",
           "stall_reset", "stall_count", "stall_edge", "gn_allowed", "gn_refused_err", "gn_refused_stall",
           "first_attempt", "gn_back_0_1", "gn_back_1_2", "gn_back_kept", "gn_back_reset", "dw_try_1", "dw_try_2", "dw_try_3p", "dw_hist_1",
           "dw_hist_3p", "dw_x8", "beyond_natt", "dead", "dw_last_kept", "hess_by_err", "hess_by_stall", "hess_held")
# the classes each case (index into ALL_CASES) reaches over its settings, found on the CPU and asserted by every run, emulated or HIP
CASE_CLASSES = {
    0: ('err_dual', 'err_dual_x1', 'err_prim_row', 'first_attempt', 'hess_by_stall', 'limit', 'mu_floor_break', 'mu_kappa', 'mu_one_kappa', 'mu_same', 'stall_count', 'stall_edge', 'stall_reset'),
    1: ('dw_last_kept', 'err_compl', 'err_dual', 'err_dual_x1', 'first_attempt', 'gn_back_reset', 'hess_by_err', 'hess_held', 'limit', 'mu_floor', 'mu_floor_break', 'mu_kappa', 'mu_multi', 'mu_one_kappa', 'mu_one_theta', 'mu_same', 'mu_theta', 'refused_prim', 'stall_edge', 'stall_reset'),
    2: ('converged', 'converged_at_limit', 'err_dual', 'err_dual_x1', 'mu_floor', 'mu_one_floor', 'stall_reset'),
    3: ('dw_last_kept', 'err_prim_row', 'first_attempt', 'hess_by_stall', 'limit', 'mu_floor_break', 'mu_kappa', 'mu_one_kappa', 'mu_same', 'stall_count', 'stall_edge', 'stall_reset'),
    4: ('dw_last_kept', 'err_compl', 'err_dual', 'err_prim_defect', 'first_attempt', 'gn_allowed', 'gn_back_0_1', 'gn_back_kept', 'gn_back_reset', 'hess_by_err', 'hess_held', 'limit', 'mu_floor', 'mu_floor_break', 'mu_kappa', 'mu_multi', 'mu_one_kappa', 'mu_same', 'mu_theta', 'refused_prim', 'stall_edge', 'stall_reset'),
    5: ('dw_last_kept', 'err_compl', 'err_dual', 'err_dual_x1', 'first_attempt', 'hess_by_stall', 'limit', 'mu_same', 'sc', 'sd_lam', 'sd_z', 'stall_count', 'stall_edge', 'stall_reset'),
    6: ('dw_last_kept', 'err_prim_row', 'first_attempt', 'limit', 'mu_floor_break', 'mu_kappa', 'mu_one_kappa', 'mu_same', 'stall_count', 'stall_edge', 'stall_reset'),
    7: ('dead', 'dw_hist_3p', 'dw_last_kept', 'dw_try_1', 'dw_try_2', 'dw_x8', 'err_compl', 'err_dual', 'err_dual_x1', 'first_attempt', 'gn_allowed', 'gn_back_0_1', 'gn_back_reset', 'gn_refused_err', 'gn_refused_stall', 'hess_by_stall', 'limit', 'mu_kappa', 'mu_one_kappa', 'mu_same', 'sd_lam', 'stall_count', 'stall_edge', 'stall_reset'),
    8: ('dw_last_kept', 'err_compl', 'err_dual', 'err_dual_x1', 'err_prim_defect', 'err_prim_r0', 'first_attempt', 'gn_allowed', 'gn_back_0_1', 'gn_back_reset', 'hess_by_err', 'hess_held', 'limit', 'mu_floor', 'mu_floor_break', 'mu_kappa', 'mu_multi', 'mu_one_floor', 'mu_one_kappa', 'mu_one_tol10', 'mu_same', 'mu_theta', 'mu_tol10', 'refused_prim', 'stall_count', 'stall_edge', 'stall_reset'),
    9: ('converged', 'converged_at_limit', 'err_dual', 'err_dual_x1', 'mu_floor', 'mu_one_floor', 'stall_reset'),
    10: ('dw_last_kept', 'err_dual', 'err_dual_x1', 'first_attempt', 'hess_by_stall', 'mu_same', 'stall_count', 'stall_reset'),
    11: ('dead', 'dw_last_kept', 'dw_try_3p', 'dw_x8', 'err_compl', 'err_dual', 'err_dual_x1', 'first_attempt', 'gn_allowed', 'gn_back_0_1', 'gn_back_1_2', 'gn_back_reset', 'gn_refused_err', 'gn_refused_stall', 'hess_by_stall', 'mu_same', 'sd_lam', 'stall_count', 'stall_reset'),
    12: ('dw_last_kept', 'err_compl', 'err_dual', 'err_dual_x1', 'first_attempt', 'hess_by_stall', 'mu_same', 'sc', 'sd_lam', 'sd_z', 'stall_count', 'stall_reset'),
    13: ('err_dual', 'err_dual_x1', 'first_attempt', 'mu_same', 'stall_count', 'stall_reset'),
    14: ('dead', 'dw_hist_1', 'dw_x8', 'err_compl', 'err_dual', 'first_attempt', 'gn_refused_err', 'hess_by_err', 'mu_floor', 'mu_kappa', 'mu_multi', 'mu_one_kappa', 'mu_same', 'mu_theta', 'stall_reset'),
    15: ('converged', 'converged_at_limit', 'err_compl', 'limit', 'mu_cmin', 'mu_floor', 'mu_one_floor', 'mu_same', 'refused_cmax', 'stall_reset'),
    16: ('err_compl', 'err_dual', 'err_dual_x1', 'first_attempt', 'hess_by_stall', 'mu_same', 'sc', 'sd_lam', 'stall_count', 'stall_reset'),
    17: ('err_dual', 'err_dual_x1', 'mu_same', 'refused_dual', 'refused_dual_alone', 'stall_reset'),
    18: ('beyond_natt', 'dead', 'dw_hist_3p', 'dw_last_kept', 'dw_try_1', 'dw_try_2', 'dw_try_3p', 'dw_x8', 'err_compl', 'err_dual', 'err_dual_x1', 'first_attempt', 'gn_allowed', 'gn_back_0_1', 'gn_back_1_2', 'gn_back_kept', 'gn_back_reset', 'gn_refused_err', 'gn_refused_stall', 'hess_by_stall', 'hess_held', 'limit', 'mu_floor_break', 'mu_kappa', 'mu_one_kappa', 'mu_same', 'sd_lam', 'stall_count', 'stall_edge', 'stall_reset'),
}
