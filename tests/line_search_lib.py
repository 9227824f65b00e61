"""Step-level pin: the filter line search of one interior-point iteration against an independent check -- TEST INFRASTRUCTURE.

What is checked: everything between the Newton step (pinned by newton_step_lib) and the KKT certificates -- the merit derivative D and
phi0 (ls0_instance, the tail of k_step), the trial point, the trial slacks with the slack reset, the multiplier update, f, theta and
sum log t of the trial points (bmpc_k_trial / bmpc_k_trial_spec), and the decisions of ls_decide.  Everything is computed from the
kernel's OWN returned zeta0, dzeta, t, z, c = t + dt, which keeps the Newton step out of this test.

This file holds no filter code taken from either implementation.  The acceptance rule is written from Waechter & Biegler, Math. Prog.
106 (2006), Sec. 2.3: with the trial step lengths alpha_j = ap 2^-j, a trial (theta_j, phi_j), phi = f - mu sum log t, is rejected
when theta_j > theta_max or when a filter entry (th, ph) has theta_j >= th and phi_j >= ph; otherwise, if the switching condition
theta_0 <= theta_min, D < 0, alpha_j (-D)^s_phi > delta theta_0^s_theta holds, it is accepted iff the Armijo condition phi_j <= phi_0 +
eta_phi alpha_j D holds, and if not, iff theta_j <= (1 - gamma_theta) theta_0 or phi_j <= phi_0 - gamma_phi theta_0.  After an
acceptance that was not switching + Armijo the filter gets the entry ((1 - gamma_theta) theta_0, phi_0 - gamma_phi theta_0).
gamma_theta = gamma_phi = 1e-5, eta_phi = 1e-4, s_theta = 1.1, s_phi = 2.3, delta = 1, theta_max / theta_min = 1e4 / 1e-4 x max(1,
theta_0) at iteration 0.  This project's deviations, read off the code (oracle/bmpc_solve.c, ls_decide):
  * no second-order correction and no restoration phase;
  * at most ten trials, then the tenth is kept as the iterate with alpha = 1e300 (and gets its filter entry);
  * a filter of eight entries that drops its oldest entry when a ninth arrives;
  * the Armijo test is relaxed by 1e-12 |phi_0|;
  * the filter is emptied when mu differs from the mu it was built with.

The reference of a trial point: w(zeta_j) is assembled in numpy (HP.build_T, the variable layout, the pinned stage 0 from lbx,
p = fk(q), v = J dq through oracle_lib.fk_batch); f is the pinned objective oracle_lib.nlp_eval(w); h_i comes from the pinned g and
the box bounds through the row table of bmpc_oracle_stage_rows (which g entry or variable, which sign) -- not the oracle's h; the
defects are stated in zeta coordinates with (A, B) of newton_step_lib.dynamics_constant_part and the pinned kinematics on the pi
rows; sums in np.longdouble.  ONE row kind cannot be recovered from g or the box of w: the two rows rs~_1 >= 0, ps~_1 >= 0 of stage 1
(the eliminated stage-0 slacks; the row table gives them as c0 y[i0] + c1 y[i1] with no bound of w behind them) -- they are stated
here as -zeta_1[rs~], -zeta_1[ps~] from that table and compared with bmpc_oracle_newton_system's h on the CPU with all the others.
"""
import numpy as np

import hessian_pin_lib as HP
import newton_step_lib as NS

LD = np.longdouble
EPS = float(np.finfo(float).eps)
NX, NZ = 32, 41
Z_PI, Z_RS, Z_PS, Z_D = 21, 24, 25, 26
YN = HP.ORACLE_Y_NAMES
YI = {n: i for i, n in enumerate(YN)}
GAMMA_TH = GAMMA_PHI = 1e-5
ETA_PHI, S_TH, S_PHI, DELTA = 1e-4, 1.1, 2.3, 1.0
NTRIAL, MAXF = 10, 8
LS = {n: i for i, n in enumerate(("ap", "ad", "D", "phi0", "alpha", "bt", "f0", "th0", "ls0", "nfilt"))}
LS.update(filt_th=10, filt_phi=18, theta_max=26, theta_min=27, it=28, flip=29, hess_mode=30, state=31, mu=32, filt_mu=33)


# ---------------------------------------------------------------- the full-space point of a zeta
def w_of_zeta(N, zeta, lbx, O, dt=0.1):
    """(w [n_w] in double, y [N-1][41] natural coordinates in extended precision, omega [N-1][3] = J_ang dq) of zeta [N-1][41]"""
    S = N - 1
    T = np.asarray(HP.build_T(YN, dt), LD)
    y = np.asarray(zeta, LD) @ T.T
    yd = np.asarray(y, float)
    w = np.zeros(44 * N + 6)
    st0 = np.arange(40) * N
    w[st0] = lbx[st0]                                       # stage 0: pinned by lbx == ubx
    k = np.arange(1, N)
    for blk, name in enumerate(("q", "dq", "ddq", "u")):
        for j in range(7):
            w[blk * 7 * N + j * N + k] = yd[:, YI[f"{name}{j}"]]
    q, dq = yd[:, :7], yd[:, 7:14]
    fk = O.fk_batch(q, dq)
    v = np.einsum("kaj,kj->ka", fk["jac"], dq)
    for c in range(3):
        w[28 * N + c * N + k] = fk["ee_pos"][:, c]
        w[28 * N + (3 + c) * N + k] = yd[:, YI[f"pi{c}"]] + 0.5 * dt * v[:, 3 + c]
    for c in range(6):
        w[34 * N + c * N + k] = v[:, c]
        w[40 * N + c] = yd[S - 1, YI[f"d{c}"]]            # the global slacks: a constant state, read at the terminal stage
    for m, name in enumerate(("rs", "drs", "ps", "dps")):
        w[(40 + m) * N + 6 + k] = yd[:, YI[name]]
    w[40 * N + 6], w[42 * N + 6] = float(zeta[0][Z_RS]), float(zeta[0][Z_PS])      # rs_0 = rs~_1, ps_0 = ps~_1 with drs_0 = dps_0 = 0
    return w, y, v[:, 3:]


def g_index(N, k, gidx):
    """position in g of inequality row gidx of stage k: 35 (N-1) equality rows, then 112 per stage, then the 21 terminal ones"""
    return 35 * (N - 1) + 112 * (k - 1) + gidx if gidx < 112 else 147 * (N - 1) + gidx - 112


def row_table(N, rows):
    """the row table as index arrays: rows of g (stage, row, g index, sign), bounds of w (stage, row, y index, upper?, w index), the
    two rows of stage 1 with no bound of w behind them (row, y indices, coefficients)"""
    nrows, meta, coef = rows
    G, X, Z = [], [], []
    for k in range(1, N):
        for i in range(nrows[k - 1]):
            gidx, gsign, xidx, kind, i0, i1 = (int(v) for v in meta[k - 1, i])
            if gidx >= 0:
                G.append((k - 1, i, g_index(N, k, gidx), gsign))
            elif xidx >= 0:
                X.append((k - 1, i, i0, coef[k - 1, i, 0] > 0, xidx))
            else:
                assert k == 1 and i1 >= 0
                Z.append((i, i0, i1, coef[k - 1, i, 0], coef[k - 1, i, 1]))
    return np.array(G, int).reshape(-1, 4), np.array(X, int).reshape(-1, 5), Z


def rows_h(N, table, w, y, g, lbg, ubg, lbx, ubx):
    """h [N-1][216] (extended precision; 0 beyond nrows) of the oracle's row table at the point (w, y) with the pinned g(w)"""
    G, X, Z = table
    h = np.zeros((N - 1, HP.MAXROWS), LD)
    gv, up = np.asarray(g[G[:, 2]], LD), G[:, 3] > 0
    h[G[:, 0], G[:, 1]] = np.where(up, gv - np.asarray(ubg[G[:, 2]], LD), np.asarray(lbg[G[:, 2]], LD) - gv)
    yv, up = y[X[:, 0], X[:, 2]], X[:, 3] > 0                 # a bound of w[xidx] = y[i0]
    h[X[:, 0], X[:, 1]] = np.where(up, yv - np.asarray(ubx[X[:, 4]], LD), np.asarray(lbx[X[:, 4]], LD) - yv)
    for i, i0, i1, c0, c1 in Z:                               # rs~_1, ps~_1 >= 0: no bound of w behind them (docstring)
        h[0, i] = LD(c0) * y[0, i0] + LD(c1) * y[0, i1]
    return h


def x1fix_of(N, lbx, dt):
    """the pinned part of x~_1 from the stage-0 pins: the jerk integrator's A x_0 + B0 u_0, and pi_1 = p_rot_0 + dt/2 w_0"""
    pin = lambda blk, j: LD(lbx[blk * 7 * N + j * N])
    x = np.zeros(24, LD)
    for j in range(7):
        q0, dq0, ddq0, u0 = (pin(b, j) for b in range(4))
        x[j] = q0 + dt * dq0 + LD(dt) ** 2 / 2 * ddq0 + LD(dt) ** 3 / 8 * u0
        x[7 + j] = dq0 + dt * ddq0 + LD(dt) ** 2 / 3 * u0
        x[14 + j] = ddq0 + LD(dt) / 2 * u0
    for c in range(3):
        x[Z_PI + c] = LD(lbx[28 * N + (3 + c) * N]) + LD(dt) / 2 * LD(lbx[34 * N + (3 + c) * N])
    return x


def defects(N, zeta, omega, lbx, dt):
    """(r [N-2][32], r0 [24], sum of the absolute terms of both) in zeta coordinates, extended precision"""
    A0, B0 = (np.asarray(a, LD) for a in NS.dynamics_constant_part(dt))
    z = np.asarray(zeta, LD)
    r = z[:-1, :NX] @ A0.T + z[:-1, NX:] @ B0.T - z[1:, :NX]
    sabs = np.abs(z[:-1, :NX]) @ np.abs(A0).T + np.abs(z[:-1, NX:]) @ np.abs(B0).T + np.abs(z[1:, :NX])
    pi = slice(Z_PI, Z_PI + 3)
    r[:, pi] = z[:-1, pi] + LD(dt) * np.asarray(omega[:-1], LD) - z[1:, pi]
    sabs[:, pi] = np.abs(z[:-1, pi]) + dt * np.abs(omega[:-1]) + np.abs(z[1:, pi])
    x1 = x1fix_of(N, lbx, dt)
    r0 = x1 - z[0, :24]
    return r, r0, float(sabs.sum() + np.abs(x1).sum() + np.abs(z[0, :24]).sum())


class Point:
    """the reference's pieces at one zeta: f (pinned objective), h (rows), defects"""

    def __init__(self, bt, i, zeta, O, gb, dt=0.1):
        N = bt["N"]
        lbx, ubx = bt["lbx"][i], bt["ubx"][i]
        self.w, self.y, om = w_of_zeta(N, zeta, lbx, O, dt)
        self.f, self.g, _, _ = O.nlp_eval(N, self.w, bt["p"][i], dt, jac=False)
        tables = bt.setdefault("row_tables", {})
        if i not in tables:
            tables[i] = row_table(N, bt["rows"][i])
        self.h = rows_h(N, tables[i], self.w, self.y, self.g, gb[0], gb[1], lbx, ubx)
        self.r, self.r0, self.sdef = defects(N, zeta, om, lbx, dt)
        self.thdef = float(np.abs(self.r).sum() + np.abs(self.r0).sum())


def gather(bt, i, a):
    """kernel slots [S][208] -> oracle row order [S][216] (0 beyond nrows)"""
    sl = bt["slot"][i]
    return np.where(sl >= 0, np.take_along_axis(a, np.where(sl >= 0, sl, 0), axis=1), 0.0)


def merit_at(pt, live, t):
    """(theta, sum of its absolute terms, sum log t, sum |log t|, per-stage row shares of theta) for slacks t on the live rows"""
    t = np.asarray(t, LD)
    rows = np.where(live, np.abs(pt.h + t), 0)
    th = rows.sum() + LD(pt.thdef)
    sth = float(np.where(live, np.abs(pt.h) + np.abs(t), 0).sum()) + pt.sdef
    lg = np.where(live, np.log(np.where(live, t, 1)), 0)
    return float(th), sth, float(lg.sum()), float(np.abs(lg).sum()), np.asarray(rows.sum(axis=1), float)


def reference(bt, i, out, O, gb, dt=0.1, nj=NTRIAL, R=None):
    """the first nj reference trials of instance i from the kernel's own zeta0, dzeta, t, c: dict of lists over j (R: a result to
    extend)"""
    N = bt["N"]
    live = bt["slot"][i] >= 0
    z0, dz = np.asarray(out["zeta0"][i], LD), np.asarray(out["dzeta"][i], LD)
    t = np.asarray(gather(bt, i, out["t0"][i]), LD)
    c = t + np.asarray(gather(bt, i, out["dt"][i]), LD)       # the entry returns dt = c - t: c is recovered to an ulp of max(c, t)
    ap = float(out["ls"][i, LS["ap"]])
    R = R or dict(alpha=[], f=[], th=[], sth=[], ls=[], sls=[], t1=[], st1=[], zeta=[], stage_share=[], r0_share=[])
    for j in range(len(R["alpha"]), nj):
        a = ap * 2.0 ** -j
        zj = z0 + LD(a) * dz
        pt = Point(bt, i, zj, O, gb, dt)
        tj = np.where(live, np.maximum(t + LD(a) * (c - t), -pt.h), 1)
        th, sth, ls, sls, share = merit_at(pt, live, tj)
        R["alpha"].append(a); R["f"].append(pt.f); R["th"].append(th); R["sth"].append(sth); R["ls"].append(ls); R["sls"].append(sls)
        R["t1"].append(np.asarray(tj, float)); R["zeta"].append(zj)
        R["st1"].append(np.asarray(np.maximum(np.abs(t) + a * np.abs(c - t), np.abs(pt.h)), float))
        R["stage_share"].append(share); R["r0_share"].append(float(np.abs(pt.r0).sum()))
    R["live"], R["t"], R["c"] = live, t, c
    return R


def start_merit(bt, i, out, O, gb, dt=0.1):
    """(f0, th0, ls0) of the iterate the search starts from, with its slacks as they are (no reset): the true merit pieces of the
    overwritten rows"""
    live = bt["slot"][i] >= 0
    pt = Point(bt, i, out["zeta0"][i], O, gb, dt)
    th, _, ls, _, _ = merit_at(pt, live, np.where(live, gather(bt, i, out["t0"][i]), 1))
    return pt.f, th, ls


def merit_derivative(bt, i, out, O, mu, dt=0.1):
    """(D, tolerance): Richardson-extrapolated central difference of the pinned f along w(zeta0 + eps dzeta) with its own error
    estimate, plus -mu sum dt_i / t_i over the live rows in extended precision; tolerance 10 x estimate + 1e-9 x sum |terms|"""
    N = bt["N"]
    z0, dz = np.asarray(out["zeta0"][i], LD), np.asarray(out["dzeta"][i], LD)
    eps = 2e-3 / max(1.0, float(np.abs(dz).max()))
    fv = lambda e: O.nlp_eval(N, w_of_zeta(N, z0 + LD(e) * dz, bt["lbx"][i], O, dt)[0], bt["p"][i], dt, jac=False)[0]
    d1 = (fv(eps) - fv(-eps)) / (2 * eps)
    d2 = (fv(eps / 2) - fv(-eps / 2)) / eps
    df, err = (4 * d2 - d1) / 3, abs(d2 - d1) / 3 + 4 * EPS * abs(fv(0.0)) / eps
    live = bt["slot"][i] >= 0
    t = np.asarray(gather(bt, i, out["t0"][i]), LD)
    dts = np.asarray(gather(bt, i, out["dt"][i]), LD)
    terms = np.where(live, LD(mu) * dts / np.where(live, t, 1), 0)
    return float(df - terms.sum()), 10 * err + 1e-9 * (abs(df) + float(np.abs(terms).sum()))


# ---------------------------------------------------------------- the acceptance rule (docstring)
def replay(th, phi, alpha, st, eth, ephi):
    """the search on the trials (th_j, phi_j, alpha_j) from the state st = dict(th0, phi0, D, theta_max, theta_min, filt = [(th,
    ph)]): (bt, failed, why [j] = what decided trial j, armijo_case, decidable).  eth [j], ephi [j]: bounds on the merit pieces --
    a comparison whose margin is below them makes the search undecidable."""
    th0, phi0, D = st["th0"], st["phi0"], st["D"]
    why, ok_all = [], True

    def cmp(lhs, rhs, tol):          # lhs <= rhs, and whether that is decidable
        nonlocal ok_all
        if abs(lhs - rhs) <= tol:
            ok_all = False
        return lhs <= rhs

    for j in range(NTRIAL):
        if not cmp(th[j], st["theta_max"], eth[j]):
            why.append("theta_max"); continue
        hit = False
        for fth, fph in st["filt"]:
            if cmp(fth, th[j], eth[j]) and cmp(fph, phi[j], ephi[j]):
                hit = True; break
        if hit:
            why.append("filter"); continue
        sw = th0 <= st["theta_min"] and D < 0 and alpha[j] * (-D) ** S_PHI > DELTA * th0 ** S_TH
        if sw:
            if cmp(phi[j], phi0 + ETA_PHI * alpha[j] * D + 1e-12 * abs(phi0), ephi[j]):
                why.append("armijo"); return j, False, why, True, ok_all
            why.append("switch_no_armijo"); continue
        a = cmp(th[j], (1 - GAMMA_TH) * th0, eth[j])
        b = cmp(phi[j], phi0 - GAMMA_PHI * th0, ephi[j])
        if a or b:
            why.append("both" if a and b else ("theta" if a else "phi")); return j, False, why, False, ok_all
        why.append("no_decrease")
    return NTRIAL - 1, True, why, False, ok_all


def filter_after(st, armijo_case):
    f = list(st["filt"])
    if not armijo_case:
        if len(f) == MAXF:
            f = f[1:]
        f.append(((1 - GAMMA_TH) * st["th0"], st["phi0"] - GAMMA_PHI * st["th0"]))
    return f


# ---------------------------------------------------------------- cases, classes and bounds
# (N, B, profile, seed) as newton_step_lib.CASES: N = 3 no interior stage (the k == 1 and terminal branches in the same two lanes, 32
# instances per wavefront), 4, 6, 20 with B = 67 (three instances on 57 lanes, ragged last wavefront), 30, 64 (63 lanes)
SPEC_CASE = (6, 32, "a", 7306)         # the 32 problems of the GPU half's bmpc_k_trial batch
CASES = NS.CASES + (SPEC_CASE,)
COLD_CASE = (6, 12, 7506)              # t, z == NULL: the rows and merit pieces of the init launch, nothing planted
MAX_LEFT_OUT = NS.MAX_LEFT_OUT
FACTOR = 32.0
# worst figures of the ORACLE's own trial point (bmpc_oracle_trial_point) against the reference over all cases, per profile, each
# relative to the sum of the absolute terms of the quantity (t1: |t| + alpha |dt|, or |h| where the reset acts; f: f itself, a sum
# of non-negative terms; theta: sum of |h| + |t| over the rows and of the absolute terms of every defect), measured on the CPU and
# rounded up; the kernels -- emulated and on the GPU -- get 32 x these
ORACLE_WORST = {"a": dict(t1=2.5e-14, f=1.9e-15, th=7.5e-17), "b": dict(t1=7.0e-13, f=3.4e-15, th=2.1e-16), "c": dict(t1=5.5e-15, f=1.3e-15, th=1.6e-15)}
MARGIN = 100.0                          # planted decisions keep every margin at least this many merit bounds wide
# derived bounds
ZETA_ULPS = 1.0                         # zeta1 = fma(alpha, dzeta, zeta0): one rounding of |zeta0| + alpha |dzeta|
Z1_ULPS = float(NS.OWN_ALPHA_ULPS)      # z1 = z + ad (mu - z c) rcp(t): the project's figure for its reciprocal paths, x sum |terms|


def logsum_bound(nlive, S, sls):
    """sum log t as the log of a renormalised running product: one rounding per multiply (live rows) and per stage log, one per add
    (rows + stages), relative to sum |log t_i| where the adds round, x 4"""
    return 4 * EPS * (2 * nlive + S + sls)


CLASSES = ("bt0", "bt1_3", "bt4_8", "bt9", "failed", "theta_max", "filter", "armijo", "switch_no_armijo", "theta_only", "phi_only",
           "full_filter", "mu_reset")
# what is planted per instance: (kind, J) in the order of the instances of a case, rotated by the case's position in CASES.
# "natural": the true merit pieces of the overwritten rows, nothing else -- theta_max / theta_min by the product's own rule at
# iteration 0.  Every other kind plants an iteration counter of 3 and ARTIFICIAL th0 / f0 (marked *): with the true ones the first
# trial is always accepted -- the seeded rows are far from closing their constraints (theta_0 ~ 2e3 against theta_j < 1e2 after the
# slack reset), so theta decreases at once -- and with the perturbed cold starts theta_j grows and phi_j falls monotonically with j,
# which leaves acceptance at a later trial reachable through phi (sufficient decrease or Armijo) or through a filter entry only,
# and rejection by theta_max only for all ten trials.
SCHEDULE = (("natural", 0), ("phi*", 2), ("phi*", 5), ("phi*", 9), ("failed*", 9), ("filter*", 1), ("armijo*", 0), ("armijo*", 3),
            ("theta*", 0), ("mu_reset", 0), ("filter*", 6), ("phi*", 0))
N_PLANNED = len(SCHEDULE)               # instances beyond these (B = 67) are "natural"
PLANT_IT = 3


def schedule_of(case_index, B):
    return [SCHEDULE[(i + 5 * case_index) % N_PLANNED] if i < N_PLANNED else ("natural", 0) for i in range(B)]


def merit_bounds(R, mu, profile, S):
    """bounds on a trial's theta and phi as the kernels may return them: 32 x the oracle's worst x the sums of the absolute terms"""
    W = ORACLE_WORST[profile]
    nlive = int(R["live"].sum())
    eth = [FACTOR * W["th"] * s for s in R["sth"]]
    ephi = [FACTOR * W["f"] * abs(f) + mu * logsum_bound(nlive, S, s) for f, s in zip(R["f"], R["sls"])]
    return eth, ephi


def plan(kind, J, R, mu, D, true, eth, ephi):
    """(plant0 [22], plant1 [19], state for the replay) for one instance, or None when the trials do not allow the kind with every
    margin >= MARGIN merit bounds.  true = (f0, th0, ls0) of the overwritten rows."""
    nan = np.nan
    f0, th0, ls0 = true
    th, phi, al = np.array(R["th"]), np.array(R["f"]) - mu * np.array(R["ls"]), np.array(R["alpha"])
    mth, mphi = MARGIN * max(eth), MARGIN * max(ephi)
    p0, p1 = np.full(22, nan), np.full(19, nan)
    p0[:3] = f0, th0, ls0
    if kind == "natural":
        st = dict(th0=th0, phi0=f0 - mu * ls0, D=D, theta_max=1e4 * max(1.0, th0), theta_min=1e-4 * max(1.0, th0), filt=[])
        return p0, None, st
    if kind == "mu_reset":      # a full filter that would reject everything, built with another mu: emptied by the line-search start
        p0[4], p0[5], p0[6:14], p0[14:22] = -7.0, 8, 0.0, -1e300
        st = dict(th0=th0, phi0=f0 - mu * ls0, D=D, theta_max=1e4 * max(1.0, th0), theta_min=1e-4 * max(1.0, th0), filt=[])
        return p0, None, st
    p0[3] = PLANT_IT
    filt, theta_max, theta_min = [], 1e300, 0.0
    lowest_before = lambda a: a[:J].min() if J else np.inf
    if kind == "phi*":          # no theta decrease, no switching; phi0 - gamma th0 between phi_J and the trials before it
        th0 = 0.5 * th.min()
        if not phi[J] + 2 * mphi < lowest_before(phi):
            return None
        edge = phi[J] + mphi if J == 0 else 0.5 * (phi[J] + phi[:J].min())
        phi0 = edge + GAMMA_PHI * th0
    elif kind == "theta*":      # theta decreases, phi does not
        if J != 0:
            return None
        th0, phi0 = 2.0 * th.max(), phi.min() - 1e3 * (1 + abs(phi).max())
    elif kind == "failed*":     # every trial above theta_max
        th0, phi0 = 2.0 * th.max(), phi.max() + 1.0
        theta_max = 0.5 * th.min()
    elif kind == "filter*":     # one entry rejects every trial before J; seven that reject nothing before it: a full filter
        if J == 0 or not phi[J] + 2 * mphi < phi[:J].min():
            return None
        filt = [(1e300, 1e300)] * (MAXF - 1) + [(th[:J].min() - mth, 0.5 * (phi[J] + phi[:J].min()))]
        th0, phi0 = 2.0 * th.max(), phi.min() - 1e3 * (1 + abs(phi).max())
    elif kind == "armijo*":     # switching condition true at every trial; Armijo true at J first
        if not D < 0:
            return None
        theta_min = 1e300
        th0 = (0.5 * al.min() * (-D) ** S_PHI / DELTA) ** (1 / S_TH)
        a = phi - ETA_PHI * al * D
        if not a[J] + 2 * mphi < lowest_before(a):
            return None
        phi0 = a[J] + mphi if J == 0 else 0.5 * (a[J] + a[:J].min())
    else:
        raise ValueError(kind)
    p0[0], p0[1] = phi0 + mu * ls0, th0
    phi0 = p0[0] - mu * ls0          # as the kernel forms it from what is planted
    p1[0] = len(filt)
    for j, (a, b) in enumerate(filt):
        p1[1 + j], p1[9 + j] = a, b
    p1[17], p1[18] = theta_max, theta_min
    return p0, p1, dict(th0=th0, phi0=phi0, D=D, theta_max=theta_max, theta_min=theta_min, filt=filt)


def plans_for(bt, profile, out, O, case_index, dt=0.1):
    """from a first run `out` of the entry (nothing planted): per instance the reference trials, the planted records and the state
    the replay starts from.  Returns (plant0 [B][22], plant1 [B][19], info list)."""
    N, B = bt["N"], bt["B"]
    gb = O.gbounds(N)
    sched = schedule_of(case_index, B)
    P0, P1, info = np.full((B, 22), np.nan), np.full((B, 19), np.nan), []
    for i in range(B):
        if out["state"][i, 1] != -1:            # no step: nothing to search
            info.append(None); continue
        mu, D = float(out["ls"][i, LS["mu"]]), float(out["ls"][i, LS["D"]])
        kind, J = sched[i]
        true = start_merit(bt, i, out, O, gb, dt)
        R = reference(bt, i, out, O, gb, dt, nj=NTRIAL if kind not in ("natural", "mu_reset") else 1)
        eth, ephi = merit_bounds(R, mu, profile, N - 1)
        got = plan(kind, J, R, mu, D, true, eth, ephi)
        if got is None:
            kind, got = "natural", plan("natural", 0, R, mu, D, true, eth, ephi)
        P0[i] = got[0]
        if got[1] is not None:
            P1[i] = got[1]
        info.append(dict(kind=kind, J=J, R=R, st=got[2], true=true, wanted=sched[i]))
    fell = tuple(i for i, inf in enumerate(info) if inf is not None and inf["kind"] != sched[i][0])
    assert fell == tuple(FALLBACKS.get(case_index, ())), f"case {case_index}: instances {fell} fall back to the natural search, the table says {FALLBACKS.get(case_index, ())}"
    return P0, P1, info


def oracle_figures(bt, i, out, R, O, dt=0.1):
    """worst (t1, f, theta) errors of bmpc_oracle_trial_point against the reference over the trials of R, relative to the sums of
    the absolute terms"""
    N, live = bt["N"], R["live"]
    w = dict(t1=0.0, f=0.0, th=0.0)
    for j in range(len(R["alpha"])):
        t1, f1, th1, _ = O.trial_point(N, bt["lbx"][i], bt["ubx"][i], bt["p"][i], out["zeta0"][i], out["dzeta"][i], np.asarray(R["t"], float),
                                       np.asarray(R["c"], float), R["alpha"][j], dt)
        w["t1"] = max(w["t1"], float(np.where(live, np.abs(t1 - R["t1"][j]) / np.where(live, R["st1"][j], 1), 0).max()))
        w["f"] = max(w["f"], abs(f1 - R["f"][j]) / abs(R["f"][j]))
        w["th"] = max(w["th"], abs(th1 - R["th"][j]) / R["sth"][j])
    return w


def measure(bt, i, profile, out, inf, spec, O, dt=0.1):
    """every figure of the pin for instance i: dict of ratios to the bounds ("r_" keys), decisions, classes"""
    N, S = bt["N"], bt["N"] - 1
    gb = O.gbounds(N)
    ls, R, st = out["ls"][i], inf["R"], inf["st"]
    mu, ap, ad = float(ls[LS["mu"]]), float(ls[LS["ap"]]), float(ls[LS["ad"]])
    btk, alpha = int(ls[LS["bt"]]), float(ls[LS["alpha"]])
    failed = alpha == 1e300
    if len(R["alpha"]) < btk + 1:
        reference(bt, i, out, O, gb, dt, nj=btk + 1, R=R)
    live, W = R["live"], ORACLE_WORST[profile]
    m = dict(kind=inf["kind"], bt=btk, failed=failed)
    # ---- decisions: the rule of the docstring on the reference's trials
    eth, ephi = merit_bounds(R, mu, profile, S)
    phi = [f - mu * l for f, l in zip(R["f"], R["ls"])]
    n = len(R["alpha"])
    rb, rfailed, why, armijo, decidable = replay((R["th"] + [np.inf] * (NTRIAL - n)), phi + [np.inf] * (NTRIAL - n), R["alpha"] + [0.0] * (NTRIAL - n),
                                                 dict(st, theta_max=st["theta_max"] if n == NTRIAL else min(st["theta_max"], 1e300)), eth + [0.0] * (NTRIAL - n), ephi + [0.0] * (NTRIAL - n))
    m["decidable"] = decidable
    m["decision_ok"] = (rb == btk and rfailed == failed and rb < n)
    m["why"] = why
    want_filt = filter_after(st, armijo)
    nf = int(ls[LS["nfilt"]])
    got_filt = [(ls[LS["filt_th"] + j], ls[LS["filt_phi"] + j]) for j in range(min(nf, MAXF))]
    m["filter_ok"] = nf == len(want_filt) and all(abs(a[0] - b[0]) <= 4 * EPS * abs(b[0]) + st.get("tol_th", 0.0) and abs(a[1] - b[1]) <= 4 * EPS * (abs(b[1]) + abs(st["phi0"])) + st.get("tol_phi", 0.0)
                                                    for a, b in zip(got_filt, want_filt))
    m["alpha_ok"] = failed or alpha == ap * 2.0 ** -btk
    it0 = PLANT_IT if inf["kind"] not in ("natural", "mu_reset") else 0
    m["state_ok"] = ls[LS["it"]] == it0 + 1 and ls[LS["flip"]] == 1 and ls[LS["state"]] == 0
    m["phi0"] = abs(ls[LS["phi0"]] - st["phi0"]) / (abs(st["phi0"]) + mu * abs(inf["plant_ls0"]) + 1e-300)
    # classes
    cls = {"bt0" if btk == 0 else "bt1_3" if btk <= 3 else "bt4_8" if btk <= 8 else ("failed" if failed else "bt9")}
    cls |= {w for w in why if w in ("theta_max", "filter", "switch_no_armijo")}
    if not failed:
        cls.add({"armijo": "armijo", "theta": "theta_only", "phi": "phi_only", "both": "both"}[why[-1]])
    if len(st["filt"]) == MAXF:
        cls.add("full_filter")
    if inf["kind"] == "mu_reset":
        cls.add("mu_reset")
    m["classes"] = cls
    # ---- the accepted trial point against the reference's trial btk
    j = btk
    z0, dz = np.asarray(out["zeta0"][i], LD), np.asarray(out["dzeta"][i], LD)
    m["r_zeta"] = float((np.abs(out["zeta1"][i] - R["zeta"][j]) / (ZETA_ULPS * EPS * (np.abs(z0) + R["alpha"][j] * np.abs(dz)) + 1e-300)).max())
    k1 = gather(bt, i, out["t1"][i])
    m["t1"] = float(np.where(live, np.abs(k1 - R["t1"][j]) / np.where(live, R["st1"][j], 1), 0).max())
    m["f"] = abs(ls[LS["f0"]] - R["f"][j]) / abs(R["f"][j])
    m["th"] = abs(ls[LS["th0"]] - R["th"][j]) / R["sth"][j]
    m["r_ls"] = abs(ls[LS["ls0"]] - R["ls"][j]) / logsum_bound(int(live.sum()), S, R["sls"][j])
    # multipliers, in kernel slots: z1 = z + ad (mu - z c) / t on the live slots (z > 0)
    zs, ts = np.asarray(out["z0"][i], LD), np.asarray(out["t0"][i], LD)
    on = out["z0"][i] > 0
    cs = ts + np.asarray(np.where(on, out["dt"][i], 0), LD)
    tt = np.where(on, ts, 1)
    want = zs + LD(ad) * (LD(mu) - zs * cs) / tt
    sz = np.abs(zs) + ad * (mu + np.abs(zs * cs)) / tt
    m["r_z1"] = float(np.where(on, np.abs(out["z1"][i] - want) / (Z1_ULPS * EPS * sz), 0).max())
    used = np.zeros(out["t1"][i].shape, bool)
    np.put_along_axis(used, np.where(live, bt["slot"][i], bt["slot"][i][:, :1]), True, axis=1)
    m["live_ok"] = bool(np.array_equal(used, on) and np.isfinite(out["t1"][i][used]).all() and np.isfinite(out["z1"][i][used]).all() and np.isfinite(out["zeta1"][i]).all())
    # slots no row uses stay as the entry planted them (NaN) -- bmpc_k_trial_spec copies whole candidate records when btk > 0
    m["pad_ok"] = bool(np.isnan(out["z1"][i][~used]).all() and (np.isnan(out["t1"][i][~used]).all() or (spec and btk > 0)))
    # ---- D against the extrapolated difference of the pinned f
    Dref, tol = merit_derivative(bt, i, out, O, mu, dt)
    m["r_D"] = abs(ls[LS["D"]] - Dref) / tol
    m["oracle"] = oracle_figures(bt, i, out, R, O, dt)
    # no bound loose enough to hide a dropped share of theta: the initial-state share, the smallest stage's rows
    m["share"] = min(min(R["r0_share"][jj], R["stage_share"][jj].min()) / R["sth"][jj] for jj in range(len(R["alpha"])))
    return m


def check_case(bt, profile, out, info, spec, O, label, wanted=(), cold=False):
    """all assertions of one case on a returned search; prints the worst ratios to their bounds; returns the per-instance figures"""
    NS.check_longdouble()
    B = bt["B"]
    for i, inf in enumerate(info):
        if inf is not None:
            inf["plant_ls0"] = inf["true"][2]
    ms = [measure(bt, i, profile, out, info[i], spec, O) if info[i] is not None else None for i in range(B)]
    live = [m for m in ms if m is not None]
    W = ORACLE_WORST[profile]
    wk = {f: max(m[f] for m in live) for f in ("t1", "f", "th")}
    wo = {f: max(m["oracle"][f] for m in live) for f in ("t1", "f", "th")}
    wr = {f: max(m[f] for m in live) for f in ("r_zeta", "r_z1", "r_ls", "r_D")}
    dec = [m for m in live if m["decidable"]]
    print(f"{label}: kernel / bound " + ", ".join(f"{f} {wk[f] / (FACTOR * W[f] + 1e-300):.2g}" for f in wk) + ", " + ", ".join(f"{f[2:]} {v:.2g}" for f, v in wr.items())
          + f", phi0 {max(m['phi0'] for m in live) / EPS:.2g} ulp; oracle " + ", ".join(f"{f} {wo[f]:.2g}" for f in wo)
          + f"; bt {[m['bt'] for m in live][:N_PLANNED]}; left out {B - len(dec)}", flush=True)
    assert B - len(dec) <= MAX_LEFT_OUT * B, f"{label}: {B - len(dec)} of {B} instances without a decidable search"
    for f in wk:
        assert wo[f] <= W[f], f"{label}: the oracle's own {f} {wo[f]:.3g} > its recorded worst {W[f]:.3g}"
        assert wk[f] <= FACTOR * W[f], f"{label}: {f} {wk[f]:.3g} > {FACTOR * W[f]:.3g}"
    assert FACTOR * W["th"] < min(m["share"] for m in live), f"{label}: the bound on theta would hide a dropped share of it"
    for f, v in wr.items():
        assert v <= 1.0, f"{label}: {f[2:]} misses its bound by a factor {v:.3g}"
    assert all(m["phi0"] <= 2 * EPS for m in live), f"{label}: phi0 is not f0 - mu ls0"
    for key, what in (("alpha_ok", "alpha is not ap 2^-bt"), ("state_ok", "it / flip / state after the search"), ("live_ok", "a live slot not written, or a slot written that no row uses"),
                      ("pad_ok", "a slot no row uses was written"))[:3 if cold else 4]:
        assert all(m[key] for m in live), f"{label}: {what} (instances {[i for i, m in enumerate(ms) if m and not m[key]]})"
    for key, what in (("decision_ok", "the search ends at another trial than the rule of the reference"), ("filter_ok", "the filter after the search")):
        bad = [(i, m["bt"], m["why"]) for i, m in enumerate(ms) if m and m["decidable"] and not m[key]]
        assert not bad, f"{label}: {what}: {bad}"
    have = set().union(*(m["classes"] for m in dec))
    assert set(wanted) <= have, f"{label}: classes {sorted(set(wanted) - have)} did not occur: the case tests less than it says"
    return ms


# the classes each planted kind must produce (asserted per case for the kinds its instances carry)
KIND_CLASSES = {"natural": {"bt0"}, "phi*": {"phi_only"}, "failed*": {"failed", "theta_max"}, "filter*": {"filter", "full_filter"},
                "armijo*": {"armijo"}, "theta*": {"theta_only", "bt0"}, "mu_reset": {"mu_reset", "bt0"}}
BT_CLASS = lambda J: "bt0" if J == 0 else "bt1_3" if J <= 3 else "bt4_8" if J <= 8 else "bt9"


# instances whose scheduled kind the trials do not allow with the margins (phi_j stops falling, or falls by less than 2 x MARGIN
# bounds, before the wanted trial): they run "natural".  Found on the CPU, asserted by every run.
FALLBACKS = {0: (2, 3), 1: (2,), 2: (4,), 3: (2,), 4: (6, 7), 5: (9,)}


def planted_kinds(case_index, B):
    return [("natural", 0) if i in FALLBACKS.get(case_index, ()) else kj for i, kj in enumerate(schedule_of(case_index, B))]


def wanted_classes(case_index, B):
    w = set()
    for kind, J in planted_kinds(case_index, B):
        w |= KIND_CLASSES[kind]
        if kind in ("phi*", "filter*", "armijo*"):
            w.add(BT_CLASS(J))
        if kind == "armijo*" and J > 0:
            w.add("switch_no_armijo")
    return w


assert set().union(*(wanted_classes(ci, c[1]) for ci, c in enumerate(CASES))) >= set(CLASSES), "the cases do not contain every class of search"


def check_cold(bt, out, O, label, dt=0.1):
    """the entry with t, z == NULL: slots from the kernel's own z0 > 0 (the row table's slots must be exactly those), the merit pieces
    of the init launch through phi0 and theta_max / theta_min, then the natural search; bounds of profile (a)"""
    N, B = bt["N"], bt["B"]
    gb = O.gbounds(N)
    bt = dict(bt, rows=[O.stage_rows(N, bt["x0"][i], bt["lbx"][i], bt["ubx"][i], bt["p"][i]) for i in range(B)])
    slot = np.full((B, N - 1, HP.MAXROWS), -1, int)
    for i in range(B):
        nrows, meta, coef = bt["rows"][i]
        for k in range(1, N):
            for r in range(nrows[k - 1]):
                s = HP.slot_of_row(N, k, meta[k - 1, r], YN)
                slot[i, k - 1, r] = s + (1 if 0 <= meta[k - 1, r, 2] < 28 * N and coef[k - 1, r, 0] < 0 else 0)
    bt["slot"] = slot
    info = []
    for i in range(B):
        mu, D = float(out["ls"][i, LS["mu"]]), float(out["ls"][i, LS["D"]])
        true = start_merit(bt, i, out, O, gb, dt)
        R = reference(bt, i, out, O, gb, dt, nj=1)
        eth, ephi = merit_bounds(R, mu, "a", N - 1)
        info.append(dict(kind="natural", J=0, R=R, st=plan("natural", 0, R, mu, D, true, eth, ephi)[2], true=true, wanted=("natural", 0)))
        tm = 1e4 * max(1.0, true[1])
        assert abs(out["ls"][i, LS["theta_max"]] - tm) <= FACTOR * ORACLE_WORST["a"]["th"] * 1e4 * R["sth"][0] and abs(out["ls"][i, LS["theta_min"]] - 1e-8 * tm) <= 1e-8 * tm * 1e-9, \
            f"{label}: theta_max / theta_min are not 1e4 / 1e-4 x max(1, theta of the init launch)"
        assert abs(out["ls"][i, LS["phi0"]] - (true[0] - mu * true[2])) <= FACTOR * ORACLE_WORST["a"]["f"] * abs(true[0]) + mu * logsum_bound(int(R["live"].sum()), N - 1, R["sls"][0]) * 4, \
            f"{label}: phi0 is not f - mu sum log t of the init launch's point"
        # (theta_0, phi_0 of the replay are the reference's, the kernel's own lie within the merit bounds of them: so do the filter entries)
        info[-1]["st"].update(phi0=float(out["ls"][i, LS["phi0"]]), tol_th=FACTOR * ORACLE_WORST["a"]["th"] * R["sth"][0],
                              tol_phi=FACTOR * ORACLE_WORST["a"]["f"] * abs(true[0]) + 4 * mu * logsum_bound(int(R["live"].sum()), N - 1, R["sls"][0]))
    return check_case(bt, "a", out, info, True, O, label, cold=True)
