"""Independent replay of the batched inverse-kinematics kernel's iteration -- TEST INFRASTRUCTURE ONLY.

Written from DESIGN.md section 9 and RobotModel.py:79-144, not from csrc/bmpc_ik.hpp:

  kinematics   a plain URDF chain (T = T_parent Trans(xyz) Rz(y) Ry(p) Rx(r) Rz(q)), values in np.longdouble, derivatives by the
               complex step (np.clongdouble, h = 1e-30: no subtraction, exact to the format's rounding)
  model        the 12-vector residual r = (p - pd, vec(R rd^T - I)) and its 12 x 7 Jacobian Jr, formed explicitly:
               J = r^T r, gh = Jr^T r, H = Jr^T Jr (no geometric-Jacobian identity, no Gram-matrix shortcut)
  step         (H + lambda diag H) s = -gh on the free joints by a dense solve, refined in np.longdouble; s = 0 on the fixed ones
  loop         the projected Levenberg-Marquardt loop of section 9 with the order of the contract's tests
  seeds        Halton points in exact rational arithmetic (fractions.Fraction), mapped onto the box as section 9 says
  winner       the total order (status != 0, J, seed), a NaN cost last

The same replay runs with every operation in double (`np.float64`, `np.complex128`): the difference of the two runs is the
problem's own sensitivity to rounding, recorded below as REF_GAP; the kernel -- CPU build and GPU -- gets FACTOR x that.  The
iterate q is a double vector in both runs (it is what the kernel returns): a trial point is rounded to double before it is used."""
import functools
from fractions import Fraction

import numpy as np

from boundplanner_amd import robots

LD = np.longdouble
DEPTHS = (0, 1, 2, 3, 5, 8, 20)
FACTOR = 32
UNLIMITED, LAMBDA_MAX, LAMBDA_MIN = 1e19, 1e16, 1e-10
BASES = (2, 3, 5, 7, 11, 13, 17)
DEFAULTS = dict(tol_cost=1e-20, tol_grad=1e-10, lambda0=1e-3)
H_CS = 1e-30


def check_longdouble():
    assert np.finfo(LD).eps < 2e-19, "np.longdouble is not an extended format on this machine: the reference would be no reference"


# ------------------------------------------------------------------------------------------------------------------------------
# robot tables
# ------------------------------------------------------------------------------------------------------------------------------
def _generic_table():
    """A chain with nothing special about it: every component of every offset and every fixed angle non-zero, angles over (-3, 3),
    joints 1, 3 and 6 unlimited, the others with asymmetric limits."""
    rng = np.random.default_rng(20241)
    sgn = lambda shape: rng.choice([-1.0, 1.0], shape)
    ang = lambda shape: np.round(sgn(shape) * rng.uniform(0.25, 3.0, shape), 4)
    length = lambda shape, a, b: np.round(sgn(shape) * rng.uniform(a, b, shape), 4)
    lo, hi = -np.round(rng.uniform(1.4, 2.9, 7), 4), np.round(rng.uniform(1.4, 2.9, 7), 4)
    for j in (0, 2, 5):
        lo[j], hi[j] = -robots.BIG, robots.BIG
    t = dict(name="generic", joint_xyz=length((7, 3), 0.03, 0.25).tolist(), joint_rpy=ang((7, 3)).tolist(),
             ee_xyz=length(3, 0.05, 0.2).tolist(), ee_rpy=ang(3).tolist(), link4_col_xyz=length(3, 0.05, 0.3).tolist(),
             q_lower=lo.tolist(), q_upper=hi.tolist(), dq_max=[2.0] * 7, ddq_max=5.0, u_max=35.0,
             col_joint_sizes=[0.09, 0.09, 0.06, 0.06, 0.06, 0.06, 0.075])
    for k in ("joint_xyz", "joint_rpy", "ee_xyz", "ee_rpy", "link4_col_xyz"):
        a = np.abs(np.asarray(t[k]))
        assert (a > 0.02).all() and (a < 3.0).all(), k
    assert np.abs(np.asarray(t["joint_rpy"])).max() > 2.5 and np.abs(np.asarray(t["joint_rpy"])).min() < 0.6
    return t


GENERIC = _generic_table()
TABLES = dict(iiwa14=robots.IIWA14, gen3=robots.GEN3, generic=GENERIC)


def limits(table):
    return np.array(table["q_lower"], float), np.array(table["q_upper"], float)


# ------------------------------------------------------------------------------------------------------------------------------
# kinematics and model
# ------------------------------------------------------------------------------------------------------------------------------
def _rpy(rpy, T):
    r, p, y = (T(v) for v in rpy)
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]], dtype=T)
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]], dtype=T)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]], dtype=T)
    return Rz @ Ry @ Rx


class Chain:
    """The URDF chain of a table in the real format T (np.float64 or np.longdouble) and its complex companion."""

    def __init__(self, table, T=LD):
        self.T, self.C = T, (np.complex128 if T is np.float64 else np.clongdouble)
        self.table = table
        self.xyz = [np.array(v, dtype=T) for v in table["joint_xyz"]]
        self.rot = [_rpy(v, T) for v in table["joint_rpy"]]
        self.ee_xyz, self.ee_rot = np.array(table["ee_xyz"], dtype=T), _rpy(table["ee_rpy"], T)
        self.l4c = np.array(table["link4_col_xyz"], dtype=T)

    def fk(self, q):
        """q [..., 7] real or complex -> p [..., 3], R [..., 3, 3], the six collision points [..., 6, 3], joint origins and axes."""
        q = np.asarray(q)
        dt = q.dtype if q.dtype.kind == "c" else self.T
        q = q.astype(dt)
        lead = q.shape[:-1]
        R = np.broadcast_to(np.eye(3, dtype=dt), lead + (3, 3))
        t = np.zeros(lead + (3,), dtype=dt)
        mv = lambda A, v: (A @ v.astype(dt)[..., None])[..., 0]
        org, axes = [], []
        for i in range(7):
            t = t + mv(R, self.xyz[i])
            R = R @ self.rot[i].astype(dt)
            org.append(t)
            axes.append(R[..., :, 2])
            c, s = np.cos(q[..., i]), np.sin(q[..., i])
            Rz = np.zeros(lead + (3, 3), dtype=dt)
            Rz[..., 0, 0], Rz[..., 0, 1], Rz[..., 1, 0], Rz[..., 1, 1], Rz[..., 2, 2] = c, -s, s, c, 1
            R = R @ Rz
            if i == 3:
                l4 = t + mv(R, self.l4c)
        p = t + mv(R, self.ee_xyz)
        return p, R @ self.ee_rot.astype(dt), np.stack(org[2:7] + [l4], -2), np.stack(org, -2), np.stack(axes, -2)

    def residual(self, q, pd, rd):
        p, R, *_ = self.fk(q)
        M = R @ np.asarray(rd, dtype=self.T).T.astype(R.dtype)
        return np.concatenate([p - np.asarray(pd, dtype=self.T), (M - np.eye(3, dtype=self.T)).reshape(M.shape[:-2] + (9,))], -1)

    def residual_jac(self, q, pd, rd):
        """r [12] and Jr [12, 7] at the real point q: one evaluation of the chain at q + i h e_j, j = 0..6, and at q"""
        Q = np.tile(np.asarray(q, dtype=self.T).astype(self.C), (8, 1))
        Q[np.arange(7), np.arange(7)] += 1j * self.T(H_CS)
        r8 = self.residual(Q, pd, rd)
        return r8[7].real, (r8[:7].imag / self.T(H_CS)).T

    def model(self, q, pd, rd):
        """J = r^T r, gh = Jr^T r, H = Jr^T Jr"""
        r, Jr = self.residual_jac(q, pd, rd)
        return r @ r, Jr.T @ r, Jr.T @ Jr

    def errors(self, q, pd, rd):
        """|p - pd| and the rotation angle of M = R rd^T (from |M - I|_F = 2 sqrt 2 sin(angle / 2) below 90 degrees, from the trace and
        the skew part above)"""
        T = self.T
        r = self.residual(np.asarray(q, dtype=T), pd, rd)
        M = r[3:].reshape(3, 3) + np.eye(3, dtype=T)
        tr = M[0, 0] + M[1, 1] + M[2, 2]
        if tr > 1:
            ang = 2 * np.arcsin(np.sqrt(r[3:] @ r[3:]) / (2 * np.sqrt(T(2))))
        else:
            w = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]], dtype=T)
            ang = np.arctan2(np.sqrt(w @ w) / 2, (tr - 1) / 2)
        return np.sqrt(r[:3] @ r[:3]), ang


def pose(table, q):
    """the chain's pose at q, computed in extended precision and rounded to double: (pd [3], rd [3, 3])"""
    p, R, *_ = chain_of(table["name"], LD).fk(np.asarray(q, dtype=LD))
    return p.astype(float), R.astype(float)


@functools.lru_cache(maxsize=None)
def chain_of(name, T=LD):
    return Chain(TABLES[name], T)


def solve_free(H, gh, lam, fixed, T):
    """(H + lam diag H) s = -gh on the joints that are not fixed, s = 0 on the others; dense, refined in T.  Also the condition
    number of that system."""
    s = np.zeros(7, dtype=T)
    F = np.flatnonzero(~fixed)
    if F.size == 0:
        return s, 1.0
    A = H[np.ix_(F, F)].copy()
    A[np.arange(F.size), np.arange(F.size)] += lam * np.diag(A)
    b = -gh[F]
    sc = 1.0 / float(np.abs(A).max())                    # the double solve sees entries of order 1 whatever lambda is
    A64 = (A * T(sc)).astype(float)
    x = np.linalg.solve(A64, (b * T(sc)).astype(float)).astype(T)
    if T is not np.float64:
        for _ in range(4):
            x = x + np.linalg.solve(A64, ((b - A @ x) * T(sc)).astype(float)).astype(T)
    s[F] = x
    return s, float(np.linalg.cond(A64))


# ------------------------------------------------------------------------------------------------------------------------------
# the loop
# ------------------------------------------------------------------------------------------------------------------------------
def replay(ch, pd, rd, q_start, lo, hi, opts, depth):
    """One lane to `depth` trials.  Returns a record: states[k] = the lane after k trials (q as doubles, f, lam, nu), end = (status,
    k) when the lane stops by itself after k trials (None: still running after `depth`), classes = the branches taken, each with
    the trial it was taken at, dec = the comparisons the outcome depends on as (trial count, kind, margin)."""
    T = ch.T
    o = dict(DEFAULTS)
    o.update(opts)
    rec = dict(states=[], end=None, classes=set(), dec=[])
    pd, rd = np.asarray(pd, float), np.asarray(rd, float).reshape(3, 3)
    q = np.array(q_start, float)
    fin = np.isfinite(pd).all() and np.isfinite(rd).all() and np.isfinite(q).all() and not np.isnan(lo).any() \
        and not np.isnan(hi).any() and not (lo > hi).any() and np.isfinite(o["lambda0"]) and o["lambda0"] > 0
    if not fin:
        rec["states"].append(dict(q=q, f=T(np.nan), gh=None, pg=None, lam=T(np.nan), nu=T(2)))
        rec["end"] = (3, 0)
        rec["classes"].add(("status3", 0))
        return rec
    if ((q < lo) | (q > hi)).any():
        rec["classes"].add(("entry_clamp", 0))
    q = np.minimum(np.maximum(q, lo), hi)
    loT, hiT = lo.astype(T), hi.astype(T)
    lam, nu = T(o["lambda0"]), T(2)
    tol_c, tol_g = T(o["tol_cost"]), T(o["tol_grad"])

    def state(q, f, gh, lam, nu):
        qT = q.astype(T)
        pg = np.abs(np.minimum(np.maximum(qT - 2 * gh, loT), hiT) - qT).max()
        rec["states"].append(dict(q=q.copy(), f=f, gh=gh, pg=pg, lam=lam, nu=nu))
        return pg

    f, gh, H = ch.model(q, pd, rd)
    pg = state(q, f, gh, lam, nu)
    k, prev_fixed, rejections = 0, None, 0
    while True:
        rec["dec"].append((k, "c0", abs(float(np.sqrt(f) - np.sqrt(tol_c)))))
        if f <= tol_c:
            rec["end"] = (0, k)
            rec["classes"].add(("status0_cost", k))
            return rec
        rec["dec"].append((k, "g0", abs(float(pg - tol_g))))
        if pg <= tol_g:
            rec["end"] = (0, k)
            rec["classes"].add(("status0_grad", k))
            return rec
        if k >= depth:
            return rec
        at_lo, at_hi = q <= lo, q >= hi
        fixed = (at_lo & (gh > 0)) | (at_hi & (gh < 0))
        k += 1
        for j in range(7):
            if at_lo[j] or at_hi[j]:
                rec["dec"].append((k, "g", 2 * abs(float(gh[j]))))
            else:
                rec["dec"].append((k, "q", float(min(q[j] - lo[j], hi[j] - q[j]))))
        if (fixed & at_lo & ~at_hi).any():
            rec["classes"].add(("fixed_lo", k))
        if (fixed & at_hi & ~at_lo).any():
            rec["classes"].add(("fixed_hi", k))
        if (fixed & at_lo & at_hi).any():
            rec["classes"].add(("fixed_lo_eq_hi", k))
        if prev_fixed is not None and (prev_fixed & ~fixed).any():
            rec["classes"].add(("released", k))
        prev_fixed = fixed
        qT = q.astype(T)
        s, cond = solve_free(H, gh, lam, fixed, T)
        rec["cond"] = max(rec.get("cond", 1.0), cond)
        raw = qT + s
        qt = np.minimum(np.maximum(raw, loT), hiT).astype(float)
        ds = qt.astype(T) - qT
        pred_of = lambda d: -(2 * (gh @ d) + d @ (H @ d))
        pred, pred_raw = pred_of(ds), pred_of(s)
        sq = float(np.sqrt(f))
        if (qt == q).all():
            # the step is below half an ulp of q on every joint that moves: ds = 0 and pred = 0 exactly, in any arithmetic
            free = ~fixed & (s != 0)
            sa = np.abs(s[free]).astype(float)
            rec["dec"].append((k, "rel", float(((0.25 * np.spacing(np.abs(q[free])) - sa) / sa).min()) if free.any() else 1.0))
            rec["classes"].add(("step_rounds_to_zero", k))
            fx, ghx, Hx = f, gh, H
        else:
            fx, ghx, Hx = ch.model(qt, pd, rd)
            rec["dec"].append((k, "c", abs(float(np.sqrt(fx)) - sq) / 2))
            rec["dec"].append((k, "c", abs(float(pred)) / (4 * sq)))
        if ((raw < loT) | (raw > hiT)).any():
            rec["classes"].add(("clamped", k))
            rec["clamp_pred"] = max(rec.get("clamp_pred", 0.0), abs(float(pred - pred_raw)) / (4 * sq))
        if pred > 0 and fx < f:
            rho = (f - fx) / pred
            t = 2 * rho - 1
            fac = 1 - t * t * t
            rec["classes"].add(("accept_first" if rejections == 0 else "accept_after_rejection", k))
            rec["classes"].add(("rho_above_half" if rho > 0.5 else "rho_below_half", k))
            if fac < T(1) / 3:
                fac = T(1) / 3
                rec["classes"].add(("third", k))
            lam = lam * fac
            if lam < T(LAMBDA_MIN):
                lam = T(LAMBDA_MIN)
                rec["classes"].add(("floor", k))
            nu = T(2)
            q, f, gh, H = qt, fx, ghx, Hx
            rejections = 0
        else:
            rejections += 1
            rec["classes"].add((f"rejected_{min(rejections, 3)}", k))
            lam = lam * nu
            nu = nu * 2
            rec["dec"].append((k, "lam", abs(float(lam) / LAMBDA_MAX - 1)))
            if lam > LAMBDA_MAX:
                rec["end"] = (2, k)
                rec["classes"].add(("status2", k))
        pg = state(q, f, gh, lam, nu)
        if rec["end"] is not None:
            return rec


def at_depth(rec, m):
    """(q, cost, iters, status) of a lane run with max_iter = m, from a replay at least m deep"""
    if rec["end"] is not None and rec["end"][1] <= m:
        st, k = rec["end"]
    else:
        st, k = 1, m
        rec["classes"].add(("status1", m))
    s = rec["states"][k]
    return s["q"], s["f"], k, st


# ------------------------------------------------------------------------------------------------------------------------------
# seeds and winner
# ------------------------------------------------------------------------------------------------------------------------------
def halton(s, b):
    """radical inverse of s in base b, exact"""
    h, f = Fraction(0), Fraction(1)
    while s > 0:
        f /= b
        h += f * (s % b)
        s //= b
    return h


PI_Q = Fraction("3.14159265358979323846264338327950288419716939937510582097494459")


def seed_point(s, q0, lo, hi):
    """seed s of an instance: q0 itself for s = 0; otherwise lo + h (hi - lo) on limited joints and q0 + (2 h - 1) pi on unlimited
    ones, h = point s of the Halton sequence with bases 2 .. 17; exact, then rounded to double once.  Also the scale the rounding
    of a double evaluation of the map is relative to: the largest of its terms."""
    if s == 0:
        return np.array(q0, float), np.abs(np.asarray(q0, float))
    q, scale = np.zeros(7), np.zeros(7)
    for j in range(7):
        h = halton(s, BASES[j])
        if lo[j] <= -UNLIMITED or hi[j] >= UNLIMITED:
            q[j] = float(Fraction(float(q0[j])) + (2 * h - 1) * PI_Q)
            scale[j] = max(abs(q0[j]), np.pi)
        else:
            q[j] = float(Fraction(float(lo[j])) + h * (Fraction(float(hi[j])) - Fraction(float(lo[j]))))
            scale[j] = max(abs(lo[j]), abs(hi[j]), hi[j] - lo[j])
    return q, scale


def key(status, cost, seed):
    c = float(cost)
    return (int(status != 0), np.inf if c != c else c, seed)


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
def _box_sample(rng, table, B, margin=0.1):
    lo, hi = limits(table)
    return rng.uniform(np.where(lo <= -UNLIMITED, -np.pi, lo + margin), np.where(hi >= UNLIMITED, np.pi, hi - margin), (B, 7))


def _poses(table, qs):
    t = [pose(table, q) for q in qs]
    return np.array([a[0] for a in t]), np.array([a[1] for a in t])


def _rot_about(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _case(kind, tname, pd, rd, q0, lo=None, hi=None, require=(), **opts):
    return dict(name=f"{kind}-{tname}", kind=kind, table=tname, pd=np.ascontiguousarray(pd), rd=np.ascontiguousarray(rd),
                q0=np.ascontiguousarray(q0), lo=lo, hi=hi, require=tuple(require), opts=opts)


KINDS = ("near", "far", "bound", "box", "floor", "floor6", "stall", "stationary", "nan")
STALL_TRIALS = 3        # the stall case passes 1e16 at this trial; it must be one of DEPTHS


@functools.lru_cache(maxsize=None)
def truncated_cases(tname, rep=0):
    """The truncated-solve cases of one table; every case is one call per depth.  `require`: the classes its replay must reach.
    rep > 0: the same generators on other random streams (the sample the recorded gaps were measured on)."""
    table = TABLES[tname]
    lo, hi = limits(table)
    lim = np.flatnonzero((lo > -UNLIMITED) & (hi < UNLIMITED))
    seed = {"iiwa14": 100, "gen3": 200, "generic": 300}[tname] + 1000 * rep
    cases = []

    # near: reachable targets from starts 0.3 rad off, the shipped options, the robot's own limits
    rng = np.random.default_rng(seed + 1)
    qs = _box_sample(rng, table, 24)
    pd, rd = _poses(table, qs)
    q0 = np.clip(qs + rng.normal(0.0, 0.3, qs.shape), lo, hi)
    cases.append(_case("near", tname, pd, rd, q0, require=("accept_first", "rho_above_half", "third", "status0_cost", "status1")))

    # far: reachable targets from anywhere in the box with little damping: the Gauss-Newton model is poor, trials are rejected
    rng = np.random.default_rng(seed + 2)
    qs = _box_sample(rng, table, 37)
    pd, rd = _poses(table, qs)
    cases.append(_case("far", tname, pd, rd, _box_sample(rng, table, 37, 0.0), lambda0=1e-4,
                       require=("rejected_1", "rejected_3", "accept_after_rejection", "rho_below_half", "rho_above_half", "status1")))

    # bound: targets whose pose needs a limited joint 0.2 rad beyond a limit, from starts with that joint ON the limit and two more
    # joints on limits of their own (the robot's limits through None): joints fixed at either side, released, trials clamped
    rng = np.random.default_rng(seed + 3)
    qs = _box_sample(rng, table, 32)
    q0 = np.clip(qs + rng.normal(0.0, 0.2, qs.shape), lo, hi)
    for b in range(32):
        js = rng.choice(lim, 3, replace=False)
        side = rng.random(3) < 0.5
        qs[b, js[0]] = lo[js[0]] - 0.2 if side[0] else hi[js[0]] + 0.2
        for j, sd in zip(js, side):
            q0[b, j] = lo[j] if sd else hi[j]
        if b < 8:                                   # ... and one of them beyond its limit: the clamp on entry puts it there
            q0[b, js[1]] += -0.3 if side[1] else 0.3
    pd, rd = _poses(table, qs)
    cases.append(_case("bound", tname, pd, rd, q0, tol_grad=1e-7,
                       require=("entry_clamp", "fixed_lo", "fixed_hi", "released", "clamped", "status0_grad")))

    # box: per-instance boxes around the start, narrower than the first steps, one joint with lo == hi; targets outside the box
    rng = np.random.default_rng(seed + 4)
    q0 = _box_sample(rng, table, 29, 0.5)
    w_lo, w_hi = rng.uniform(0.02, 0.4, q0.shape), rng.uniform(0.02, 0.4, q0.shape)
    blo, bhi = q0 - w_lo, q0 + w_hi
    for b in range(29):
        j = rng.integers(7)
        blo[b, j] = bhi[b, j] = q0[b, j]
    pd, rd = _poses(table, q0 + rng.normal(0.0, 0.5, q0.shape))
    q0[:6] += rng.choice([-1.0, 1.0], (6, 7)) * rng.uniform(0.0, 0.8, (6, 7))      # six starts outside their boxes
    cases.append(_case("box", tname, pd, rd, q0, blo, bhi, tol_grad=1e-5, lambda0=1e-4,
                       require=("entry_clamp", "clamped", "clamp_pred", "fixed_lo_eq_hi", "fixed_lo", "fixed_hi", "status0_grad")))

    # floor: the damping starts at its floor; non-default tolerances
    rng = np.random.default_rng(seed + 5)
    qs = _box_sample(rng, table, 16)
    pd, rd = _poses(table, qs)
    q0 = np.clip(qs + rng.normal(0.0, 0.15, qs.shape), lo, hi)
    cases.append(_case("floor", tname, pd, rd, q0, lambda0=1e-10, tol_cost=1e-15, tol_grad=1e-11,
                       require=("floor", "third", "status0_cost")))

    # floor6: the VALUE of the floor.  One joint has lo == hi, the target keeps it there, so the six free joints face a square,
    # well-conditioned system and the replay's own gap is at rounding level; lambda0 = 1e-10 and every accepted trial multiplies by
    # 1/3, so every trial after the first runs at the floor.  Another floor changes those steps by |floor - 1e-10| |s|, far above
    # the gap
    rng = np.random.default_rng(seed + 9)
    qs = _box_sample(rng, table, 96, 0.3)
    q0 = np.clip(qs + rng.normal(0.0, 0.3, qs.shape), lo, hi)
    blo, bhi = np.tile(lo, (96, 1)), np.tile(hi, (96, 1))
    for b in range(96):
        j = rng.integers(7)
        blo[b, j] = bhi[b, j] = q0[b, j] = qs[b, j]
    pd, rd = _poses(table, qs)
    o6 = dict(lambda0=1e-10)
    # of 96 candidates the first 19 whose systems stay below a condition number of 3000 along the replay (the six-joint chain has
    # singular configurations of its own)
    keep = [b for b in range(96) if replay(chain_of(tname), pd[b], rd[b], q0[b], blo[b], bhi[b], o6, DEPTHS[-1]).get("cond", 1e9) <= 3000.0][:19]
    assert len(keep) >= 6, (tname, rep, len(keep))
    pd, rd, q0, blo, bhi = pd[keep], rd[keep], q0[keep], blo[keep], bhi[keep]
    cases.append(_case("floor6", tname, pd, rd, q0, blo, bhi, lambda0=1e-10, require=("floor", "fixed_lo_eq_hi", "status0_cost")))

    # stall: unreachable targets, the start a stretched-out configuration near a stationary point (the replay's own iterate after 40
    # trials), damping so large that q + s rounds to q: ds = 0 exactly, pred = 0, the trial is rejected whatever the arithmetic,
    # and the ladder lambda0 * 2 * 4 * 8 = 1.28e16 passes 1e16 at the third rejection, a depth the cases run (status 2 at max_iter = 3,
    # where a lane that checked max_iter first would report 1).  Of 32 candidates the first 8 whose steps
    # are below a quarter ulp of q (by the replay) are kept
    rng = np.random.default_rng(seed + 6)
    u = rng.normal(size=(32, 3))
    pd = 3.0 * u / np.linalg.norm(u, axis=1, keepdims=True)
    rd = np.array([_rot_about(rng.normal(size=3), rng.uniform(0.0, 3.0)) for _ in range(32)])
    q0 = _box_sample(rng, table, 32, 0.3)
    ch = chain_of(tname)
    q0 = np.array([replay(ch, pd[b], rd[b], q0[b], lo, hi, {}, 40)["states"][-1]["q"] for b in range(32)])
    def exact(b):
        r = replay(ch, pd[b], rd[b], q0[b], lo, hi, dict(lambda0=2e14), 3)
        rel = [m for _, kind, m in r["dec"] if kind == "rel"]
        return r["end"] == (2, STALL_TRIALS) and len(rel) == STALL_TRIALS and min(rel) > 1e-6
    keep = [b for b in range(32) if exact(b)][:8]
    assert len(keep) >= 3, (tname, rep, keep)
    cases.append(_case("stall", tname, pd[keep], rd[keep], q0[keep], lambda0=2e14,
                       require=("rejected_1", "rejected_3", "status2", "status1", "step_rounds_to_zero")))

    # stationary: the start reaches the position, the target rotation is the start's turned by 180 degrees: M is symmetric, w = 0,
    # gh = 0 and the projected gradient passes although J = 8
    rng = np.random.default_rng(seed + 7)
    q0 = _box_sample(rng, table, 4)
    pd, rd = _poses(table, q0)
    rd = np.array([_rot_about(rng.normal(size=3), np.pi) @ R for R in rd])
    cases.append(_case("stationary", tname, pd, rd, q0, require=("status0_grad",)))

    # nan: non-finite inputs and an empty box, with one sound instance among them
    rng = np.random.default_rng(seed + 8)
    qs = _box_sample(rng, table, 5)
    pd, rd = _poses(table, qs)
    q0 = np.clip(qs + rng.normal(0.0, 0.2, qs.shape), lo, hi)
    blo, bhi = np.tile(np.maximum(lo, -4.0), (5, 1)), np.tile(np.minimum(hi, 4.0), (5, 1))
    pd[0, 1], rd[1, 2, 0], q0[2, 4] = np.nan, np.nan, np.nan
    blo[3, 2], bhi[3, 2] = 0.5, 0.25
    cases.append(_case("nan", tname, pd, rd, q0, blo, bhi, require=("status3", "accept_first")))
    assert tuple(c["kind"] for c in cases) == KINDS
    for c in cases:
        c["rep"] = rep
    return cases


_REPLAYS = {}


def replays(case, T=LD):
    """the replay of every instance of a truncated case to the deepest cut-off, computed once"""
    k = (case["name"], case.get("rep", 0), T)
    if k not in _REPLAYS:
        ch = chain_of(case["table"], T)
        lo, hi = limits(TABLES[case["table"]])
        B = case["pd"].shape[0]
        _REPLAYS[k] = [replay(ch, case["pd"][b], case["rd"][b], case["q0"][b], lo if case["lo"] is None else case["lo"][b],
                              hi if case["hi"] is None else case["hi"][b], case["opts"], DEPTHS[-1]) for b in range(B)]
    return _REPLAYS[k]


def outputs(ch, rec, m, pd, rd):
    """what a lane run with max_iter = m returns, in the chain's format"""
    q, f, it, st = at_depth(rec, m)
    if st == 3:
        return dict(q=q, rcost=np.nan, pos_err=np.nan, rot_err=np.nan, iters=it, status=st)
    pe, re = ch.errors(q, pd, rd)
    return dict(q=q, rcost=np.sqrt(f), pos_err=pe, rot_err=re, iters=it, status=st)


# ------------------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------------------
FLOATS = ("q", "rcost", "pos_err", "rot_err")      # rcost = sqrt(cost) = |r|: J = |r|^2, so the rounding error of |r| is absolute
DECS = ("q", "rcost", "grad")


def bucket(k):
    return next((d for d in DEPTHS if d >= k), DEPTHS[-1])


def _absmax(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD))))


def lane_gaps(rec, recd):
    """|double replay - extended replay| of the quantities the loop compares, per state of one lane, for as long as the two runs
    take the same path: list of dict(q, rcost, grad); grad covers the entries of grad J = 2 gh and the projected gradient"""
    g = []
    for k, (s, sd) in enumerate(zip(rec["states"], recd["states"])):
        if s["gh"] is None or sd["gh"] is None or abs(float(sd["lam"] / s["lam"]) - 1) > 1e-3:
            break
        g.append(dict(q=_absmax(s["q"], sd["q"]), rcost=_absmax(np.sqrt(s["f"]), np.sqrt(sd["f"])),
                      grad=max(2 * _absmax(s["gh"], sd["gh"]), _absmax(s["pg"], sd["pg"]))))
    return g


def measure_gaps(cases, lanes=None, depths=DEPTHS):
    """Worst difference between the replay in double and the one in extended precision over `cases`: out[f][depth] for the outputs
    of a call cut off at that depth, floor[f] for the quantities the loop compares at the start (no trial yet: the rounding of one
    evaluation), and the number of lanes whose integers differ between the two runs (left out from that depth on).
    lanes: function case -> (extended records, double records, pd, rd) for cases that are not truncated-solve cases."""
    out = {f: dict.fromkeys(depths, 0.0) for f in FLOATS}
    floor = dict.fromkeys(DECS, 0.0)
    differ = 0
    for case in cases:
        ch, chd = chain_of(case["table"]), chain_of(case["table"], np.float64)
        rl, rdb, pds, rds = lanes(case) if lanes else (replays(case), replays(case, np.float64), case["pd"], case["rd"])
        for b in range(len(rl)):
            same = True
            for m in depths:
                o, od = outputs(ch, rl[b], m, pds[b], rds[b]), outputs(chd, rdb[b], m, pds[b], rds[b])
                if (o["iters"], o["status"]) != (od["iters"], od["status"]):
                    differ += same
                    same = False
                if not same or o["status"] == 3:
                    continue
                for f in FLOATS:
                    out[f][m] = max(out[f][m], _absmax(o[f], od[f]))
            for f, v in (lane_gaps(rl[b], rdb[b]) or [{}])[0].items():
                floor[f] = max(floor[f], v)
    return out, floor, differ


def _round_up(x):
    """to two significant digits, upwards; an exact 0 stays 0"""
    if x == 0.0:
        return 0.0
    e = int(np.floor(np.log10(x))) - 1
    return float(f"{np.ceil(x / 10.0 ** e) * 10.0 ** e:.1e}")


# Worst |double replay - extended replay| per case kind, output and depth, over the three tables and sixteen random streams of each
# generator (rep = 0 .. 15: the amplification of a rounding error along a lane is heavy-tailed -- one lane in a hundred is 100 x its
# neighbours -- so the sample is sixteen times what the tests run), rounded up: `PYTHONPATH=. python tests/ik_pin_lib.py` prints these tables.
# The kernel gets FACTOR x these.  "seeds": the lanes of the winner cases, which start at Halton points.
REF_GAP = \
{'near': {'q': {0: 0.0, 1: 3.4e-13, 2: 4.7e-12, 3: 4.7e-12, 5: 9.1e-12, 8: 9.3e-12, 20: 1.3e-10},
          'rcost': {0: 7.6e-16, 1: 4.5e-13, 2: 4.1e-12, 3: 4.1e-12, 5: 9e-12, 8: 4.1e-13, 20: 2.1e-13},
          'pos_err': {0: 3.8e-16, 1: 1.6e-13, 2: 1.6e-13, 3: 2.5e-13, 5: 2.7e-12, 8: 1.8e-13, 20: 2.1e-13},
          'rot_err': {0: 9.5e-16, 1: 3.2e-13, 2: 3.6e-12, 3: 3.6e-12, 5: 6.8e-12, 8: 3.6e-13, 20: 1.2e-13}},
 'far': {'q': {0: 0.0, 1: 1.6e-11, 2: 1.2e-10, 3: 1.5e-10, 5: 1.2e-09, 8: 3.8e-09, 20: 1.6e-07},
         'rcost': {0: 9.9e-16, 1: 7.8e-12, 2: 1.1e-10, 3: 1.6e-10, 5: 4.5e-10, 8: 9.9e-10, 20: 2.1e-07},
         'pos_err': {0: 5.1e-16, 1: 5e-12, 2: 1.4e-11, 3: 2.7e-11, 5: 8.7e-11, 8: 6.3e-10, 20: 1.4e-08},
         'rot_err': {0: 8.8e-16, 1: 1.3e-11, 2: 1.4e-10, 3: 1.4e-10, 5: 4.2e-10, 8: 7.2e-10, 20: 2e-07}},
 'bound': {'q': {0: 0.0, 1: 9.1e-13, 2: 7.4e-12, 3: 1.2e-11, 5: 3e-11, 8: 1.2e-10, 20: 8.4e-10},
           'rcost': {0: 1.1e-15, 1: 5.8e-13, 2: 1.6e-12, 3: 5.8e-12, 5: 1.4e-11, 8: 5.8e-11, 20: 3.7e-11},
           'pos_err': {0: 3.5e-16, 1: 3.5e-13, 2: 4.9e-13, 3: 9.2e-13, 5: 2.6e-12, 8: 5.4e-12, 20: 5.3e-11},
           'rot_err': {0: 6.8e-16, 1: 4.6e-13, 2: 3.6e-12, 3: 5.2e-12, 5: 1.2e-11, 8: 4.5e-11, 20: 1.6e-10}},
 'box': {'q': {0: 0.0, 1: 8.2e-12, 2: 5.1e-12, 3: 1.9e-12, 5: 1.2e-12, 8: 3.4e-12, 20: 3.6e-12},
         'rcost': {0: 8.4e-16, 1: 2.1e-12, 2: 3.8e-12, 3: 1.1e-12, 5: 7.8e-13, 8: 4e-13, 20: 2e-15},
         'pos_err': {0: 3.7e-16, 1: 1.5e-12, 2: 1.3e-12, 3: 3e-13, 5: 2.4e-13, 8: 1.2e-12, 20: 6.8e-14},
         'rot_err': {0: 9.2e-16, 1: 5.8e-12, 2: 3e-12, 3: 8.9e-13, 5: 5.7e-13, 8: 3.2e-12, 20: 4.6e-14}},
 'floor': {'q': {0: 0.0, 1: 5.6e-06, 2: 5.6e-06, 3: 5.6e-06, 5: 5.6e-06, 8: 8.7e-06, 20: 1.3e-05},
           'rcost': {0: 4.7e-16, 1: 2.5e-06, 2: 1.3e-06, 3: 1.3e-06, 5: 1.3e-06, 8: 1e-06, 20: 6e-09},
           'pos_err': {0: 2.6e-16, 1: 5e-07, 2: 4e-07, 3: 4e-07, 5: 4e-07, 8: 4.3e-07, 20: 8.3e-09},
           'rot_err': {0: 4e-16, 1: 1.8e-06, 2: 8.6e-07, 3: 8.6e-07, 5: 8.6e-07, 8: 6.9e-07, 20: 1.2e-08}},
 'floor6': {'q': {0: 0.0, 1: 1.7e-13, 2: 4.8e-13, 3: 1.7e-13, 5: 1.7e-13, 8: 3.1e-13, 20: 6e-12},
            'rcost': {0: 6.4e-16, 1: 1.8e-13, 2: 4.9e-13, 3: 1.4e-13, 5: 1.2e-13, 8: 4.1e-13, 20: 2.6e-13},
            'pos_err': {0: 3.1e-16, 1: 7.7e-14, 2: 1.1e-13, 3: 5.2e-14, 5: 2.9e-14, 8: 1.5e-13, 20: 2.9e-13},
            'rot_err': {0: 5.9e-16, 1: 1.2e-13, 2: 3.5e-13, 3: 9.1e-14, 5: 9.1e-14, 8: 3.2e-13, 20: 3.1e-14}},
 'stall': {'q': {0: 0.0, 1: 0.0, 2: 0.0, 3: 0.0, 5: 0.0, 8: 0.0, 20: 0.0},
           'rcost': {0: 6.3e-16, 1: 6.3e-16, 2: 6.3e-16, 3: 6.3e-16, 5: 6.3e-16, 8: 6.3e-16, 20: 6.3e-16},
           'pos_err': {0: 6.8e-16, 1: 6.8e-16, 2: 6.8e-16, 3: 6.8e-16, 5: 6.8e-16, 8: 6.8e-16, 20: 6.8e-16},
           'rot_err': {0: 4.1e-16, 1: 4.1e-16, 2: 4.1e-16, 3: 4.1e-16, 5: 4.1e-16, 8: 4.1e-16, 20: 4.1e-16}},
 'stationary': {'q': {0: 0.0, 1: 0.0, 2: 0.0, 3: 0.0, 5: 0.0, 8: 0.0, 20: 0.0},
                'rcost': {0: 8.8e-16, 1: 8.8e-16, 2: 8.8e-16, 3: 8.8e-16, 5: 8.8e-16, 8: 8.8e-16, 20: 8.8e-16},
                'pos_err': {0: 2.3e-16, 1: 2.3e-16, 2: 2.3e-16, 3: 2.3e-16, 5: 2.3e-16, 8: 2.3e-16, 20: 2.3e-16},
                'rot_err': {0: 4.5e-16, 1: 4.5e-16, 2: 4.5e-16, 3: 4.5e-16, 5: 4.5e-16, 8: 4.5e-16, 20: 4.5e-16}},
 'nan': {'q': {0: 0.0, 1: 9.5e-14, 2: 1.9e-13, 3: 2.6e-13, 5: 2.8e-13, 8: 2.8e-13, 20: 2.8e-13},
         'rcost': {0: 4.7e-16, 1: 4.8e-14, 2: 2.3e-14, 3: 4.2e-14, 5: 3.5e-15, 8: 2.6e-16, 20: 2.6e-16},
         'pos_err': {0: 2e-16, 1: 1.5e-14, 2: 6.6e-15, 3: 1.2e-14, 5: 1.9e-15, 8: 3.1e-16, 20: 3.1e-16},
         'rot_err': {0: 2.9e-16, 1: 3.4e-14, 2: 1.6e-14, 3: 3.1e-14, 5: 2.2e-15, 8: 3.4e-16, 20: 3.4e-16}},
 'seeds': {'q': {5: 3.9e-11}, 'rcost': {5: 5.3e-12}, 'pos_err': {5: 2.5e-12}, 'rot_err': {5: 5.3e-12}}}
# the same difference for the quantities the loop compares, at the start of a lane (one evaluation, no trial): worst over all kinds
DEC_FLOOR = {'q': 2.3e-16, 'rcost': 1.1e-15, 'grad': 3.9e-15}


RESIDUAL_LEVEL = ("rcost", "pos_err", "rot_err")


def bound(kind, f, m):
    """FACTOR x the recorded gap of output f at depth m.  rcost, pos_err and rot_err are norms of (parts of) one residual vector
    behind one Jacobian: they share the largest of their three gaps, which triples the sample of a heavy-tailed figure.  With each
    output's own gap one lane of 516 (bound, Gen3, depth 8) misses in pos_err by 1.2 x on the CPU build while its q, from which
    pos_err follows, is at 0.19 of its bound."""
    g = REF_GAP[kind]
    return FACTOR * (max(g[r][m] for r in RESIDUAL_LEVEL) if f in RESIDUAL_LEVEL else g[f][m])


# the comparisons a replay records in rec["dec"] as (trial count, code, margin): code -> (what is compared, the gap it goes against)
COMPARISONS = {
    "c0": ("J <= tol_cost on the state after k trials, as |sqrt f - sqrt tol_cost|", "rcost at state k"),
    "g0": ("projected gradient <= tol_grad on the state after k trials", "grad at state k"),
    "c": ("acceptance of trial k: fx < f as |sqrt fx - sqrt f| / 2, pred > 0 as pred / (4 sqrt f)", "rcost at states k - 1 and k"),
    "g": ("sign of grad J_j = 2 gh_j of a joint at a bound, before trial k", "grad at states k - 1 and k"),
    "q": ("distance of a free joint to its nearer bound, before trial k", "q at states k - 1 and k"),
    "lam": ("lambda > 1e16 after the rejection of trial k, as |lambda / 1e16 - 1|", "1e-6, relative"),
    "rel": ("trial k rounds to q: (ulp(q_j) / 4 - |s_j|) / |s_j|, smallest over the moving joints", "1e-6, relative"),
}
RELATIVE = 1e-6         # lambda and s carry the conditioning of H + lambda D: below 1e10 roundings


def undecidable_from(rec, recd):
    """First trial count from which the lane's outcome hangs on a comparison whose margin in the extended replay `rec` is below
    FACTOR x the gap of the compared quantity (None: never).  That gap is the lane's own: |double replay - extended replay| of the
    quantity at the states the comparison reads (lane_gaps), at least DEC_FLOOR -- what a lane's rounding error is amplified by
    differs by orders of magnitude from lane to lane and from trial to trial, and drops again as the lane converges.  Costs are
    compared as residual norms (fx < f, J <= tol_cost); the decrease the model predicts is a difference of two squared norms about
    sqrt f apart, so pred / (4 sqrt f) goes against the same gap; the projected gradient against tol_grad and the sign of a
    gradient entry at a bound against the gap of the gradient; the distance of a free joint to its bound against the gap of q;
    lambda against 1e16 and a step against a quarter ulp of q, both relative, against 1e-6 (lambda and s carry the conditioning of
    H + lambda D, below 1e10 roundings).  A lane whose two replays part ways is undecidable from there."""
    if rec["end"] == recd["end"] == (3, 0):
        return None
    g = lane_gaps(rec, recd)
    n = len(rec["states"])
    first = None if len(g) == n == len(recd["states"]) and rec["end"] == recd["end"] else max(len(g) - 1, 0)
    for k, kind_c, margin in rec["dec"]:
        assert kind_c in COMPARISONS
        if kind_c in ("lam", "rel"):
            thr = RELATIVE
        else:
            f = dict(c="rcost", g="grad", q="q")[kind_c[0]]       # c0, g0: the tests on the state after k trials read that state alone
            thr = FACTOR * max([DEC_FLOOR[f]] + [g[i][f] for i in ((k,) if kind_c[1:] else (k - 1, k)) if 0 <= i < len(g)])
        if margin <= thr and (first is None or k < first):
            first = k
    return first


# ------------------------------------------------------------------------------------------------------------------------------
# checks
# ------------------------------------------------------------------------------------------------------------------------------
def _kernel_floats(out, b):
    return dict(q=out["q"][b], rcost=np.sqrt(out["cost"][b]), pos_err=out["pos_err"][b], rot_err=out["rot_err"][b])


def _compare(kind, m, o, out, b, worst, fails, label):
    """one instance of one call against what the reference returns for it; worst[f] = [error, bound] at the worst ratio"""
    got = (int(out["iters"][b]), int(out["status"][b]))
    if got != (o["iters"], o["status"]):
        fails.append(f"{label} b={b} depth {m}: (iters, status) = {got}, reference {(o['iters'], o['status'])}")
        return
    if o["status"] == 3:
        if not (np.isnan(out["cost"][b]) and np.array_equal(out["q"][b], o["q"], equal_nan=True)):
            fails.append(f"{label} b={b} depth {m}: status 3 must leave q as it came and return a NaN cost")
        return
    kf = _kernel_floats(out, b)
    for f in FLOATS:
        e, bd = _absmax(o[f], kf[f]), bound(kind, f, m)
        if not e <= bd:
            fails.append(f"{label} b={b} depth {m}: {f} off by {e:.3e}, bound {bd:.3e}")
        if e >= worst[f][0]:
            worst[f] = [e, bd]


def check_truncated(case, run):
    """One truncated-solve case through `run(pd, rd, q0, n_seeds, lo, hi, **opts)` (the dict of HipBoundMPC.ik) at every depth:
    iters, status, seed equal, the floating-point outputs within FACTOR x REF_GAP, every required class present among the decidable
    lanes, at most 2 % of the lanes undecidable.  Returns the number of undecidable lanes."""
    check_longdouble()
    kind, ch = case["kind"], chain_of(case["table"])
    recs = replays(case)
    B = len(recs)
    undec = [undecidable_from(r, d) for r, d in zip(recs, replays(case, np.float64))]
    n_undec = sum(u is not None for u in undec)
    assert n_undec <= 0.02 * B, f"{case['name']}: {n_undec} of {B} lanes undecidable"
    fails = []
    for m in DEPTHS:
        out = run(case["pd"], case["rd"], case["q0"], 1, case["lo"], case["hi"], max_iter=m, **case["opts"])
        worst = {f: [0.0, bound(kind, f, m)] for f in FLOATS}
        assert (out["seed"] == 0).all()
        for b in range(B):
            if undec[b] is None or undec[b] > m:
                _compare(kind, m, outputs(ch, recs[b], m, case["pd"][b], case["rd"][b]), out, b, worst, fails, case["name"])
        print(f"{case['name']:>18} depth {m:2d}  worst / bound: " + "  ".join(f"{f} {worst[f][0]:.1e} / {worst[f][1]:.1e}" for f in FLOATS))
    assert not fails, "\n".join(fails[:20])
    present = {c for r, u in zip(recs, undec) for c, k in r["classes"] if u is None or k < u}
    at = lambda c: {k for r, u in zip(recs, undec) for cc, k in r["classes"] if cc == c and (u is None or k < u)}
    for c in case["require"]:
        if c == "clamp_pred":
            big = max(r.get("clamp_pred", 0.0) for r in recs)
            assert big > max(bound(kind, "rcost", m) for m in DEPTHS), (case["name"], c, big)
        elif c == "status1" and kind == "far":
            assert at(c) >= set(DEPTHS), (case["name"], "status 1 at every depth", at(c))
        else:
            assert c in present, (case["name"], c)
    if kind == "stall":
        assert STALL_TRIALS in DEPTHS and at("rejected_3") and {r["end"] for r in recs} == {(2, STALL_TRIALS)}
    return n_undec


# --- seeds ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seed_case(tname):
    """63 instances, instance s - 1 with the chain's pose at ITS seed point s as the target, from starts q0 != 0 inside the box"""
    table = TABLES[tname]
    lo, hi = limits(table)
    rng = np.random.default_rng(dict(iiwa14=11, gen3=12, generic=13)[tname])
    q0 = np.clip(rng.normal(0.0, 0.7, (63, 7)), lo, hi)
    pts = [seed_point(s, q0[s - 1], lo, hi) for s in range(1, 64)]
    pd, rd = _poses(table, [p[0] for p in pts])
    return dict(table=tname, pd=pd, rd=rd, q0=q0, q=np.array([p[0] for p in pts]), scale=np.array([p[1] for p in pts]))


def seed_run(tname, run):
    """the call of the seed case: row s - 1 of its q is the kernel's own seed point s of that instance"""
    c = seed_case(tname)
    return run(c["pd"], c["rd"], c["q0"], 64, None, None, max_iter=0)


def check_seeds(tname, run):
    """n_seeds = 64, max_iter = 0: only seed s has J <= tol_cost, so the call returns seed s, status 0, iters 0 and the seed point
    itself.  "Within 4 ulp of its magnitude": the map lo + h (hi - lo) (q0 + (2 h - 1) pi) cancels, so a double evaluation of it is
    good to roundings of its largest term, not of its result; the ulp is that of max(|lo|, |hi|, hi - lo) (max(|q0|, pi)).
    Measured, CPU build and MI355X: at most 2 ulp of that term; in ulps of |q| itself up to 357 (Gen3), which no double evaluation
    of the map can avoid."""
    c = seed_case(tname)
    out = seed_run(tname, run)
    assert np.array_equal(out["seed"], np.arange(1, 64)), out["seed"]
    assert (out["status"] == 0).all() and (out["iters"] == 0).all()
    ulps = np.abs(out["q"] - c["q"]) / np.spacing(c["scale"])
    print(f"seeds-{tname}: worst |q - exact seed point| = {ulps.max():.2f} ulp of the map's largest term (bound 4), "
          f"{(np.abs(out['q'] - c['q']) / np.spacing(np.abs(c['q']))).max():.1f} ulp of |q| itself")
    assert ulps.max() <= 4.0


# --- winner --------------------------------------------------------------------------------------------------------------------
WINNER_DEPTH = 5
TIE_SEED = 5


@functools.lru_cache(maxsize=None)
def winner_case(tname):
    """Five instances, run with n_seeds = 2, 8 and 64 at a depth where some seeds have converged and others have not:
    0  the start is a stationary point that misses the target (180 degrees): seed 0 has status 0 with J = 8 and must outrank every
       unconverged seed of lower cost
    1  a target next to the start: seed 0 converges
    2  a target next to the instance's seed point 1, the start far away
    3  a target next to seed point 3, the start far away
    4  a target next to seed point TIE_SEED; the checks replace its q0 by that seed point (see check_winner)"""
    table = TABLES[tname]
    lo, hi = limits(table)
    rng = np.random.default_rng(dict(iiwa14=21, gen3=22, generic=23)[tname])
    q0 = _box_sample(rng, table, 5, 0.3)
    near = lambda q: np.clip(q + rng.normal(0.0, 0.08, 7), lo, hi)
    tq = [q0[0], near(q0[1]), near(seed_point(1, q0[2], lo, hi)[0]), near(seed_point(3, q0[3], lo, hi)[0]),
          near(seed_point(TIE_SEED, q0[4], lo, hi)[0])]
    pd, rd = _poses(table, tq)
    rd[0] = _rot_about(rng.normal(size=3), np.pi) @ rd[0]
    return dict(table=tname, kind="seeds", name=f"seeds-{tname}", pd=pd, rd=rd, q0=q0)


_LANES = {}


def _lane(tname, T, pd, rd, start, lo, hi):
    k = (tname, T, pd.tobytes(), rd.tobytes(), start.tobytes())
    if k not in _LANES:
        _LANES[k] = replay(chain_of(tname, T), pd, rd, start, lo, hi, {}, WINNER_DEPTH)
    return _LANES[k]


def winner_lanes(case, q0=None, T=LD):
    """the replays of all 64 seeds of every instance of a winner case: [instance][seed]"""
    lo, hi = limits(TABLES[case["table"]])
    q0 = case["q0"] if q0 is None else q0
    return [[_lane(case["table"], T, case["pd"][b], case["rd"][b], seed_point(s, q0[b], lo, hi)[0], lo, hi) for s in range(64)]
            for b in range(len(q0))]


def check_winner(tname, run, tie_point=None):
    """tie_point: what the kernel returned for seed TIE_SEED of a box (check_seeds on a table whose joints are all limited).  It
    becomes q0 of instance 4, so lanes 0 and TIE_SEED of that instance start from the same bits, run the same arithmetic and tie
    exactly in status and cost: seed 0 must be reported.  The reference gives both lanes that start as well."""
    check_longdouble()
    case = winner_case(tname)
    table = TABLES[tname]
    lo, hi = limits(table)
    ch = chain_of(tname)
    q0 = case["q0"].copy()
    if tie_point is not None:
        exact, scale = seed_point(TIE_SEED, q0[4], lo, hi)
        assert (np.abs(tie_point - exact) <= 4 * np.spacing(scale)).all()
        q0[4] = tie_point
    lanes, lanes_d = winner_lanes(case, q0), winner_lanes(case, q0, np.float64)
    if tie_point is not None:
        lanes[4][TIE_SEED], lanes_d[4][TIE_SEED] = lanes[4][0], lanes_d[4][0]
    B, m = len(q0), WINNER_DEPTH
    fails, seen, n_undec = [], set(), 0
    for n, idx in ((2, range(B)), (8, range(B)), (64, range(B)), (2, [1])):           # the last call has B = 1
        idx = list(idx)
        out = run(case["pd"][idx], case["rd"][idx], q0[idx], n, None, None, max_iter=m)
        worst = {f: [0.0, bound("seeds", f, m)] for f in FLOATS}
        for i, b in enumerate(idx):
            res = [at_depth(lanes[b][s], m) for s in range(n)]
            keys = [key(r[3], r[1], s) for s, r in enumerate(res)]
            w = min(range(n), key=lambda s: keys[s])
            tie = tie_point is not None and b == 4 and n > TIE_SEED
            und = any(undecidable_from(lanes[b][s], lanes_d[b][s]) is not None for s in range(n))
            for s in range(n):
                if s != w and keys[s][0] == keys[w][0] and not (tie and {s, w} == {0, TIE_SEED}) and \
                        abs(np.sqrt(keys[s][1]) - np.sqrt(keys[w][1])) <= 2 * bound("seeds", "rcost", m):
                    und = True
            if und:
                n_undec += 1
                continue
            if int(out["seed"][i]) != w:
                fails.append(f"winner-{tname} n_seeds {n} b={b}: seed {int(out['seed'][i])}, reference {w} "
                             f"(keys {keys[int(out['seed'][i])]} / {keys[w]})")
                continue
            o = outputs(ch, lanes[b][w], m, case["pd"][b], case["rd"][b])
            _compare("seeds", m, o, out, i, worst, fails, f"winner-{tname} n_seeds {n}")
            if any(k[0] == 1 and k[1] < keys[w][1] for k in keys) and keys[w][0] == 0:
                seen.add("converged_outranks_cheaper")
            if tie and w == 0 and keys[TIE_SEED][:2] == keys[0][:2]:
                seen.add("exact_tie")
            if w > 0:
                seen.add("later_seed_wins")
            if {k[0] for k in keys} == {0, 1}:
                seen.add("mixed")
        print(f"winner-{tname} n_seeds {n:2d} B {len(idx)}  worst / bound: " + "  ".join(f"{f} {worst[f][0]:.1e} / {worst[f][1]:.1e}" for f in FLOATS))
    assert not fails, "\n".join(fails[:20])
    assert n_undec <= 0.02 * (3 * B + 1), n_undec
    need = {"converged_outranks_cheaper", "later_seed_wins", "mixed"} | ({"exact_tie"} if tie_point is not None else set())
    assert seen >= need, (tname, need - seen)
    return n_undec


# --- model ---------------------------------------------------------------------------------------------------------------------
MODEL_GAP = {'J': 4.5e-15, 'gh': 1.1e-15, 'H': 2.2e-15}          # worst |double - extended| of J, gh and H of the explicit model over model_points of the three tables


@functools.lru_cache(maxsize=None)
def model_points(tname):
    rng = np.random.default_rng(dict(iiwa14=31, gen3=32, generic=33)[tname])
    q = _box_sample(rng, TABLES[tname], 16, 0.0)
    pd = rng.normal(0.0, 0.5, (16, 3))
    rd = np.array([_rot_about(rng.normal(size=3), rng.uniform(0.0, np.pi)) for _ in range(16)])
    return q, pd, rd


def measure_model_gap():
    w = dict(J=0.0, gh=0.0, H=0.0)
    for tname in TABLES:
        q, pd, rd = model_points(tname)
        for b in range(16):
            a, d = chain_of(tname).model(q[b], pd[b], rd[b]), chain_of(tname, np.float64).model(q[b], pd[b], rd[b])
            for k, x, y in zip(("J", "gh", "H"), a, d):
                w[k] = max(w[k], _absmax(x, y))
    return w


def check_model(tname, model):
    """model(q, pd, rd, robot=table) -> (J, gh [7], H [7, 7]) of the kernel against r^T r, Jr^T r and Jr^T Jr, entry by entry"""
    check_longdouble()
    q, pd, rd = model_points(tname)
    w = dict(J=0.0, gh=0.0, H=0.0)
    for b in range(16):
        ref = chain_of(tname).model(q[b], pd[b], rd[b])
        for k, x, y in zip(("J", "gh", "H"), ref, model(q[b], pd[b], rd[b], robot=TABLES[tname])):
            w[k] = max(w[k], _absmax(x, y))
    print(f"model-{tname}  worst / bound: " + "  ".join(f"{k} {w[k]:.1e} / {FACTOR * MODEL_GAP[k]:.1e}" for k in w))
    for k in w:
        assert w[k] <= FACTOR * MODEL_GAP[k], (tname, k, w[k])


# --- forward kinematics on the generic table -----------------------------------------------------------------------------------
def fk_reference(table, q, dq):
    """Every key of HipBoundMPC.fk / oracle_lib.fk_batch from the plain chain in extended precision and derivatives of it alone:
    jac = d(p, rotation) / dq by the complex step (angular rows: vee((dR/dq_j) R^T)), dvdq = d(jac dq) / dq with jac dq by the complex
    step along dq and the outer derivative by fourth-order central differences (h = 1e-4: truncation h^4 f^(5) / 30 ~ 1e-16,
    rounding 1e-19 / h)."""
    ch = Chain(table, LD)
    B = q.shape[0]
    out = dict(ee_pos=np.zeros((B, 3)), ee_rot=np.zeros((B, 3, 3)), col_pts=np.zeros((B, 6, 3)), jac=np.zeros((B, 6, 7)),
               dvdq=np.zeros((B, 6, 7)))
    h, hd = LD(H_CS), LD(1e-4)
    vee = lambda S: np.stack([S[..., 2, 1] - S[..., 1, 2], S[..., 0, 2] - S[..., 2, 0], S[..., 1, 0] - S[..., 0, 1]], -1) / 2

    def twist(Q):                                   # (dp, vee(dR R^T)) / h of complex points Q [..., 7]
        p, R, *_ = ch.fk(Q)
        return np.concatenate([p.imag, vee(R.imag @ np.swapaxes(R.real, -1, -2))], -1) / h

    for b in range(B):
        qb, dqb = q[b].astype(LD), dq[b].astype(LD)
        p, R, col, _, _ = ch.fk(qb)
        out["ee_pos"][b], out["ee_rot"][b], out["col_pts"][b] = p, R, col
        Q = np.tile(qb.astype(np.clongdouble), (7, 1))
        Q[np.arange(7), np.arange(7)] += 1j * h
        out["jac"][b] = twist(Q).T
        v = lambda x: twist(x.astype(np.clongdouble) + 1j * h * dqb)
        e = np.eye(7, dtype=LD) * hd
        out["dvdq"][b] = ((-v(qb + 2 * e) + 8 * v(qb + e) - 8 * v(qb - e) + v(qb - 2 * e)) / (12 * hd)).T
    return out


def check_fk(table, got, q, dq, tol=1e-12):
    ref = fk_reference(table, q, dq)
    assert set(got) == set(ref)
    for k in ref:
        e = np.abs(got[k] - ref[k]).max()
        print(f"fk-{table['name']} {k}: {e:.1e} / {tol:.0e}")
        assert e <= tol, k


if __name__ == "__main__":
    import pprint
    import sys
    check_longdouble()
    reps = range(16)
    gaps, floors = {}, dict.fromkeys(DECS, 0.0)
    for kind in (sys.argv[1:] or KINDS):
        cs = [c for t in TABLES for r in reps for c in truncated_cases(t, r) if c["kind"] == kind]
        gaps[kind], fl, n = measure_gaps(cs)
        floors = {f: max(floors[f], fl[f]) for f in DECS}
        n0 = measure_gaps([c for c in cs if c["rep"] == 0])[2]
        print(f"# {kind}: lanes whose integers differ between the two runs: {n} of {sum(len(c['q0']) for c in cs)} (rep 0: {n0})")
    wl = lambda c: (sum(winner_lanes(c), []), sum(winner_lanes(c, T=np.float64), []), np.repeat(c["pd"], 64, 0), np.repeat(c["rd"], 64, 0))
    gaps["seeds"], fl, n = measure_gaps([winner_case(t) for t in TABLES], wl, (WINNER_DEPTH,))
    floors = {f: max(floors[f], fl[f], np.finfo(float).eps) for f in DECS}
    print(f"# seeds: lanes whose integers differ: {n}")
    print("REF_GAP = \\")
    pprint.pprint({k: {f: {m: _round_up(v) for m, v in fm.items()} for f, fm in kf.items()} for k, kf in gaps.items()}, width=150, sort_dicts=False)
    print("DEC_FLOOR =", {f: _round_up(v) for f, v in floors.items()})
    print("MODEL_GAP =", {k: _round_up(v) for k, v in measure_model_gap().items()})
