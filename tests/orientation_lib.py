"""Independent reference of the device loop's orientation block (csrc/bmpc_loop.hpp: lp_rotvec_to_mat, lp_mat_to_rotvec,
lp_euler_zyx, lp_jac_inv, lp_initial_rot_errors, the dual basis v1..v3, lp_integrate_rot_ref) -- TEST INFRASTRUCTURE ONLY.

numpy in np.longdouble; nothing here comes from so3.py, from bmpc_loop.hpp or from scipy: every quantity is written down from
its mathematical definition.
  exp(v)      Rodrigues' formula  I + sin a / a W + (1 - cos a) / a^2 W^2,  W = skew(v), a = |v|
  log(M)      angle atan2(|w|, (tr M - 1) / 2) with w = vee(M - M^T) / 2 = sin a n; the axis from w, or past 120 deg from the
              largest column of (M + M^T) / 2 - cos a I = (1 - cos a) n n^T with the sign of w.  A result is JUDGED by the rotation
              distance |log(exp(v) M^T)| and |v| <= pi, so within 1e-12 of a half turn either sign of the axis passes.
  Euler       M = Rx(e2) Ry(e1) Rz(e0): M[0] = (c1 c0, -c1 s0, s1), M[:, 2] = (s1, -s2 c1, c2 c1).  Inside scipy's lock window
              (| |e1| - pi/2 | <= ~1e-7) the convention of the library the reference calls: e2 = 0 and e0 = atan2(M[1,0], M[1,1])
              carries e0 +- e2.  The switch itself sits somewhere in LOCK_IN .. LOCK_OUT: no input may lie there.
  J^-1        the reference's  I + sign W / 2 + (1 / a^2 - (1 + cos a) / (2 a sin a)) W^2  with a = |v| + 1e-6, and -- as the thing
              that formula is meant to be -- the derivative of log(exp(v) exp(d)) (right, sign +1) / log(exp(d) exp(v)) (left, -1)
  dual basis  rows of [g h k]^-1 by the adjugate, no Gram matrix
  integrate   log(exp(w / |w| dphi |w|) exp(pr_ref)); the rotation is left alone below |w| = 1e-4

TOLERANCES.  HOST_WORST[quantity/family] is the worst deviation of the host mirror (so3.py on scipy and libm, in double) from this
reference over the cases below, measured with `python tests/test_loop_orientation.py` and rounded up, relative to the scale noted next to
it; the CPU build and the GPU get MARGIN = 32 times that (another libm, another contraction order), and where the host's figure is 0
the floor is 16 ulp of the scale.  The derived terms are added on top, each where it applies:
  * an input matrix with orthogonality defect d = max|M M^T - I| is a rotation only to d: log and the Euler split get + 4 d
  * first and third Euler angle come from atan2 of two entries of size cos e1 that carry the matrix' rounding: scale 1 / cos e1
  * inside the lock window e2 = 0 is a convention, not the matrix: the rebuilt matrix is off by up to 2 | |e1| - pi/2 | (the two
    entry pairs of size cos e1 that the convention turns)
  * the dual basis goes through the Gram matrix on host and device alike: scale cond([g h k])^2
  * the +pi rule replaces an outer Euler angle within 1e-12 of +-pi: + 1e-12 where it applied
  * next to a half turn the sign of the axis is decided by entries of size sin a: within 1e-12 of it both signs are the answer
"""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
PI = 4 * np.arctan(LD(1))
MARGIN = 32.0
LOCK_IN, LOCK_OUT = 0.5e-7, 2e-7           # scipy 1.15.3 switches between 1.0e-7 and 1.1e-7
HALF_TURN = 1e-12                          # closer to pi than this: the sign of the axis is free
assert np.finfo(LD).eps < 2e-19, "the reference needs an extended-precision long double"

# the scale every figure of a quantity is relative to
SCALE = {
    "exp": "1 (matrix entries)",
    "log": "1 (rotation distance, rad), + 4 defect",
    "euler_rebuild": "1 (matrix entries), + 4 defect, + 2 lock distance inside the window",
    "euler_e1": "1 (rad), + 4 defect",
    "euler_e02": "1 / cos e1 outside the window, 1 inside (rad), + 4 defect / cos e1",
    "jac": "1 + |v|^2 (matrix entries)",
    "dtau": "1 (rotation distance, rad)",
    "dtau_par": "1 (rad)",
    "dtau_o12": "1 / cos e1 outside the window, 1 inside (rad)",
    "dual": "cond([g h k])^2 max|v_i|",
    "pr_ref": "1 (rotation distance, rad)",
    "iw_ref": "max(1, |iw_ref|)",
    "p_lie": "1 (rotation distance to the oracle's R_ee, rad)",
}
# "quantity/family" -> worst deviation of the host mirror over that scale, rounded up (python tests/test_loop_orientation.py prints it)
HOST_WORST = {
    "exp/small": 2.3e-16, "exp/mid": 3.0e-16, "exp/half": 3.9e-16,
    "log/small": 0.0, "log/mid": 2.9e-16, "log/half": 3.9e-16,
    "euler_rebuild/free": 5.2e-16, "euler_rebuild/near": 2.3e-17, "euler_rebuild/lock": 3.6e-17, "euler_rebuild/pi_outer": 0.0,
    "euler_e1/free": 1.4e-16, "euler_e1/near": 0.0, "euler_e1/lock": 4.3e-16, "euler_e1/pi_outer": 0.0,
    "euler_e02/free": 5.3e-16, "euler_e02/near": 0.0, "euler_e02/lock": 1.9e-16, "euler_e02/pi_outer": 0.0,
    # (1 + cos a) / sin a cancels next to a half turn, in so3.py as on the device: rel. error eps / (1 + cos a) of a term of size
    # (pi - a) / (4 pi) at pi - a = 1e-6, i.e. some 1e-11 of the coefficient of W^2 -- hence the two `half` figures
    "jac/small": 2.5e-16, "jac/mid": 2.2e-16, "jac/half": 6.5e-12,
    "dtau/small": 7.1e-16, "dtau/mid": 7.4e-16, "dtau/half": 8.0e-16, "dtau/near": 9.8e-16, "dtau/lock": 9.4e-16, "dtau/pi_outer": 8.2e-16,
    "dtau_par/small": 5.5e-16, "dtau_par/mid": 6.6e-16, "dtau_par/half": 1.3e-15, "dtau_par/near": 7.2e-16, "dtau_par/lock": 8.4e-16,
    "dtau_par/pi_outer": 5.0e-16,
    "dtau_o12/small": 1.6e-15, "dtau_o12/mid": 1.2e-15, "dtau_o12/half": 1.1e-15, "dtau_o12/near": 9.7e-16, "dtau_o12/lock": 1.2e-15,
    "dtau_o12/pi_outer": 4.1e-16,
    "dual/mid": 8.0e-16, "dual/near": 1.4e-16, "dual/lock": 4.7e-16, "dual/half": 5.5e-10,
    "pr_ref/rest": 5.1e-16, "pr_ref/moved": 9.7e-16, "pr_ref/flip": 1.2e-15,
    "iw_ref/all": 2.5e-16,
    "p_lie/generic": 0.0, "p_lie/half": 0.0,      # (the host takes the logarithm of the very matrix the check holds it against)
}


def bound(key, scale=1.0, extra=0.0):
    return max(MARGIN * HOST_WORST[key], 16 * EPS) * scale + extra


# ---- the definitions ---------------------------------------------------------------------------------------------------
def ld(a):
    return np.array(a, dtype=LD)


def skew(w):
    w = ld(w)
    z = LD(0)
    return np.array([[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]], dtype=LD)


def exp(v):
    v = ld(v)
    a2 = v @ v
    a, W = np.sqrt(a2), skew(v)
    if a < 1e-2:
        A = 1 - a2 / 6 * (1 - a2 / 20 * (1 - a2 / 42 * (1 - a2 / 72)))
        B = (1 - a2 / 12 * (1 - a2 / 30 * (1 - a2 / 56 * (1 - a2 / 90)))) / 2
    else:
        A, B = np.sin(a) / a, 2 * np.sin(a / 2) ** 2 / a2
    return np.eye(3, dtype=LD) + A * W + B * (W @ W)


def _sin_axis(M):
    return ld([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]) / 2


def angle(M):
    M = ld(M)
    w = _sin_axis(M)
    return np.arctan2(np.sqrt(w @ w), (np.trace(M) - 1) / 2)


def log(M, hint=None):
    """The rotation vector of M with |v| <= pi.  Where the sign of the axis is free (HALF_TURN) it follows `hint`."""
    M = ld(M)
    w = _sin_axis(M)
    s, c = np.sqrt(w @ w), (np.trace(M) - 1) / 2
    t = np.arctan2(s, c)
    if c > -0.5:
        return w * (t / s) if s > 0 else np.zeros(3, dtype=LD)
    Nn = (M + M.T) / 2 - c * np.eye(3, dtype=LD)
    n = Nn[:, int(np.argmax(np.diag(Nn)))]
    n = n / np.sqrt(n @ n)
    if n @ w < 0:
        n = -n
    if hint is not None and PI - t < HALF_TURN and n @ ld(hint) < 0:
        n = -n
    return t * n


def rot_dist(v, M):
    """How far the rotation vector v is from the matrix M, as a rotation angle."""
    return float(angle(exp(v) @ ld(M).T))


def defect(M):
    M = ld(M)
    return float(np.abs(M @ M.T - np.eye(3, dtype=LD)).max())


def _rot(axis, a):
    c, s = np.cos(LD(a)), np.sin(LD(a))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3, dtype=LD)
    R[i, i] = c; R[j, j] = c; R[i, j] = -s; R[j, i] = s
    return R


def euler_build(e):
    return _rot(0, e[2]) @ _rot(1, e[1]) @ _rot(2, e[0])


def euler_exact(M):
    M = ld(M)
    return ld([np.arctan2(-M[0, 1], M[0, 0]), np.arctan2(M[0, 2], np.hypot(M[0, 0], M[0, 1])), np.arctan2(-M[1, 2], M[2, 2])])


def lock_distance(M):
    return float(abs(PI / 2 - abs(euler_exact(M)[1])))


def euler_reference(M):
    """-> (angles, locked).  The split the reference's library returns, with the project's +pi rule for the outer angles."""
    M = ld(M)
    e, d = euler_exact(M), lock_distance(M)
    assert not (LOCK_IN <= d <= LOCK_OUT), f"lock distance {d:.3e} lies in the undecidable band"
    locked = d < LOCK_IN
    if locked:
        e[0], e[2] = np.arctan2(M[1, 0], M[1, 1]), LD(0)
    for i in (0, 2):
        if abs(abs(e[i]) - PI) < 1e-12:
            e[i] = PI
    return e, locked


def jac_inv_formula(v, sign):
    v = ld(v)
    a, W = np.sqrt(v @ v) + LD(1e-6), skew(v)
    coef = 1 / (a * a) - (1 + np.cos(a)) / (2 * a * np.sin(a))
    return np.eye(3, dtype=LD) + LD(sign) * W / 2 + coef * (W @ W)


def jac_inv_true(v, sign, h=LD(1e-4)):
    """d/dd log(exp(v) exp(d)) (sign +1) or d/dd log(exp(d) exp(v)) (sign -1) at d = 0 by fourth-order central differences:
    truncation h^4 ~ 1e-16, rounding 1e-19 / h ~ 1e-15.  For |v| well below pi."""
    Rv, J = exp(v), np.zeros((3, 3), dtype=LD)

    def f(d):
        return log(Rv @ exp(d) if sign > 0 else exp(d) @ Rv)
    for j in range(3):
        d = np.zeros(3, dtype=LD)
        d[j] = h
        J[:, j] = (8 * (f(d) - f(-d)) - (f(2 * d) - f(-2 * d))) / (12 * h)
    return J


# |coef(a + 1e-6) - coef(a)| |W^2| <= 1e-6 max|coef'| a^2 with |coef'| < 0.02 on [0, pi] (coef = 1/12 + a^2/720 + ..., coef'(pi) =
# -2/pi^3 + 1/(4 pi) = 0.015), plus the 1e-15 of the difference quotient
def jac_quirk_bound(v):
    return 0.02e-6 * float(ld(v) @ ld(v)) + 1e-13


def initial_errors(pr, pr_ref, dpn, br1, br2, hint=None):
    """-> dtau (free sign follows `hint`), dtau_par, dtau_o1, dtau_o2, the Euler angles, locked, lock distance, cos e1."""
    M = exp(pr) @ exp(pr_ref).T
    r01 = np.column_stack((ld(br2), ld(dpn), ld(br1)))
    d01 = r01.T @ M @ r01
    e, locked = euler_reference(d01)
    return dict(dtau=log(M, hint), M=M, par=e[1] * ld(dpn), o1=e[0] * ld(br1), o2=e[2] * ld(br2), eul=e, locked=locked,
                lock_distance=lock_distance(d01), cos1=float(np.cos(euler_exact(d01)[1])))


def inv3(B):
    B = ld(B)
    C = np.zeros((3, 3), dtype=LD)
    for i in range(3):
        for j in range(3):
            a, b = [(1, 2), (0, 2), (0, 1)][i], [(1, 2), (0, 2), (0, 1)][j]
            C[i, j] = (-1) ** (i + j) * (B[a[0], b[0]] * B[a[1], b[1]] - B[a[0], b[1]] * B[a[1], b[0]])
    det = B[0] @ C[0]
    return C.T / det


def _logs(M):
    """log(M), both signs where the sign is free."""
    v = log(M)
    return [v, -v] if float(PI - angle(M)) < HALF_TURN else [v]


def dual_basis(dtau0, dtau_o1, dtau_par, br1, dpn, br2):
    """-> [(V, B)], cond: V = rows v1, v2, v3 of [g h k]^-1 and B = [g h k], one pair per admissible choice of free signs."""
    g = jac_inv_formula(dtau0, +1) @ ld(br1)
    rest1 = exp(dtau0) @ exp(dtau_o1).T
    rest2 = rest1 @ exp(dtau_par).T
    out = []
    for l1 in _logs(rest1):
        for l2 in _logs(rest2):
            B = np.column_stack((g, jac_inv_formula(l1, +1) @ ld(dpn), jac_inv_formula(l2, +1) @ ld(br2)))
            out.append((inv3(B), B))
    return out, float(np.linalg.cond(out[0][1].astype(float)))


def integrate(pr_ref, omega, dphi, hint=None):
    """-> (rotation matrix, rotation vector) of the reference orientation after advancing the path parameter by dphi."""
    om = ld(omega)
    n = np.sqrt(om @ om)
    M = exp(om / n * (LD(dphi) * n)) @ exp(pr_ref) if n > 1e-4 else exp(pr_ref)
    return M, log(M, hint)


# ---- input families ----------------------------------------------------------------------------------------------------
ANGLES = [0.0, 1e-9, 1e-5, 0.999e-3, 1e-3, 1.001e-3, 0.1, 1.0, 2.0, 3.0, float(PI) - 1e-3, float(PI) - 1e-6, float(PI) - 1e-9, float(PI)]
PITCHES = [s * (float(PI) / 2 - d) for d in (1e-5, 1e-6, 1e-8, 1e-9, 0.0) for s in (1, -1)]
OUTER = [(0.3, -0.7), (-2.1, 1.3), (1.1, 2.6), (-0.4, -1.9)]       # first and third angle of the pitch family: never 0
TRIVIAL = (np.array([0.0, 0, -1]), np.array([0.0, 1, 0]), np.array([1.0, 0, 0]))        # br2, dpn, br1 of the start-up path


def unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def random_frame(rng):
    """Orthonormal (br2, dpn, br1), right-handed as the planner's bases are (br2 = dpn x br1)."""
    a = unit(rng)
    b = rng.normal(size=3)
    b -= (a @ b) * a
    b /= np.linalg.norm(b)
    return np.cross(a, b), a, b


def error_specs(rng):
    """The orientation errors of the families, as (tag, make(frame) -> rotation matrix in long double).  The angle family turns
    about the coordinate axes and about random axes; the pitch family is Rx(e2) Ry(pitch) Rz(e0) in the frame (br2, dpn, br1);
    `pi_outer` makes the first / third angle a half turn (the project's +pi rule)."""
    specs = []
    for a in ANGLES:
        for k in range(5):
            ax = np.eye(3)[k] if k < 3 else unit(rng)
            specs.append((f"angle:{a:.17g}:{'xyz'[k] if k < 3 else 'random'}", (lambda f, v=ld(ax) * LD(a): exp(v)), "angle"))
    for pitch in PITCHES:
        for e0, e2 in OUTER:
            def make(f, e=(e0, pitch, e2)):
                r01 = np.column_stack([ld(x) for x in f])
                return r01 @ euler_build(e) @ r01.T
            specs.append((f"pitch:{pitch:.17g}:{e0}:{e2}", make, "pitch"))
    for i in (0, 2):
        def make(f, i=i):
            e = [LD(0.4), LD(-0.3), LD(0.2)]
            e[i] = PI
            r01 = np.column_stack([ld(x) for x in f])
            return r01 @ euler_build(e) @ r01.T
        specs.append((f"pi_outer:{i}", make, "pi_outer"))
    return specs


def reference_rotvec(E, pr):
    """The double rotation vector v with exp(pr) exp(v)^T = E as nearly as a double can say it: v = log(E^T exp(pr))."""
    return log(ld(E).T @ exp(pr)).astype(float)


# Joint configurations of the 7-axis arm whose end-effector orientation R_ee(q) lies within 1e-6 of a half turn (found once with the
# project's inverse kinematics on its CPU build for targets turned by exactly pi about the given axes), and generic ones.
Q_HALF_TURN = [
    [0.4638680367598892, -0.5553911023222109, 1.2969853600890948, -1.4467634355278742, -1.0900691720352875, -1.2839742242111711, 0.26294810894614185],
    [-2.966652252513571, 0.2945913559303172, 2.9478280212490553, -0.636141688898661, 0.011594076450882807, -1.9211332924861901, -1.5067181574925956],
    [-2.256808873219749, -0.2985642244993721, 1.4944750455490914, -0.7837625050387849, -1.112786996712129, 1.29562471875501, -0.5475483501045045],
    [-0.1020793094224703, 0.533548129406625, -1.9384075987705927, 0.2923097736702445, -2.465636577937079, 0.9371980565680194, -2.7331735580403356],
    [-2.4729678481428845, 0.052530968847642204, -0.23233312846599138, 0.33110986738255355, -0.21432395265575174, -0.49122049071444196, 1.524087897500919],
    [-2.2564979794441573, 0.6808712659904859, -1.2850980440372328, -0.43330559784347045, -0.28941675646240167, 0.5890944621725436, -2.655602859372567],
]
Q_GENERIC = [
    [-0.278585067423031, -0.1802891188231095, 0.14634004246632482, -0.9433453612306, -0.0061614880442064646, -0.5034764967352634, -1.5342981483772942],
    [-0.3197057385205637, 0.4193662620828109, -0.7020273197289115, 0.5364162111726081, 1.028161464787732, -1.2214091045286808, -1.0425401003563546],
    [-0.770325444610237, 0.23197852192494306, -0.046401023382121265, 0.17107436113961105, -1.5174750760349207, -0.5350481291222299, -1.2432366647823896],
    [0.8758593638849439, 0.46113714750678025, -0.6946933594353495, 0.9454089288074481, -1.297342972614853, -1.2118487207699884, -0.46416809480227594],
]
Q_ALL = Q_GENERIC + Q_HALF_TURN


class Worst:
    """Worst deviation / bound per "quantity/family": what the tests print and DESIGN.md quotes.  With measure=True (the host mirror,
    when HOST_WORST is being established) the figure kept is the deviation over its scale, after the derived terms."""

    def __init__(self, measure=False):
        self.measure, self.ratio, self.dev, self.count = measure, {}, {}, {}

    def add(self, key, dev, scale=1.0, extra=0.0, what=""):
        dev = float(dev)
        r = max(dev - extra, 0.0) / scale if self.measure else dev / bound(key, scale, extra)
        if not r < self.ratio.get(key, -1.0):
            self.ratio[key] = r
            self.dev[key] = (dev, what)
        self.count[key] = self.count.get(key, 0) + 1

    def report(self, title):
        print(title)
        for k in sorted(self.ratio):
            print(f"  {k:24s} n={self.count[k]:5d}  worst deviation {self.dev[k][0]:.3e} = {self.ratio[k]:9.3e} "
                  f"{'x scale' if self.measure else 'x bound'}   {self.dev[k][1]}")

    def failures(self):
        return {k: (r, self.dev[k]) for k, r in self.ratio.items() if not r <= 1.0}


def fam_angle(a):
    return "small" if a <= 1.0011e-3 else ("mid" if a <= 3.0 else "half")


def fam_pitch(pitch):
    return "near" if float(PI) / 2 - abs(pitch) >= 0.99e-6 else "lock"


def fam_of(tag):
    kind, *rest = tag.split(":")
    return fam_angle(float(rest[0])) if kind == "angle" else (fam_pitch(float(rest[0])) if kind == "pitch" else "pi_outer")


def mat_branch(M):
    """Which of (M00, M11, M22, trace) is largest: the four ways a matrix can ask to be turned into a quaternion."""
    return int(np.argmax([M[0, 0], M[1, 1], M[2, 2], M[0, 0] + M[1, 1] + M[2, 2]]))


# ---- the helpers one by one ----------------------------------------------------------------------------------------------
def check_exp_log(sub, W, rng):
    branches, fams = set(), set()
    for a in ANGLES:
        for k in range(7):
            ax = np.eye(3)[k] * (1 if k % 2 else -1) if k < 3 else unit(rng)
            v = a * ax
            fam = fam_angle(a)
            W.add("exp/" + fam, np.abs(ld(sub.exp(v)) - exp(v)).max(), what=f"angle {a!r}")
            M = exp(v).astype(float)
            vk = np.asarray(sub.log(M), float)
            d = defect(M)
            W.add("log/" + fam, rot_dist(vk, M), extra=4 * d, what=f"angle {a!r}")
            assert np.linalg.norm(vk) <= float(PI) * (1 + 4 * EPS), (a, vk)
            if float(PI) - a > 1e-3:          # away from the half turn the vector itself is determined
                W.add("log/" + fam, np.abs(ld(vk) - log(M)).max(), extra=4 * d, what=f"vector, angle {a!r}")
            branches.add(mat_branch(M)); fams.add(fam)
    assert branches == {0, 1, 2, 3} and fams == {"small", "mid", "half"}, (branches, fams)


def euler_matrices(rng):
    """(tag, double matrix): the pitch family, generic rotations and the half turns of the outer angles with either sign of zero."""
    out = []
    for pitch in PITCHES:
        for e0, e2 in OUTER:
            out.append((f"pitch:{pitch:.17g}:{e0}:{e2}", euler_build((e0, pitch, e2)).astype(float)))
    for _ in range(60):
        out.append(("angle:1.0:random", exp(unit(rng) * rng.uniform(0.05, 3.1)).astype(float)))
    for z in (0.0, -0.0):
        M = np.diag([-1.0, -1.0, 1.0]); M[0, 1] = z
        out.append(("pi_outer:0", M))
        M = np.diag([1.0, -1.0, -1.0]); M[1, 2] = z
        out.append(("pi_outer:2", M))
    for i in (0, 2):
        for s in (1, -1):
            e = [LD(0.4), LD(-0.3), LD(0.2)]
            e[i] = s * (PI - LD(1e-13))
            out.append((f"pi_outer:{i}", euler_build(e).astype(float)))
    return out


def check_euler_one(W, key, M, ek, scipy_e=None):
    """The split ek of the double matrix M against the definition: rebuild, exact angles or the lock convention, the +pi rule."""
    M = np.asarray(M, float)
    ek = np.asarray(ek, float)
    ref, locked = euler_reference(M)
    d, ldist, c1 = defect(M), lock_distance(M), float(np.cos(euler_exact(M)[1]))
    ruled = 1e-12 if (ref[0] == PI or ref[2] == PI) else 0.0        # the +pi rule moves an outer angle by up to its radius
    W.add("euler_rebuild/" + key, np.abs(euler_build(ld(ek)) - ld(M)).max(), extra=4 * d + (2 * ldist if locked else 0.0) + ruled,
          what=f"lock distance {ldist:.1e}")
    W.add("euler_e1/" + key, abs(LD(ek[1]) - ref[1]), extra=4 * d, what=f"lock distance {ldist:.1e}")
    sc = 1.0 if locked else 1.0 / c1
    W.add("euler_e02/" + key, max(abs(LD(ek[0]) - ref[0]), abs(LD(ek[2]) - ref[2])), scale=sc, extra=4 * d * sc + ruled, what=f"lock distance {ldist:.1e}")
    if locked:
        assert ek[2] == 0.0, (key, ek)
        if scipy_e is not None:       # the convention is the library's: first angle as scipy has it on the same matrix
            W.add("euler_e02/" + key, abs(ek[0] - scipy_e[0]), extra=4 * d + HOST_WORST.get("euler_e02/" + key, 0.0), what="against scipy")
            assert scipy_e[2] == 0.0
    for i in (0, 2):
        if ref[i] == PI:
            assert ek[i] == np.pi, (key, i, ek)
    return locked


def check_euler(sub, W, rng, scipy_euler=None):
    seen = {}
    for tag, M in euler_matrices(rng):
        key = fam_of(tag) if not tag.startswith("angle") else "free"
        locked = check_euler_one(W, key, M, sub.euler(M), scipy_euler(M) if scipy_euler else None)
        seen[key] = seen.get(key, 0) + 1
        assert locked == (key == "lock"), (tag, locked)
    assert seen == {"near": 16, "lock": 24, "free": 60, "pi_outer": 8}, seen


def check_jac(sub, W, rng):
    fams = set()
    for a in ANGLES:
        for k in range(5):
            v = a * (np.eye(3)[k] if k < 3 else unit(rng))
            fam = fam_angle(a)
            fams.add(fam)
            for sign in (+1.0, -1.0):
                Jk = ld(sub.jac(v, sign))
                W.add("jac/" + fam, np.abs(Jk - jac_inv_formula(v, sign)).max(), scale=1 + a * a, what=f"angle {a!r}")
                if a <= 3.0:      # what the formula is: the inverse right / left Jacobian, up to its 1e-6
                    dq = float(np.abs(Jk - jac_inv_true(v, sign)).max())
                    assert W.measure or dq <= bound("jac/" + fam, 1 + a * a, jac_quirk_bound(v)), (a, sign, dq)
                    if a >= 0.1:      # ... and not the other one: the two differ by |v| in the skew part
                        assert np.abs(Jk - jac_inv_true(v, -sign)).max() > 0.5 * a
    assert fams == {"small", "mid", "half"}


def check_initial_errors_one(W, fam, out, pr, pr_ref, dpn, br1, br2):
    e0, par, o1, o2 = (np.asarray(x, float) for x in out)
    ref = initial_errors(pr, pr_ref, dpn, br1, br2, hint=e0)
    W.add("dtau/" + fam, rot_dist(e0, ref["M"]), what=f"angle {float(angle(ref['M'])):.9f}")
    assert np.linalg.norm(e0) <= float(PI) * (1 + 4 * EPS)
    what = f"lock distance {ref['lock_distance']:.1e}"
    W.add("dtau_par/" + fam, np.abs(ld(par) - ref["par"]).max(), what=what)
    sc = 1.0 if ref["locked"] else 1.0 / ref["cos1"]
    W.add("dtau_o12/" + fam, max(np.abs(ld(o1) - ref["o1"]).max(), np.abs(ld(o2) - ref["o2"]).max()), scale=sc, what=what)
    if ref["locked"]:
        assert (o2 == 0.0).all()
    return ref


def check_initial_errors(sub, W, rng):
    seen = set()
    for frame_kind in ("trivial", "random"):
        for tag, make, _ in error_specs(rng):
            br2, dpn, br1 = TRIVIAL if frame_kind == "trivial" else random_frame(rng)
            pr = unit(rng) * rng.uniform(0.1, 2.8)
            pr_ref = reference_rotvec(make((br2, dpn, br1)), pr)
            ref = check_initial_errors_one(W, fam_of(tag), sub.initial_errors(pr, pr_ref, dpn, br1, br2), pr, pr_ref, dpn, br1, br2)
            assert ref["locked"] == (fam_of(tag) == "lock"), (tag, ref["lock_distance"])
            seen.add((frame_kind, fam_of(tag)))
    assert len(seen) == 12, seen


def integrate_cases(rng):
    """(family, pr_ref, omega, phi0, phi1): |omega| on both sides of 1e-4 (`rest`: the rotation stays), generic advances, and
    advances that carry the result across the half turn, so that the returned vector flips."""
    out = []
    for n in (0.0, 0.5e-4, 1e-4 - 1e-8, 1e-4 + 1e-8, 2e-4, 0.3, 1.0, 2.5):
        for _ in range(4):
            out.append(("rest" if n <= 1e-4 else "moved", unit(rng) * rng.uniform(0.0, 3.0), unit(rng) * n, rng.uniform(0, 1), rng.uniform(1, 3)))
    for over in (0.1, 1e-3, 1e-6):
        for _ in range(3):
            ax = unit(rng)
            out.append(("flip", ax * (float(PI) - 0.05), ax * 0.7, 0.25, 0.25 + (0.05 + over) / 0.7))
    return out


def check_integrate_one(W, fam, out, pr_ref, omega, dphi):
    out = np.asarray(out, float)
    M, v = integrate(pr_ref, omega, dphi, hint=out)
    W.add("pr_ref/" + fam, rot_dist(out, M), what=f"angle {float(angle(M)):.9f}")
    assert np.linalg.norm(out) <= float(PI) * (1 + 4 * EPS)
    if float(PI - angle(M)) > 1e-9:          # the vector itself, with the eps / sin term of the axis next to the half turn
        W.add("pr_ref/" + fam, np.abs(ld(out) - v).max(), extra=16 * EPS / float(np.sin(angle(M)) + 1e-300) if fam == "flip" else 0.0, what="vector")
    return v


def check_integrate(sub, W, rng):
    seen = set()
    for fam, pr_ref, om, phi0, phi1 in integrate_cases(rng):
        v = check_integrate_one(W, fam, sub.integrate(pr_ref, om, phi0, phi1), pr_ref, om, LD(phi1) - LD(phi0))
        if fam == "flip":
            assert v @ ld(pr_ref) < 0              # the case does cross the half turn
        if fam == "rest":
            assert np.abs(v - ld(pr_ref)).max() < 1e-17 + 1e-18
        seen.add(fam)
    assert seen == {"rest", "moved", "flip"}


def check_helpers(sub, W, scipy_euler=None, seed=7):
    rng = np.random.default_rng(seed)
    check_exp_log(sub, W, rng)
    check_euler(sub, W, rng, scipy_euler)
    check_jac(sub, W, rng)
    check_initial_errors(sub, W, rng)
    check_integrate(sub, W, rng)


# ---- whole loop_prepare / loop_finish calls --------------------------------------------------------------------------------
# where the orientation block lands in the 875 parameters (offset, count), in the order of the solver's parameter vector
P_OFF = dict(iw_ref=(11, 3), dtau=(14, 12), dtau_par=(26, 12), dtau_o1=(38, 12), dtau_o2=(50, 12), jac_r=(70, 9), jac_l=(79, 9),
             dpn=(136, 12), br1=(172, 12), br2=(184, 12), v1=(232, 12), v2=(244, 12), v3=(256, 12))
COND_MAX = 1e3


def rollout_cases(seed=11):
    """One rollout per (error spec, kind of frame): segment i of rollout k carries spec k + 37 i, so every spec is met in segment 0
    (whose error also feeds jac_l / jac_r and every segment's rest rotations) and in segments 1 to 3, each segment with its own
    frame and its own r_taud.  The end-effector orientations cycle through Q_ALL.  With every rollout goes one case of the rotation
    reference's integration for loop_finish."""
    rng = np.random.default_rng(seed)
    specs = error_specs(rng)
    fin = []
    while len(fin) < 2 * len(specs):
        fin += integrate_cases(rng)
    cases = []
    for kind in ("trivial", "random"):
        for k in range(len(specs)):
            seg = [specs[(k + 37 * i) % len(specs)] for i in range(4)]
            frames = [TRIVIAL if kind == "trivial" else random_frame(rng) for _ in range(4)]
            qi = (k + (3 if kind == "random" else 0)) % len(Q_ALL)
            cases.append(dict(kind=kind, tags=[s[0] for s in seg], make=[s[1] for s in seg], frames=frames, qi=qi,
                              qfam="half" if qi >= len(Q_GENERIC) else "generic", fin=fin[len(cases)], pd_r=rng.normal(size=3),
                              dp=unit(rng)))
    return cases


def install(V, case, R_ee):
    """Overwrites, in the state view V of one rollout (made for the joint configuration Q_ALL[case qi], whose end-effector
    orientation is R_ee), what the orientation block reads: pr_ref and r_taud so that segment i sees the wanted error, the bases,
    the path direction; and for loop_finish the rotation the reference orientation starts from, its angular rate, the Lie-space
    reference the rate is added to, and a unit path direction along which the solution is planted."""
    pr = log(R_ee)
    for i in range(4):
        br2, dpn, br1 = case["frames"][i]
        v = reference_rotvec(case["make"][i](case["frames"][i]), pr)
        if i == 0:
            V["pr_ref"][:] = v
        else:
            V["rp_r_taud"].reshape(3, 4)[:, i] = v
        V["rp_dpdn"].reshape(3, 4)[:, i] = dpn
        V["rp_br1"].reshape(-1, 3)[i] = br1
        V["rp_br2"].reshape(-1, 3)[i] = br2
    _, pr_ref, om, phi0, phi1 = case["fin"]
    V["rp_r_tau"].reshape(-1, 3)[0] = pr_ref
    V["rp_dpd"].reshape(6, 4)[3:, 0] = om
    V["rp_dpd"].reshape(6, 4)[:3, 0] = case["dp"]
    V["rp_pd"].reshape(6, 4)[3:, 0] = case["pd_r"]
    V["rp_phi_switch"][0] = phi0
    assert V["rp_sector"][0] == 0 and V["sw"][0] == 0 and V["has_prev"][0] == 0


def plant(N, x0, V, case):
    """The solution loop_finish is given: the cold start, with the stage-1 position moved along the path so that opt_phi[1] comes out
    as the wanted path parameter."""
    x = np.array(x0, float)
    pd, dpd = V["rp_pd"].reshape(6, 4), V["rp_dpd"].reshape(6, 4)
    phi0, phi1 = case["fin"][3], case["fin"][4]
    for c in range(3):
        x[28 * N + c * N + 1] = pd[c, 0] + (phi1 - phi0) * dpd[c, 0]
    return x


def check_prepare_one(W, case, V0, V1, p, R_ee, left_out):
    """One rollout after loop_prepare: V0 the state before (what the block read), V1 after, p the 875 parameters."""
    pr = np.array(V1["p_lie"][3:6])
    W.add("p_lie/" + case["qfam"], rot_dist(pr, R_ee), extra=4 * defect(R_ee), what=f"angle {float(angle(R_ee)):.12f}")
    assert np.linalg.norm(pr) <= float(PI) * (1 + 4 * EPS)
    f4 = lambda name: np.array(V1[name]).reshape(4, 3)
    dtau, par, o1, o2 = f4("dtau"), f4("dtau_par"), f4("dtau_o1"), f4("dtau_o2")
    vs = [np.array(V1[n]).reshape(3, 4) for n in ("v1", "v2", "v3")]
    for i in range(4):
        prs = np.array(V0["pr_ref"]) if i == 0 else np.array(V0["rp_r_taud"]).reshape(3, 4)[:, i]
        dpn, br1, br2 = (np.array(V0["rp_dpdn"]).reshape(3, 4)[:, i], np.array(V0["rp_br1"]).reshape(-1, 3)[i],
                         np.array(V0["rp_br2"]).reshape(-1, 3)[i])
        fam = fam_of(case["tags"][i])
        ref = check_initial_errors_one(W, fam, (dtau[i], par[i], o1[i], o2[i]), pr, prs, dpn, br1, br2)
        assert ref["locked"] == (fam == "lock"), (case["tags"][i], ref["lock_distance"])
        # the dual basis of this stage's own inputs: dtau of segment 0 and this segment's split, as the state holds them
        cands, cond = dual_basis(dtau[0], o1[i], par[i], br1, dpn, br2)
        random_family = case["kind"] == "random" or "random" in case["tags"][i] or "random" in case["tags"][0]
        left_out["random" if random_family else "structured"][1] += 1
        if not cond <= COND_MAX:
            left_out["random" if random_family else "structured"][0] += 1
            if not random_family:
                assert about_path_direction(case["tags"][0]) or about_path_direction(case["tags"][i]), (case["tags"], cond)
            continue
        Vk = ld([v[:, i] for v in vs])
        dev, delta = min((float(np.abs(Vk - V).max()), float(np.abs(Vk @ B - np.eye(3)).max())) for V, B in cands)
        vmax = float(np.abs(cands[0][0]).max())
        # (1 + cos a) / sin a of the Jacobian formula cancels next to a half turn, on the host as on the device: a family of its own
        rest1 = exp(dtau[0]) @ exp(o1[i]).T
        near_half = max(float(angle(exp(dtau[0]))), float(angle(rest1)), float(angle(rest1 @ exp(par[i]).T))) > float(PI) - 2e-3
        dfam = "half" if near_half else ("mid" if fam in ("small", "half", "pi_outer") else fam)
        W.add("dual/" + dfam, dev, scale=cond ** 2 * vmax, what=f"cond {cond:.2f}")
        W.add("dual/" + dfam, delta, scale=cond ** 2 * vmax * float(np.abs(cands[0][1]).max()), what=f"v . (g h k), cond {cond:.2f}")
    a0 = float(np.linalg.norm(dtau[0]))
    for name, sign in (("jac_r", +1), ("jac_l", -1)):
        W.add("jac/" + fam_angle(a0), np.abs(ld(np.array(V1[name]).reshape(3, 3)) - jac_inv_formula(dtau[0], sign)).max(),
              scale=1 + a0 * a0, what=name)
    # the parameter rows hold the same numbers, transposed where loop_prepare transposes
    if p is None:
        return
    row = lambda n: p[P_OFF[n][0]:P_OFF[n][0] + P_OFF[n][1]]
    for n in ("dtau", "dtau_par", "dtau_o1", "dtau_o2", "v1", "v2", "v3"):
        assert (row(n) == np.array(V1[n])).all(), n
    for n in ("jac_r", "jac_l"):
        assert (row(n).reshape(3, 3) == np.array(V1[n]).reshape(3, 3).T).all(), n
    assert (row("iw_ref") == np.array(V0["iw_ref"])).all() and (row("dpn") == np.array(V0["rp_dpdn"])).all()
    for n in ("br1", "br2"):
        assert (row(n).reshape(3, 4) == np.array(V0["rp_" + n]).reshape(-1, 3)[:4].T).all(), n


def check_finish_one(W, case, V1, V2):
    """One rollout after loop_finish: V1 the state loop_finish was given, V2 after."""
    fam, pr_ref, om, phi0, phi1 = case["fin"]
    phi = float(V2["phi_current"][0])
    assert abs(phi - phi1) <= 16 * EPS * max(1.0, abs(phi1)), (phi, phi1)
    check_integrate_one(W, fam, V2["pr_ref"], pr_ref, om, LD(phi) - LD(phi0))
    iw = ld(case["pd_r"]) + (LD(phi) - LD(phi0)) * ld(om)
    W.add("iw_ref/all", np.abs(ld(np.array(V2["iw_ref"])) - iw).max(), scale=max(1.0, float(np.abs(iw).max())))


def about_path_direction(tag):
    """A rotation by 2 rad or more about the path direction of the trivial frame.  Its Euler split has both outer angles at a half
    turn, rest1 is a half turn, and [g h k] is singular or close to it by construction (at angle pi, g = pi/2 br2 is parallel to
    k = br2): cond([g h k]) is 1e3 to 1e14 there, on the host mirror, the reference and the device alike."""
    kind, *rest = tag.split(":")
    return kind == "angle" and rest[1] == "y" and float(rest[0]) >= 2.0


def check_left_out(left_out):
    """A random family leaves at most 1 % out of the dual basis' check (cond > COND_MAX); of the structured families only segments
    that see a rotation by 2 rad or more about the path direction may be left out (asserted where they are), and most are kept."""
    assert left_out["structured"][0] <= 0.1 * left_out["structured"][1] and left_out["structured"][1] > 0, left_out
    assert left_out["random"][0] <= 0.01 * left_out["random"][1] and left_out["random"][1] > 0, left_out
