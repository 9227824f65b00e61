"""The closest pair between a segment and an obstacle polytope, and the greedy separating halfspaces built on it, stated
independently of the product -- TEST INFRASTRUCTURE ONLY.  numpy and scipy; nothing of boundplanner_amd/collision_sets.py or of the
C++ sources is used here.

The QP (ConvexSetFinder.py:52-99, 491-510):   min |p0 + phi (p1 - p0) - x|^2   s.t.  A x <= b - 0.001,  0 <= phi <= 1.

exact_pairs() solves it exactly:
  * the segment is clipped against the shrunk polytope (Cyrus-Beck in np.longdouble); where a piece is left the distance is 0 and
    the case is `through`;
  * otherwise the active sets are enumerated: every set of at most three rows that meet in a vertex of the polytope (the rows with a
    positive multiplier at x* are active at x*, three of them suffice, and a face that holds x* holds a vertex), each with phi at 0,
    at 1 and free.  The KKT system of every candidate is solved in double (minimum-norm solution, so that a flat minimum and a
    duplicated row do no harm), the nearest candidate that is feasible with multipliers of the right sign is refined in
    np.longdouble until it stalls and then has to pass the KKT conditions in np.longdouble at 1e-15.  Every case gets an answer or
    the library raises.
  * d* = |x* - y*|, s* = x* - y* (unique: the QP is strictly convex in it; x* and phi* need not be), a* = s* / d*,
    bh* = a*.x* - 0.001, and the class of the closest feature: face / edge / vertex (1, 2, 3 rows with a positive multiplier),
    phi at 0, at 1 or inside, and whether the minimum is flat (the segment parallel to all of those rows, so that the pair may slide:
    only s and d are defined).

certificate() trusts no hand-written QP code: for a returned (x, y, dist) it reports the infeasibility of x relative to |a_i|, how
far y is from the segment, |dist - |y - x||, and the duality gap dist - (min(n.p0, n.p1) - max{n.z : A z <= b - 0.001}) with
n = (y - x) / dist and the maximum from scipy.optimize.linprog (highs): a lower bound on the distance of ANY pair.  The bound is
sharp only for the exact direction n*: where the segment or the obstacle can pivot about the closest pair it falls off in first
order, by at most |n - n*| (|p1 - p0| + diameter of the obstacle) with |n - n*| <= 2 |s - s*| / d*.  The figure that is measured and
bounded is therefore gap x d* / (|p1 - p0| + diameter + d*), which is of the size of |s - s*|.

Bounds on the rows that follow from the bound on s.  With e = |s - s*| and d* the exact distance: a = s / |s| gives
|a - a*| <= 2 e / d* (normalising a vector moves it by at most twice its relative error).  bh = a.x - 0.001 with
|a.x - a*.x*| <= |a - a*| |x| + |a*.(x - x*)|; a* separates, so a*.x >= a*.x* - feas for a point x that is feasible to feas, and
a*.x = a*.y + a*.s <= a*.y* + a*.s* + e = a*.x* + e; hence |bh - bh*| <= |a - a*| EXTENT + e + feas, EXTENT bounding |x| over the
scene.

replay() runs the greedy selection (ConvexSetFinder.py:330-375) on the exact pairs: nearest first, first index on ties, obstacles
with min_v a.v - bh >= -1e-4 dropped, the touching fall-backs, overflow at the caller's capacity.  A comparison whose margin is below
the bound on the compared quantity (two distances closer than 2 x the distance bound, a min_v within the row bound of -1e-4) makes
the case undecidable; it is then left out, and the callers cap the share of such cases at MAX_LEFT_OUT."""
import itertools

import numpy as np
from scipy.optimize import linprog

LD = np.longdouble
SHRINK = 0.001
FACTOR = 32.0                       # the kernels -- emulated and on the GPU -- get 32 x the host's measured worst
CAP = 1e-7                          # nothing may exceed this in distance or s [m] (tests/test_device_loop_scenes_gpu.py)
ROW_TOL_FAR = 1e-6                  # rows away from flat minima at d* >= FAR (the project's tolerance against the reference's finder)
FAR = 0.05
MAX_LEFT_OUT = 0.02
EXTENT = 2.0                        # |x| over every scene of the cases below [m]
# Worst deviations of the host statement as built for the CPU (emu_closest_pair: the device source compiled by g++) from the exact
# reference over the orthogonal-row cases (axis-aligned, rotated and scaled boxes: there the code was converged before the
# projection became a KKT solve), rounded up.  feas: max(A x - b + 0.001) / |a_i|; gap: the certificate's duality gap, scaled as the
# docstring says; dist, s: against d*, s* [m].
# Measured: feas 1.43e-16, gap 6.17e-10, dist 9.06e-14 (the golden section leaves phi at 1e-8: second order in the distance, first
# order in s), s 5.20e-9.
HOST_WORST = dict(feas=1.5e-16, gap=6.5e-10, dist=9.6e-14, s=5.5e-9)
BOUND = {k: min(FACTOR * v, CAP) for k, v in HOST_WORST.items()}


def check_longdouble():
    assert np.finfo(LD).eps < 2e-19, "np.longdouble is not the 80-bit extended format here"


# ---------------------------------------------------------------------------------------------------------------------------------
# polytopes
# ---------------------------------------------------------------------------------------------------------------------------------
def vertices_of(A, b, tol=1e-9):
    """(vertices [n][3], active rows of each vertex) of {A x <= b} by intersecting row triples."""
    A, b = np.asarray(A, float), np.asarray(b, float)
    nrm = np.linalg.norm(A, axis=1)
    V, act = [], []
    for t in itertools.combinations(range(len(b)), 3):
        M = A[list(t)]
        if abs(np.linalg.det(M / nrm[list(t), None])) < 1e-9:
            continue
        v = np.linalg.solve(M, b[list(t)])
        if np.all((A @ v - b) / nrm <= tol) and not any(np.linalg.norm(v - w) < 1e-7 for w in V):
            V.append(v)
            act.append(tuple(np.flatnonzero(np.abs(A @ v - b) / nrm <= 1e-7)))
    return np.array(V), act


def inradius(A, b, centre=False):
    """radius (and centre) of the largest ball in {A x <= b - SHRINK}"""
    A, b = np.asarray(A, float), np.asarray(b, float)
    r = linprog([0, 0, 0, -1.0], A_ub=np.hstack((A, np.linalg.norm(A, axis=1)[:, None])), b_ub=b - SHRINK, bounds=[(None, None)] * 4, method="highs")
    assert r.status == 0
    return (-r.fun, r.x[:3]) if centre else -r.fun


class Poly:
    """An obstacle: rows A x <= b, the vertex array handed to the product (pts), the family's name; for the reference the vertices
    of the SHRUNK polytope with their active rows, and the candidate active sets."""

    def __init__(self, name, A, b, extra_pts=None, orthogonal=False):
        self.name, self.A, self.b, self.orthogonal = name, np.ascontiguousarray(A, float), np.ascontiguousarray(b, float), orthogonal
        self.pts, _ = vertices_of(self.A, self.b)
        if extra_pts is not None:
            self.pts = np.vstack((self.pts, extra_pts))
        self.V, self.act = vertices_of(self.A, self.b - SHRINK)
        assert len(self.A) <= 15 and 4 <= len(self.pts) <= 32 and len(self.V) >= 4, (name, len(self.A), len(self.pts))
        sets = {()}
        for a in self.act:
            for m in (1, 2, 3):
                sets.update(itertools.combinations(a, m))
        self.sets = sorted(sets, key=lambda s: (len(s), s))
        self.centre = self.V.mean(axis=0)
        self.inrad, self.inner = inradius(self.A, self.b, centre=True)
        self.size = np.linalg.norm(self.V - self.centre, axis=1).max()

    def moved(self, Q, t, name=None):
        """the polytope turned by Q and moved by t"""
        p = Poly.__new__(Poly)
        p.__dict__.update(self.__dict__)
        p.name = name or self.name
        p.A = np.ascontiguousarray(self.A @ Q.T)
        p.b = self.b + p.A @ t
        p.pts, p.V, p.centre, p.inner = self.pts @ Q.T + t, self.V @ Q.T + t, Q @ self.centre + t, Q @ self.inner + t
        return p

    def as_set(self):
        return [self.A, self.b]


def _rot(rng):
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(rng.normal(size=3) * 1.5).as_matrix()


def _from_points(name, P, **kw):
    from scipy.spatial import ConvexHull
    h = ConvexHull(P)
    eq = np.unique(np.round(h.equations, 12), axis=0)
    return Poly(name, eq[:, :3], -eq[:, 3], **kw)


def wedge(deg, L, depth=0.1):
    """triangular prism: two long faces meet at the interior angle `deg` along the edge x = y = 0, legs of length L, closed by the
    face opposite to the edge and two end caps at z = +- depth / 2 (5 rows, 6 vertices)"""
    h = np.radians(deg) / 2
    n1, n2 = np.array([-np.sin(h), np.cos(h), 0.0]), np.array([-np.sin(h), -np.cos(h), 0.0])
    A = np.array([n1, n2, [1.0, 0, 0], [0, 0, 1.0], [0, 0, -1.0]])
    return Poly(f"wedge{deg:g}", A, np.array([0.0, 0.0, L * np.cos(h), depth / 2, depth / 2]))


def families(seed=11):
    """The obstacle shapes of the issue, centred near the origin: name -> list of Poly.  Shrunk inradius >= 5 mm, sizes 0.05 .. 0.4 m."""
    rng = np.random.default_rng(seed)
    box = lambda h: (np.vstack((np.eye(3), -np.eye(3))), np.concatenate((h, h)))
    F = {}
    A, b = box(np.array([0.06, 0.1, 0.04]))
    F["axis_box"] = [Poly("axis_box", A, b, orthogonal=True)]
    F["rot_box"] = [Poly("rot_box", A, b, orthogonal=True).moved(_rot(rng), np.zeros(3))]
    S = np.array([[1.0, 0.9, 0.4], [0.0, 1.0, 0.7], [0.0, 0.0, 1.0]])           # x = S u: rows A S^-1
    F["sheared_box"] = [Poly("sheared_box", A @ np.linalg.inv(S), b)]
    tets = []
    while len(tets) < 6:                      # random tetrahedra; the later ones are slivers (one vertex pressed towards the opposite face)
        P = rng.normal(size=(4, 3)) * 0.1
        if len(tets) >= 3:
            n = np.cross(P[1] - P[0], P[2] - P[0]); n /= np.linalg.norm(n)
            P[3] = P[:3].mean(axis=0) + 0.03 * n + 0.02 * rng.normal(size=3)
        t = _from_points("tet_sliver" if len(tets) >= 3 else "tet", P)
        if inradius(t.A, t.b) >= 0.005 and t.size <= 0.4:
            tets.append(t)
    F["tet"], F["tet_sliver"] = tets[:3], tets[3:]
    for deg in (30, 10, 6, 4, 2):
        F[f"wedge{deg}"] = [wedge(deg, 0.4 if deg <= 6 else 0.2)]
    base = 0.04 * np.array([[1, 1, 0], [1, -1, 0], [-1, -1, 0], [-1, 1, 0]], float)
    F["pyramid"] = [_from_points("pyramid", np.vstack((base, [[0, 0, 0.35]])))]
    ang = 2 * np.pi * np.arange(13) / 13
    ring = 0.12 * np.column_stack((np.cos(ang), np.sin(ang)))
    P13 = np.vstack((np.column_stack((ring, np.full(13, -0.05))), np.column_stack((ring, np.full(13, 0.05)))))
    F["prism13"] = [_from_points("prism13", P13)]
    mid = 0.5 * (P13[:6] + P13[13:19])        # six more entries of the vertex array, on the prism's upright edges: 32 in all
    F["pts32"] = [_from_points("pts32", P13, extra_pts=mid)]
    Ar, br = F["rot_box"][0].A, F["rot_box"][0].b
    F["dup_redundant"] = [Poly("dup_redundant", np.vstack((Ar, Ar[0], Ar[1] + 0.3 * Ar[2])), np.concatenate((br, [br[0], br[1] + 0.3 * br[2] + 0.05])),
                               orthogonal=False)]
    sc = np.array([0.1, 10.0, 0.1, 1.0, 10.0, 0.1])
    F["scaled_box"] = [Poly("scaled_box", Ar * sc[:, None], br * sc, orthogonal=True)]
    w = wedge(10, 0.2)
    F["scaled_wedge"] = [Poly("scaled_wedge", w.A * sc[:5, None], w.b * sc[:5])]
    for name, ps in F.items():
        for p in ps:
            assert inradius(p.A, p.b) >= 0.005 and 0.05 <= 2 * p.size <= 0.85, (name, inradius(p.A, p.b), p.size)
    assert len(F["prism13"][0].A) == 15 and len(F["prism13"][0].pts) == 26 and len(F["pts32"][0].pts) == 32
    return F


SHARP = ("tet_sliver", "wedge6", "wedge4", "wedge2")


# ---------------------------------------------------------------------------------------------------------------------------------
# the exact QP
# ---------------------------------------------------------------------------------------------------------------------------------
def _clip(A, bs, p0, d):
    """Cyrus-Beck: the parameters [t0, t1] of the part of p0 + t d, 0 <= t <= 1, inside {A x <= bs}; None when there is none"""
    t0, t1 = LD(0), LD(1)
    for a, beta in zip(A, bs):
        den, num = a @ d, beta - a @ p0
        if den == 0:
            if num < 0:
                return None
        elif den > 0:
            t1 = min(t1, num / den)
        else:
            t0 = max(t0, num / den)
    return (t0, t1) if t0 <= t1 else None


def _kkt_matrices(poly, d):
    """K [3 states][sets][8][8] and the constraint index table of the candidates: unknowns (x, phi, mu_1..3 of the rows, nu of phi)"""
    ns = len(poly.sets)
    K = np.zeros((3, ns, 8, 8))
    K[:, :, :3, :3] = np.eye(3)
    K[:, :, :3, 3] = -d; K[:, :, 3, :3] = -d
    K[:, :, 3, 3] = d @ d
    for s, W in enumerate(poly.sets):
        for k in range(3):
            if k < len(W):
                K[:, s, 4 + k, :3] = poly.A[W[k]]; K[:, s, :3, 4 + k] = poly.A[W[k]]
            else:
                K[:, s, 4 + k, 4 + k] = 1.0
    K[:2, :, 7, 3] = 1.0; K[:2, :, 3, 7] = 1.0          # states 0, 1: phi = 0, phi = 1
    K[2, :, 7, 7] = 1.0                                 # state 2: phi free
    return K


def exact_pairs(poly, P0, P1):
    """The exact closest pairs of the segments [P0[i], P1[i]] and the obstacle `poly`: list of dicts (see the module's docstring)."""
    check_longdouble()
    A, bs = poly.A.astype(LD), poly.b.astype(LD) - LD(SHRINK)
    nrm = np.linalg.norm(poly.A, axis=1)
    ns = len(poly.sets)
    out = []
    for p0, p1 in zip(np.asarray(P0, float).reshape(-1, 3), np.asarray(P1, float).reshape(-1, 3)):
        d = p1.astype(LD) - p0.astype(LD)
        point = bool(np.all(p0 == p1))
        clip = _clip(A, bs, p0.astype(LD), d)
        if clip is not None:
            depth = max(float(np.min((bs - A @ (p0 + t * d)) / nrm)) for t in (clip[0], 0.5 * (clip[0] + clip[1]), clip[1]))
            out.append(dict(through=True, d=0.0, depth=depth, point=point))
            continue
        dd = np.asarray(d, float)
        K = _kkt_matrices(poly, dd)
        rhs = np.zeros((3, ns, 8))
        rhs[:, :, :3] = p0; rhs[:, :, 3] = -(dd @ p0)
        for s, W in enumerate(poly.sets):
            rhs[:, s, 4:4 + len(W)] = (poly.b - SHRINK)[list(W)]
        rhs[1, :, 7] = 1.0
        states = (0,) if point else (0, 1, 2)
        Kp = np.linalg.pinv(K[list(states)], rcond=1e-13)
        z = np.einsum("tsij,tsj->tsi", Kp, rhs[list(states)])
        x, phi = z[..., :3], z[..., 3]
        y = p0 + phi[..., None] * dd
        dist = np.linalg.norm(x - y, axis=-1)
        # the double solve only screens (a sliver's edge nearly parallel to the segment has a condition of 1e8): 1e-6 here, the
        # KKT conditions at 1e-15 after the refinement
        scr = 1e-6
        ok = np.all((x @ poly.A.T - (poly.b - SHRINK)) / nrm <= scr, axis=-1) & np.all(z[..., 4:7] >= -scr, axis=-1)
        ok &= (phi >= -scr) & (phi <= 1 + scr)
        res = np.linalg.norm(np.einsum("tsij,tsj->tsi", K[list(states)], z) - rhs[list(states)], axis=-1)
        ok &= res <= scr
        for k, t in enumerate(states):      # nu is the multiplier of phi = c: the objective may not fall towards the inside of [0, 1]
            if t == 0:
                ok[k] &= z[k, :, 7] <= scr
            if t == 1:
                ok[k] &= z[k, :, 7] >= -scr
        best = None
        for k, s in sorted(zip(*np.nonzero(ok)), key=lambda ks: dist[ks]):
            r = _refine(K[states[k], s], Kp[k, s], rhs[states[k], s].astype(LD), z[k, s].astype(LD), poly, states[k], s, p0, d, A, bs, nrm)
            if r is not None:
                best = r
                break
        assert best is not None, f"{poly.name}: no KKT point for the segment {p0} {p1}"
        out.append(best)
    return out


def _refine(K, Kp, rhs, z, poly, state, s, p0, d, A, bs, nrm):
    """iterative refinement of one candidate in longdouble, then the KKT conditions at 1e-15"""
    # the right-hand side in longdouble: p0, -d.p0 and b - 0.001 carry digits past double
    W = poly.sets[s]
    rhs = rhs.copy()
    rhs[3] = -(d @ p0.astype(LD))
    for k, w in enumerate(W):
        rhs[4 + k] = bs[w]
    KL = K.astype(LD)
    KL[:3, 3] = -d; KL[3, :3] = -d; KL[3, 3] = d @ d
    last = np.inf
    for _ in range(8):
        r = rhs - KL @ z
        nr = float(np.abs(r).max())
        if nr >= last:
            break
        last = nr
        z = z + Kp.astype(LD) @ r
    x, phi, mu, nu = z[:3], z[3], z[4:4 + len(W)], z[7]
    y = p0 + phi * d
    sv = x - y
    dist = np.sqrt(sv @ sv)
    tol = LD(1e-15)
    if np.any((A @ x - bs) / nrm > tol) or np.any(mu * nrm[list(W)] < -tol) or phi < -tol or phi > 1 + tol:
        return None
    # stationarity: x - y + A_W^T mu = 0, and the slope along the segment
    if np.abs(sv + A[list(W)].T @ mu).max() > tol if len(W) else np.abs(sv).max() > tol:
        return None
    slope = -(d @ sv)                      # d/dphi of 0.5 |y - x|^2
    scale = max(float(np.sqrt(d @ d)), 1e-300)
    if (state == 0 and slope < -tol * scale) or (state == 1 and slope > tol * scale) or (state == 2 and abs(slope) > tol * scale):
        return None
    if not dist > 0:
        return None
    ph = float(phi)
    pcls = "0" if (state == 0 or ph <= 1e-12) else "1" if (state == 1 or ph >= 1 - 1e-12) else "in"
    # the feature: the rows that push (positive multiplier); flat: the segment runs parallel to all of them, so that the pair may slide
    Wp = np.array([w for w, m in zip(W, mu) if m * nrm[w] > 1e-9 * dist], int)
    n_act = len(Wp)
    flat = bool(scale >= 1e-12 and n_act and np.all(np.abs(np.asarray(A[Wp] @ d, float)) <= 1e-9 * nrm[Wp] * scale))
    a = sv / dist
    return dict(through=False, d=float(dist), s=np.asarray(sv, float), a=np.asarray(a, float), bh=float(a @ x - LD(SHRINK)), x=np.asarray(x, float),
                y=np.asarray(y, float), phi=ph, feature={1: "face", 2: "edge"}.get(n_act, "vertex"), phi_class=pcls, flat=flat, point=False,
                s_ld=sv, x_ld=x, y_ld=y, d_ld=dist)


# ---------------------------------------------------------------------------------------------------------------------------------
# the certificate
# ---------------------------------------------------------------------------------------------------------------------------------
def certificate(A, b, p0, p1, x, y, dist):
    """dict(feas, seg, norm, gap) for a claimed closest pair (x in the polytope, y on the segment, distance dist > 0)"""
    A, b = np.asarray(A, float), np.asarray(b, float)
    x, y, p0, p1 = (np.asarray(v, LD) for v in (x, y, p0, p1))
    nrm = np.linalg.norm(A, axis=1)
    feas = float(np.max((A.astype(LD) @ x - (b.astype(LD) - LD(SHRINK))) / nrm))
    d = p1 - p0
    dd = d @ d
    t = min(max((y - p0) @ d / dd, LD(0)), LD(1)) if dd > 0 else LD(0)
    seg = float(np.abs(y - (p0 + t * d)).max())
    if not (y - x) @ (y - x) > 0:           # no direction to certify with (the cases are clear by 1e-4 at least): no bound at all
        return dict(feas=feas, seg=seg, norm=float(abs(LD(dist))), gap=float("inf"))
    n = (y - x) / np.sqrt((y - x) @ (y - x))
    r = linprog(-np.asarray(n, float), A_ub=A, b_ub=b - SHRINK, bounds=[(None, None)] * 3, method="highs")
    assert r.status == 0, r.message
    z = r.x.astype(LD)                      # the LP's vertex; its value is recomputed in longdouble
    lower = min(n @ p0, n @ p1) - n @ z
    return dict(feas=feas, seg=seg, norm=float(abs(LD(dist) - np.sqrt((y - x) @ (y - x)))), gap=float(LD(dist) - lower))


# ---------------------------------------------------------------------------------------------------------------------------------
# the greedy selection on the exact pairs
# ---------------------------------------------------------------------------------------------------------------------------------
def row_bounds(E, e_s=None, feas=None):
    """(bound on |a - a*|, bound on |bh - bh*|) of the row of the exact pair E when s is within e_s of s*"""
    e_s = BOUND["s"] if e_s is None else e_s
    feas = BOUND["feas"] if feas is None else feas
    ea = 2 * e_s / E["d"]
    return ea, ea * EXTENT + e_s + feas


def replay(polys, pairs, p0, p1, cap):
    """The greedy selection on the exact pairs of one segment with the obstacles `polys`.
    Returns dict(rows=[(a*, bh*, pair)], overflow, touched, decidable)."""
    remain = list(range(len(polys)))
    rows, touched, decidable, overflow = [], False, True, False
    while remain:
        ds = sorted((pairs[i]["d"], i) for i in remain)
        if len(ds) > 1 and ds[1][0] - ds[0][0] <= 2 * BOUND["dist"]:
            decidable = False
        idx = ds[0][1]
        E = pairs[idx]
        if E["through"]:
            touched = True
            rows.append((None, None, E))          # the offsets of a touching row are undetermined (expected_set_params)
            # what it drops cannot be replayed either: a scene with a touched obstacle counts rows only when it is the last one
            remain = [i for i in remain if i != idx]
            if remain:
                decidable = False
            if len(rows) > cap - 6:
                overflow = True
            continue
        a, bh = E["a"], E["bh"]
        ea, eb = row_bounds(E)
        keep = []
        for i in remain:
            if i == idx:
                continue
            mn = float(np.min(polys[i].pts @ a - bh))
            if abs(mn + 1e-4) <= ea * EXTENT + eb:
                decidable = False
            if mn < -1e-4:
                keep.append(i)
        remain = keep
        rows.append((a, bh, E))
        if len(rows) > cap - 6:
            overflow = True
    return dict(rows=rows, overflow=overflow, touched=touched, decidable=decidable)


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
def segments_around(poly, rng, n, length_all=None):
    """n segments placed so that the classes of the issue occur around `poly`: closest feature a face / an edge / a vertex, phi at
    0, at 1 and inside, parallel to a face and to an edge, lengths 0 (p0 == p1), 1e-13, ~0.05 and ~0.6, clear by >= 1e-4 or through
    by >= 5 mm.  What class a segment is in is decided by the reference afterwards, not here.  length_all: every segment has this length
    (0: single points), for callers whose segments are given and who move the obstacle instead."""
    A, nrm = poly.A, np.linalg.norm(poly.A, axis=1)
    P0, P1 = [], []
    unit = lambda v: v / np.linalg.norm(v)
    k = 0
    while len(P0) < n:
        k += 1
        kind = k % 10 if length_all is None else (0 if length_all == 0 else (2, 3, 4, 5, 6, 7, 8, 9)[k % 8])
        v = int(rng.integers(len(poly.V)))
        rows = list(poly.act[v])
        m = (1, 2, 3)[k % 3]
        W = list(rng.choice(rows, size=min(m, len(rows)), replace=False))
        # a point of the feature spanned by W: the vertex pulled towards the other vertices of that feature
        on = [j for j, a in enumerate(poly.act) if set(W) <= set(a)]
        w = rng.dirichlet(np.ones(len(on)))
        t = (poly.V[on] * w[:, None]).sum(axis=0)
        nv = unit((A[W] / nrm[W, None] * rng.uniform(0.2, 1.0, size=(len(W), 1))).sum(axis=0))
        gap = float(10 ** rng.uniform(-3.5, -0.5))
        ystar = t + gap * nv
        length = (0.05, 0.6)[(k // 10) % 2] * rng.uniform(0.8, 1.2) if length_all is None else length_all
        perp = unit(np.cross(nv, rng.normal(size=3)))
        if kind == 0:                                   # a single point
            p0 = p1 = ystar
        elif kind == 1:                                 # shorter than the 1e-12 switch
            p0, p1 = ystar, ystar + 1e-13 * unit(rng.normal(size=3))
        elif kind == 2:                                 # phi = 0: leaves away from the obstacle
            p0, p1 = ystar, ystar + length * unit(nv + 0.8 * perp)
        elif kind == 3:                                 # phi = 1
            p0, p1 = ystar + length * unit(nv + 0.8 * perp), ystar
        elif kind == 4 and len(W) == 1:                 # parallel to a face
            dv = unit(np.cross(A[W[0]], rng.normal(size=3)))
            p0, p1 = ystar - 0.3 * length * dv, ystar + 0.7 * length * dv
        elif kind == 5 and len(W) >= 2 and np.linalg.norm(np.cross(A[W[0]], A[W[1]])) > 1e-6 * nrm[W[0]] * nrm[W[1]]:     # parallel to an edge
            dv = unit(np.cross(A[W[0]], A[W[1]]))
            p0, p1 = ystar - 0.3 * length * dv, ystar + 0.7 * length * dv
        elif kind == 6:                                 # through the obstacle
            c = poly.inner + 0.05 * poly.inrad * unit(rng.normal(size=3))
            dv = unit(rng.normal(size=3))
            p0, p1 = c - 0.5 * length * dv, c + 0.5 * length * dv
        else:                                           # phi inside: passes by
            f = rng.uniform(0.2, 0.8)
            p0, p1 = ystar - f * length * perp, ystar + (1 - f) * length * perp
        P0.append(np.array(p0, float)); P1.append(np.array(p1, float))
    return np.array(P0), np.array(P1)


def place_at(poly, q0, q1, rng):
    """`poly` turned and moved so that the given segment [q0, q1] lies around it the way one of segments_around's does (an
    axis-aligned box is only moved: it has to stay one)"""
    L = float(np.linalg.norm(q1 - q0))
    g0, g1 = segments_around(poly, rng, 1 + int(rng.integers(8)), length_all=L if L >= 1e-12 else 0.0)
    g0, g1 = g0[-1], g1[-1]
    Q = np.eye(3)
    if poly.name != "axis_box" and L >= 1e-12:
        from scipy.spatial.transform import Rotation
        u, v = (g1 - g0) / np.linalg.norm(g1 - g0), (q1 - q0) / L
        Q0 = Rotation.align_vectors(v[None], u[None])[0].as_matrix()
        Q = Rotation.from_rotvec(v * rng.uniform(0, 2 * np.pi)).as_matrix() @ Q0
    elif poly.name != "axis_box":
        Q = _rot(rng)
    return poly.moved(Q, q0 - Q @ g0)


def admissible(E):
    """the cases the issue leaves out: exact distances in (0, 1e-4), a through case shallower than 5 mm, a single point inside"""
    if E["through"]:
        return E["depth"] >= 0.005 and not E["point"]
    return E["d"] >= 1e-4


def single_cases(seed=5, per_poly=48):
    """[(family, Poly, P0, P1, exact pairs)]: every polytope of families() turned and moved into the workspace, with per_poly admissible
    segments around it"""
    rng = np.random.default_rng(seed)
    out = []
    for fam, polys in families().items():
        for poly in polys:
            p = poly if fam == "axis_box" else poly.moved(_rot(rng) if fam != "rot_box" else np.eye(3), np.zeros(3))
            p = p.moved(np.eye(3), rng.uniform([-0.5, -0.5, 0.2], [0.5, 0.5, 0.9]))
            P0, P1, EX = [], [], []
            while len(P0) < per_poly:
                a0, a1 = segments_around(p, rng, per_poly)
                for q0, q1, E in zip(a0, a1, exact_pairs(p, a0, a1)):
                    if admissible(E) and len(P0) < per_poly:
                        P0.append(q0); P1.append(q1); EX.append(E)
            out.append((fam, p, np.array(P0), np.array(P1), EX))
    return out


def classes_of(EX, P0, P1):
    """which of the issue's classes occur among the exact pairs EX"""
    c = dict.fromkeys(("through", "face", "edge", "vertex", "phi0", "phi1", "phi_in", "flat_face", "flat_edge", "point", "tiny", "short", "long"), 0)
    for E, p0, p1 in zip(EX, P0, P1):
        L = np.linalg.norm(p1 - p0)
        c["point"] += L == 0; c["tiny"] += 0 < L < 1e-12; c["short"] += 0.03 < L < 0.07; c["long"] += L > 0.45
        if E["through"]:
            c["through"] += 1
            continue
        c[E["feature"]] += 1
        c[{"0": "phi0", "1": "phi1", "in": "phi_in"}[E["phi_class"]]] += 1
        if E["flat"]:
            c["flat_" + ("face" if E["feature"] == "face" else "edge")] += 1
    return c


def multi_scenes(seed=9, max_obs=16):
    """8 scenes of 2 .. max_obs polytopes of every family: scattered through the workspace, and two sphere arrangements (every
    obstacle needs a halfspace of its own: more rows than the capacity), as in tests/test_segment_rows.py.
    [(polys, centre or None)]"""
    rng = np.random.default_rng(seed)
    pool = [p for ps in families().values() for p in ps]
    counts = [2, 3, 5, 8, 12, max_obs, 12, max_obs]
    out = []
    for k, n in enumerate(counts):
        polys = []
        centre = rng.uniform([-0.3, -0.3, 0.4], [0.3, 0.3, 0.8]) if k >= 6 else None
        for j in range(n):
            base = pool[(3 * k + j) % len(pool)]
            Q = np.eye(3) if base.name == "axis_box" else _rot(rng)
            if centre is None:
                t = rng.uniform([-0.7, -0.7, 0.0], [0.7, 0.7, 1.1])
            else:
                dv = rng.normal(size=3)
                t = centre + (0.45 + base.size) * dv / np.linalg.norm(dv)
            polys.append(base.moved(Q, t - Q @ base.centre))
        out.append((polys, centre))
    return out


def scene_segments(polys, centre, rng, n):
    """n admissible segments for a scene: anywhere in the workspace, or starting near the sphere's centre"""
    P0, P1 = [], []
    while len(P0) < n:
        p0 = rng.uniform([-0.7, -0.7, 0.0], [0.7, 0.7, 1.1]) if centre is None else centre + 0.01 * rng.normal(size=3)
        dv = rng.normal(size=3)
        L = (0.0, 0.05, 0.6)[len(P0) % 3] * rng.uniform(0.8, 1.2)
        p1 = p0 + L * dv / np.linalg.norm(dv)
        EX = [exact_pairs(p, p0[None], p1[None])[0] for p in polys]
        # (a segment through an obstacle leaves the direction of its row, and with it what the row drops, undetermined: the flag
        # and the row count of such segments are checked on the single-obstacle scenes)
        if all(admissible(E) and not E["through"] for E in EX):
            P0.append(p0); P1.append(p1)
    return np.array(P0), np.array(P1)


# ---------------------------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------------------------
def pair_errors(poly, p0, p1, E, rec):
    """figures of one 8-double record (x, y, dist, phi) against the exact pair E (clear cases)"""
    x, y, dist = np.asarray(rec[:3], LD), np.asarray(rec[3:6], LD), float(rec[6])
    c = certificate(poly.A, poly.b, p0, p1, x, y, dist)
    reach = float(np.linalg.norm(np.asarray(p1, float) - p0)) + 2 * poly.size + E["d"]
    return dict(feas=c["feas"], seg=c["seg"], norm=c["norm"], gap=abs(c["gap"]) * E["d"] / reach, dist=float(abs(LD(dist) - E["d_ld"])),
                s=float(np.sqrt(((x - y - E["s_ld"]) ** 2).sum())))


def check_rows(label, rows_a, rows_b, n, flag, rep, shift=0.0):
    """The rows 6.. a product routine returned (rows_a [.][3], rows_b [.], count n or < 0 on overflow, touched flag) against the replay
    `rep` of a decidable case.  The loop's offsets carry the joint size: bh = rows_b + shift; it has no touched flag: None.  Returns
    the worst |a - a*| / bound, |bh - bh*| / bound."""
    assert flag is None or bool(flag) == rep["touched"], f"{label}: touched {flag}, the reference says {rep['touched']}"
    assert (n < 0) == rep["overflow"], f"{label}: overflow {n < 0}, the reference says {rep['overflow']}"
    if n < 0:
        return 0.0, 0.0
    assert n - 6 == len(rep["rows"]), f"{label}: {n - 6} rows, the reference has {len(rep['rows'])}"
    wa = wb = 0.0
    for k, (a, bh, E) in enumerate(rep["rows"]):
        if a is None:
            continue
        ea, eb = row_bounds(E)
        if E["d"] >= FAR and not E["flat"]:
            ea, eb = min(ea, ROW_TOL_FAR), min(eb, ROW_TOL_FAR)
        da, db = float(np.linalg.norm(rows_a[6 + k] - a)), float(abs(rows_b[6 + k] + shift - bh))
        assert da <= ea and db <= eb, f"{label}: row {6 + k}: |a - a*| = {da:.3g} (bound {ea:.3g}), |bh - bh*| = {db:.3g} (bound {eb:.3g}), d* = {E['d']:.3g}"
        wa, wb = max(wa, da / ea), max(wb, db / eb)
    return wa, wb


def check_single_rows(label, cases, rows_fn, cap, every=1):
    """rows_fn(polys, P0, P1) -> [(n or < 0, A, b, touched or None)] per segment, on single-obstacle cases
    [(family, Poly, P0, P1, exact pairs)]: the one row against the exact pair; a segment through the obstacle gives the flag and 7 rows"""
    wa = wb = 0.0
    n_through = 0
    for fam, p, P0, P1, EX in cases:
        P0, P1, EX = P0[::every], P1[::every], EX[::every]
        for k, (p0, p1, E, (n, a, b, touched)) in enumerate(zip(P0, P1, EX, rows_fn([p], P0, P1))):
            rep = replay([p], [E], p0, p1, cap)
            assert rep["decidable"]
            if E["through"]:
                assert touched in (None, 1, True) and n == 7, f"{label}: {fam} {k}: a segment through the obstacle gives touched {touched}, {n} rows"
                n_through += 1
                continue
            ra, rb = check_rows(f"{label}: {fam} {k}", a, b, n, touched, rep)
            wa, wb = max(wa, ra), max(wb, rb)
    print(f"{label}: single obstacles: worst row / bound: a {wa:.2g}, bh {wb:.2g}; through {n_through}", flush=True)
    return n_through


def scene_cases(seed=21, nseg=12):
    """[(polys, P0, P1, exact pairs [segment][obstacle])] of the 8 multi-obstacle scenes (up to 32 obstacles: the loop takes the
    first 16)"""
    rng = np.random.default_rng(seed)
    out = []
    for polys, centre in multi_scenes(max_obs=32):
        P0, P1 = scene_segments(polys, centre, rng, nseg)
        ex = [exact_pairs(p, P0, P1) for p in polys]
        out.append((polys, P0, P1, [[ex[o][k] for o in range(len(polys))] for k in range(nseg)]))
    return out


def grazing_cases(seed=4):
    """Scenes of two obstacles that decide at the -1e-4 of the dropping rule: the second obstacle reaches in front of the first
    one's halfspace by 0.05 mm (it is dropped: 7 rows) or by 0.15 mm (it needs a row of its own: 8 rows).  Same format as
    scene_cases()."""
    rng = np.random.default_rng(seed)
    F = families()
    out = []
    for first, second in (("rot_box", "tet"), ("wedge4", "pyramid"), ("prism13", "sheared_box")):
        for reach in (0.5e-4, 1.5e-4):
            while True:
                a = F[first][0].moved(_rot(rng), rng.uniform([-0.3, -0.3, 0.3], [0.3, 0.3, 0.8]))
                P0, P1 = segments_around(a, rng, 8)
                E = exact_pairs(a, P0[-1:], P1[-1:])[0]
                if not E["through"] and 0.05 <= E["d"] <= 0.3:        # (far enough for the row bound to be well below 0.05 mm)
                    break
            p0, p1 = P0[-1], P1[-1]
            b = F[second][0].moved(_rot(rng), np.zeros(3))
            side = np.cross(E["a"], rng.normal(size=3))
            b = b.moved(np.eye(3), E["x"] + 0.1 * side / np.linalg.norm(side))
            b = b.moved(np.eye(3), (-reach - float(np.min(b.pts @ E["a"] - E["bh"]))) * E["a"])
            out.append(([a, b], p0[None], p1[None], [[E, exact_pairs(b, p0[None], p1[None])[0]]]))
            assert out[-1][3][0][1]["d"] > E["d"] + 1e-4
    return out


def check_scene_rows(label, scenes, rows_fn, cap, max_obs, every=1, shifts=None):
    """the rows of multi-obstacle scenes [(polys, P0, P1, exact pairs)] against the replay; returns (overflows, most rows of a set)"""
    n_cases = left_out = overflow = most = 0
    wa = wb = 0.0
    for s, (polys, P0, P1, EX) in enumerate(scenes):
        polys, P0, P1, EX = polys[:max_obs], P0[::every], P1[::every], EX[::every]
        for k, (p0, p1, ex, (n, a, b, touched)) in enumerate(zip(P0, P1, EX, rows_fn(polys, P0, P1))):
            rep = replay(polys, ex[:max_obs], p0, p1, cap)
            n_cases += 1
            if not rep["decidable"]:
                left_out += 1
                continue
            ra, rb = check_rows(f"{label}: scene {s} segment {k}", a, b, n, touched, rep, shift=0.0 if shifts is None else shifts[k])
            wa, wb = max(wa, ra), max(wb, rb)
            overflow += rep["overflow"]
            most = max(most, min(len(rep["rows"]), cap - 6))
    print(f"{label}: scenes: {n_cases} cases, left out {left_out}, overflow {overflow}, most rows {6 + most}; worst row / bound: a {wa:.2g}, bh {wb:.2g}", flush=True)
    assert left_out <= MAX_LEFT_OUT * n_cases, (label, left_out, n_cases)
    return overflow, most


def scene_for_segments(P0, P1, n, rng, sphere=None):
    """n polytopes of every family around given segments (the collision points of an arm): each 0.1 .. 0.5 m from one of the
    segments' ends, or -- sphere: a centre -- on a sphere around it so that each needs a halfspace of its own; every pair clear by
    >= 1e-4.  Returns (polys, exact pairs [segment][obstacle])."""
    pool = [p for ps in families().values() for p in ps]
    polys, ex = [], []
    while len(polys) < n:
        base = pool[int(rng.integers(len(pool)))]
        Q = np.eye(3) if base.name == "axis_box" else _rot(rng)
        dv = rng.normal(size=3); dv /= np.linalg.norm(dv)
        if sphere is None:
            t = P0[int(rng.integers(len(P0)))] + (rng.uniform(0.1, 0.5) + base.size) * dv
        else:
            t = sphere + (0.45 + base.size) * dv
        c = base.moved(Q, t - Q @ base.centre)
        E = exact_pairs(c, P0, P1)
        if all(admissible(e) and not e["through"] for e in E):
            polys.append(c); ex.append(E)
    return polys, [[ex[o][k] for o in range(n)] for k in range(len(P0))]
