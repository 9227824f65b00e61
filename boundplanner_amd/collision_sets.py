"""Per-step convex collision-avoidance sets for the 6 collision points.

Restates ConvexSetFinder.find_set_collision_avoidance(pl, pf, limit_space=True, e_max)
(/root/reference/bound_planner/BoundPlanner/ConvexSetFinder.py:309-375) together with
init_halfspaces_point (:400-421) and compute_set_projs_line (:491-510).

The reference solves, per obstacle polytope {x: A x <= b - 0.001}, the QP
    min_{x, phi in [0,1]} |p0 + phi (p1 - p0) - x|^2   s.t.  A x <= b - 0.001
with qpOASES through CasADi (third-party, not in this image).  Here the same strictly convex
QP in (x, phi) is solved by exact minimisation over phi (1-D convex: golden section on the distance
from the segment point to the polytope), each distance being an exact polytope projection: the KKT
point of an active set that Hildreth's dual coordinate ascent guesses, checked, with an enumeration
of the active sets of size 1..3 behind it (_project_polytope).
"""
import itertools

import numpy as np


def init_halfspaces_point(p, e_max=0.3):
    """Axis-aligned box of half-width e_max around p as 6 halfspaces, ordered +x,-x,+y,-y,+z,-z."""
    a, b = [], []
    for i in range(3):
        e = np.eye(3)[i]
        a.append(e.copy()); b.append(p[i] + e_max)
        a.append(-e); b.append(-p[i] + e_max)
    return a, b


SWEEPS = 100        # Hildreth sweeps for the active-set guess (csrc/bmpc_freespace.hpp: LP_SWEEPS)


def _kkt_point(A, b, rows, y):
    """The KKT point of y on the (1..3) `rows` of {A x <= b} held with equality: x = y - sum lam_k a_k with a_k.x = b_k, one step of
    iterative refinement included.  None unless it is the projection of y: rows independent, lam_k |a_k| >= -1e-12 and
    a_r.x - b_r <= 1e-12 |a_r| for every row (csrc/bmpc_freespace.hpp: lp_kkt_point)."""
    Aw, bw = A[rows], b[rows]
    G = Aw @ Aw.T
    if not np.linalg.det(G) > 1e-12 * np.prod(np.diag(G)):
        return None
    x, lam = y.copy(), np.zeros(len(rows))
    for _ in range(2):
        d = np.linalg.solve(G, Aw @ x - bw)
        lam += d
        x = x - Aw.T @ d
    if np.any(lam * np.sqrt(np.diag(G)) < -1e-12) or np.any(A @ x - b > 1e-12 * np.linalg.norm(A, axis=1)):
        return None
    return x


def _project_polytope(A, b, y):
    """Euclidean projection of y onto {x: A x <= b} (tiny sizes: <= 15 rows).

    The projection is x = y - A_W^T lam with the rows W that hold with equality, lam >= 0.  Hildreth's dual coordinate ascent on
    lam >= 0 only guesses W (the rows it leaves with lam > 0); the answer is the KKT point of those rows in closed form, accepted when
    it is feasible with no negative multiplier, which makes it the projection.  Hildreth's own iterate is never returned: between
    two rows at a sharp angle it converges too slowly to be of use.  Where the guess fails, the active sets of size 1, 2, 3 are
    enumerated; where that finds nothing either, the polytope is empty to rounding: ValueError.  The device states the same in
    csrc/bmpc_freespace.hpp (lp_project_polytope)."""
    if np.all(A @ y - b <= 1e-12):
        return y.copy()
    n = A.shape[0]
    lam = np.zeros(n)
    AAt = A @ A.T
    diag = np.maximum(np.diag(AAt), 1e-16)
    Ay = A @ y
    for _ in range(SWEEPS):
        max_change = 0.0
        for i in range(n):
            r = Ay[i] - AAt[i] @ lam - b[i]
            new = max(0.0, lam[i] + r / diag[i])
            max_change = max(max_change, abs(new - lam[i]))
            lam[i] = new
        if max_change < 1e-13:
            break
    guess = np.flatnonzero(lam > 0.0)
    if 1 <= len(guess) <= 3:
        x = _kkt_point(A, b, guess, y)
        if x is not None:
            return x
    for m in (1, 2, 3):
        for rows in itertools.combinations(range(n), m):
            x = _kkt_point(A, b, list(rows), y)
            if x is not None:
                return x
    raise ValueError("closest pair: the obstacle polytope has no point (empty after the 1 mm shrink)")


def closest_pair_segment_polytope(A, b, p0, p1):
    """argmin over x in polytope, phi in [0,1] of |p0 + phi (p1-p0) - x|.  Returns (x, phi)."""
    d = p1 - p0

    def dist(phi):
        y = p0 + phi * d
        x = _project_polytope(A, b, y)
        return np.linalg.norm(y - x), x

    if np.linalg.norm(d) < 1e-12:
        return dist(0.0)[1], 0.0
    lo, hi = 0.0, 1.0
    gr = (np.sqrt(5.0) - 1.0) / 2.0
    c, e = hi - gr * (hi - lo), lo + gr * (hi - lo)
    fc, fe = dist(c)[0], dist(e)[0]
    for _ in range(80):
        if fc < fe:
            hi, e, fe = e, c, fc
            c = hi - gr * (hi - lo)
            fc = dist(c)[0]
        else:
            lo, c, fc = c, e, fe
            e = lo + gr * (hi - lo)
            fe = dist(e)[0]
    phi = 0.5 * (lo + hi)
    cands = [(dist(ph)[0], ph) for ph in (0.0, 1.0, phi)]
    phi = min(cands)[1]
    return dist(phi)[1], phi


def separating_halfspaces(obs_sets, obs_points_sets, p0, p1):
    """Greedy nearest-first separating halfspaces between the segment [p0, p1] and the obstacles (ConvexSetFinder.py:330-375): the
    nearest obstacle's halfspace through its closest point, shifted by 1 mm; obstacles whose vertices all lie behind it are
    dropped; repeat.  A segment that touches its obstacle falls back to cp - p0, then to p1 - p0.  The one host statement of the
    loop (the device's: csrc/bmpc_freespace.hpp); its callers prepend their own six rows.

    obs_sets: list of [A, b]; obs_points_sets: list of vertex arrays (n_v x 3).
    Returns (rows a (list of [3]), offsets b (list), collision flag)."""
    a_set, b_set = [], []
    collision = False
    remain = list(range(len(obs_sets)))
    pts, closest, dists = {}, {}, {}
    for i in remain:
        A, b = obs_sets[i]
        x, phi = closest_pair_segment_polytope(np.asarray(A), np.asarray(b) - 0.001, p0, p1)
        pts[i] = x
        closest[i] = p0 + phi * (p1 - p0)
        dists[i] = np.linalg.norm(x - closest[i])
    while remain:
        idx = min(remain, key=lambda i: dists[i])
        cp = pts[idx]
        a = cp - closest[idx]
        na = np.linalg.norm(a)
        if na < 1e-6:
            collision = True
            a = cp - p0
            na = np.linalg.norm(a)
            if na < 1e-6:
                a = p1 - p0
                na = np.linalg.norm(a)
        a = a / na
        bh = a @ cp - 0.001
        drop = [idx]
        for i in remain:
            if i != idx and np.min(obs_points_sets[i] @ a - bh) >= -1e-4:
                drop.append(i)
        remain = [i for i in remain if i not in drop]
        a_set.append(a)
        b_set.append(bh)
    return a_set, b_set, collision


def find_set_collision_avoidance(obs_sets, obs_points_sets, p0, p1, e_max=0.3):
    """The per-step set of one collision point: the box of half-width e_max around p0, then the separating halfspaces of the
    segment [p0, p1].  Returns (A (n x 3), b (n), collision flag)."""
    a_set, b_set = init_halfspaces_point(p0, e_max)
    a_sep, b_sep, collision = separating_halfspaces(obs_sets, obs_points_sets, p0, p1)
    return np.array(a_set + a_sep), np.array(b_set + b_sep), collision
