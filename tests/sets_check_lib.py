"""Checks shared by tests/test_convex_sets.py (CPU build of the kernel body) and tests/test_convex_sets_gpu.py (the HIP kernel):
scenes, free seeds, agreement with the host ConvexSetFinder and certificates that do not depend on the host."""
import numpy as np

from boundplanner_amd import scenes
from boundplanner_amd.bound_planner import BoundPlanner


def example_finder():
    boxes = scenes.example_scene()[0]
    return BoundPlanner(obstacles=boxes, e_p_max=0.5, seed=7).set_finder


def random_box_finder(seed, n_boxes=10):
    rng = np.random.default_rng(seed)
    lo = rng.uniform([-0.9, -0.9, 0.0], [0.7, 0.7, 0.9], (n_boxes, 3))
    boxes = np.hstack((lo, lo + rng.uniform(0.05, 0.3, (n_boxes, 3))))
    return BoundPlanner(obstacles=boxes, e_p_max=0.5, seed=7).set_finder


def free_seeds(f, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        s = rng.uniform(f.e_min, f.e_max)
        if all(np.max(a @ s - b) > 1e-3 for a, b in f.obs_sets):
            out.append(s)
    return np.array(out)


def certificates(f, r, k, seed=None, behind_tol=1e-4):
    """Host-independent checks of instance k of a batched result: the set contains `seed`, every obstacle lies behind some row
    (min_v a.v - b >= -behind_tol; the segment sets separate from obstacles shrunk by 1 mm; None: not checked -- a
    segment that touches an obstacle is not separated from it), the ellipsoid is inscribed, the box
    rows are the workspace's."""
    n = int(r["nrows"][k])
    A, b = r["A"][k, :n], r["b"][k, :n]
    assert n >= 6 and np.abs(r["A"][k, n:]).max(initial=0) == 0
    if seed is not None:
        assert (A @ seed - b).max() <= 1e-9
    for a_o, v in zip(f.obs_sets, f.obs_points_sets) if behind_tol is not None else ():
        assert max(np.min(v @ A[i] - b[i]) for i in range(n)) >= -behind_tol
    # the box rows come first and are the workspace's
    assert np.array_equal(A[:6], np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1.0]]))
    assert np.allclose(b[:6], [f.e_max[0], -f.e_min[0], f.e_max[1], -f.e_min[1], f.e_max[2], -f.e_min[2]])
    q = np.linalg.inv(r["q_ellipse"][k])
    L = np.linalg.cholesky(0.5 * (q + q.T))
    c = r["centre"][k]
    assert (np.linalg.norm(A @ L, axis=1) - (b - A @ c)).max() <= 1e-9


def compare_points(f, r, seeds, fixed_mid, optimize=True):
    """Agreement with ConvexSetFinder.find_set_around_point: returns (number of seeds that differ, messages).  Seeds where the host
    raises must carry status 1."""
    bad, msgs = 0, []
    for k, s in enumerate(seeds):
        try:
            A, b, q, c = f.find_set_around_point(s, fixed_mid=fixed_mid, optimize=optimize)
        except RuntimeError as e:
            assert "Ellipse violates" in str(e) and r["status"][k] == 1, (k, str(e), r["status"][k])
            continue
        assert r["status"][k] == 0, (k, r["status"][k])
        n = int(r["nrows"][k])
        same = n == A.shape[0] and np.abs(r["A"][k, :n] - A).max() < 1e-6 and np.abs(r["b"][k, :n] - b).max() < 1e-6 and \
            np.abs(r["q_ellipse"][k] - q).max() <= 1e-6 * max(1.0, np.abs(q).max()) and np.abs(r["centre"][k] - c).max() < 1e-6
        if not same:
            bad += 1
            msgs.append(f"seed {k}: rows {n} vs {A.shape[0]}")
    return bad, msgs


def segments(f, n, seed):
    """Segments (p0 free, p1 = p0 + a random step of up to 0.3 m): some of them touch obstacles."""
    p0 = free_seeds(f, n, seed)
    rng = np.random.default_rng(seed + 1)
    return p0, p0 + rng.uniform(-0.3, 0.3, p0.shape)


def compare_segments(f, r, p0, p1):
    bad, msgs = 0, []
    for k in range(p0.shape[0]):
        A, b, q, c, col = f.find_set_collision_avoidance(p0[k], p1[k], True)
        assert r["status"][k] == 0, (k, r["status"][k])
        n = int(r["nrows"][k])
        same = n == A.shape[0] and np.abs(r["A"][k, :n] - A).max() < 1e-6 and np.abs(r["b"][k, :n] - b).max() < 1e-6 and \
            np.abs(r["q_ellipse"][k] - q).max() <= 1e-6 * max(1.0, np.abs(q).max()) and np.abs(r["centre"][k] - c).max() < 1e-6 and \
            bool(r["collision"][k]) == col
        if not same:
            bad += 1
            msgs.append(f"segment {k}: rows {n} vs {A.shape[0]}, collision {r['collision'][k]} vs {col}")
    return bad, msgs
