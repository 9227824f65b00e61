"""Batched convex free-space sets (boundplanner_amd/csrc/bmpc_sets.hpp) through its CPU build (tests/emu_sets_lib.py): the
ellipsoid-metric projection, the MVIE, the set growth and the segment variant against the host finder
(boundplanner_amd/convex_set_finder.py, planner_opt.py), and the planner with the batched backend against tests/golden/plan.npz."""
import os

import numpy as np
import pytest

import emu_sets_lib as ES
import sets_check_lib as SC
from boundplanner_amd import planner_opt as PO
from boundplanner_amd.bound_planner import BoundPlanner
from boundplanner_amd.convex_set_finder import ConvexSetFinder


def _rand_poly(rng, n):
    A = rng.normal(size=(n, 3)); A /= np.linalg.norm(A, axis=1)[:, None]
    return np.vstack((np.eye(3), -np.eye(3), A)), np.concatenate((np.ones(6), rng.uniform(0.2, 1.0, n)))


def test_projection_is_exact_and_scale_free():
    rng = np.random.default_rng(0)
    n_cmp = 0
    for it in range(200):
        A, b = _rand_poly(rng, int(rng.integers(0, 10)))
        p0 = rng.normal(size=3) * 2
        M = rng.normal(size=(3, 3))
        E = M @ M.T + 0.1 * np.eye(3)
        for scale in (1.0, 1e-4):
            try:
                u = PO.project_polytope(A @ (scale * E), b - A @ p0, np.zeros(3))
            except RuntimeError:        # the host's absolute 1e-10 is below the rounding of a'.u at |u| ~ 1e5
                continue
            want = scale * E @ u + p0
            got = ES.project(A, b, scale * E, p0)
            assert np.abs(got - want).max() < 1e-10 * max(1.0, np.abs(want).max()), (it, scale, got, want)
            n_cmp += 1
    assert n_cmp >= 350


def _mvie_checks(A, b, q, c, qh, ch):
    L = np.linalg.cholesky(q)
    obj = lambda L: 0.25 * np.log(L[0, 0]) + 0.5 * np.log(L[1, 1]) + 0.25 * np.log(L[2, 2])
    Lh = np.linalg.cholesky(qh)
    assert abs(obj(L) - obj(Lh)) <= 1e-8 * max(1.0, abs(obj(Lh)))
    assert np.abs(q - qh).max() < 1e-6 and np.abs(c - ch).max() < 1e-6
    assert (np.linalg.norm(A @ L, axis=1) - (b - A @ c)).max() <= 1e-9


def test_mvie_fixed_and_free_centre():
    rng = np.random.default_rng(1)
    for it in range(40):
        A, b = _rand_poly(rng, int(rng.integers(0, 15)))       # up to 20 rows
        qh, ch = PO.mvie(A, b)
        q, c, st, nw = ES.mvie(A, b, start=np.zeros(3))
        assert st == 0 and nw > 0
        _mvie_checks(A, b, q, c, qh, ch)
        cf = ch + rng.uniform(-0.05, 0.05, 3)
        if (b - A @ cf).min() > 1e-3:
            qh, _ = PO.mvie(A, b, fixed_mid=cf)
            q, c, st, _ = ES.mvie(A, b, fixed_mid=cf)
            assert st == 0 and np.array_equal(c, cf)
            _mvie_checks(A, b, q, c, qh, cf)
    # a fixed centre outside the polytope: status 3 (the host raises)
    A, b = _rand_poly(rng, 4)
    assert ES.mvie(A, b, fixed_mid=np.array([5.0, 0, 0]))[2] == 3


_SCENES = [("example", SC.example_finder, 300, 0)] + [(f"boxes{s}", (lambda s=s: SC.random_box_finder(s)), 50, s) for s in range(1, 5)]


@pytest.mark.parametrize("name,make,n,seed", _SCENES, ids=[s[0] for s in _SCENES])
def test_set_growth_matches_the_host_finder(name, make, n, seed):
    f = make()
    seeds = SC.free_seeds(f, n, 100 + seed)
    for fixed_mid in (True, False):
        r = ES.sets(f.obs_sets, f.obs_points_sets, f.e_min, f.e_max, seeds, fixed_mid=fixed_mid)
        bad, msgs = SC.compare_points(f, r, seeds, fixed_mid)
        print(f"{name} fixed_mid={fixed_mid}: {bad} of {n} seeds differ from the host (near-ties in the greedy order)", msgs[:5])
        assert bad <= 0.01 * n
        for k in np.nonzero(r["status"] == 0)[0]:
            SC.certificates(f, r, k, seed=seeds[k] if fixed_mid else r["centre"][k])
        assert (r["rounds"][r["status"] == 0] >= 1).all() and (r["rounds"] <= 5).all()
    r = ES.sets(f.obs_sets, f.obs_points_sets, f.e_min, f.e_max, seeds[:50], optimize=False)
    bad, _ = SC.compare_points(f, r, seeds[:50], False, optimize=False)
    assert bad == 0 and (r["rounds"] == 1).all()
    assert np.array_equal(r["centre"], seeds[:50]) and np.array_equal(r["q_ellipse"], np.broadcast_to(1e4 * np.eye(3), (50, 3, 3)))


def test_segment_sets_match_the_host_finder():
    f = SC.example_finder()
    p0, p1 = SC.segments(f, 120, 7)
    r = ES.sets(f.obs_sets, f.obs_points_sets, f.e_min, f.e_max, p0, p1)
    bad, msgs = SC.compare_segments(f, r, p0, p1)
    assert bad <= 0.01 * len(p0), msgs
    assert r["collision"].sum() > 0            # some segments touch an obstacle
    assert (r["rounds"] == 1).all()
    for k in range(len(p0)):
        free = not r["collision"][k]
        SC.certificates(f, r, k, seed=None, behind_tol=2e-3 if free else None)


def test_status_codes():
    f = SC.example_finder()
    inside = np.array([0.6, 0.0, -0.05])            # in the table
    with pytest.raises(RuntimeError, match="Ellipse violates"):
        f.find_set_around_point(inside, fixed_mid=True)
    r = ES.sets(f.obs_sets, f.obs_points_sets, f.e_min, f.e_max, [inside, [0.6, 0.1, 0.5]], fixed_mid=True)
    assert r["status"].tolist() == [1, 0] and r["nrows"][0] == 0
    # outside the workspace box: no interior point for the fixed-centre ellipsoid
    r = ES.sets(f.obs_sets, f.obs_points_sets, f.e_min, f.e_max, [[0.0, 0.0, 2.0]], fixed_mid=True)
    assert r["status"].tolist() == [3]
    r = ES.sets(f.obs_sets, f.obs_points_sets, f.e_min, f.e_max, [[np.nan, 0.0, 0.5]])
    assert r["status"].tolist() == [4]
    # a ring of 24 small cubes around the seed needs more than 14 halfspaces
    ang = np.linspace(0, 2 * np.pi, 24, endpoint=False)
    ring = [np.concatenate((c - 0.02, c + 0.02)) for c in np.stack((0.2 * np.cos(ang), 0.2 * np.sin(ang), np.full(24, 0.5)), 1)]
    pl = BoundPlanner(obstacles=np.array(ring), e_p_max=0.5, obs_size_increase=0.0, seed=0)
    g = pl.set_finder
    A, _, _, _ = g.find_set_around_point(np.array([0.0, 0.0, 0.5]), optimize=False)
    assert A.shape[0] > 20
    r = ES.sets(g.obs_sets, g.obs_points_sets, g.e_min, g.e_max, [[0.0, 0.0, 0.5]], optimize=False)
    assert r["status"].tolist() == [2] and r["nrows"][0] == 0
    h = ConvexSetFinder(g.obs_sets, g.obs_points_sets, g.e_max, g.e_min, sets_fn=ES.sets)
    with pytest.raises(RuntimeError, match="more than 20 rows"):
        h.find_sets_around_points([[0.0, 0.0, 0.5]], optimize=False)


def test_batched_finder_methods():
    f = SC.example_finder()
    seeds = SC.free_seeds(f, 6, 3)
    g = ConvexSetFinder(f.obs_sets, f.obs_points_sets, f.e_max, f.e_min, sets_fn=ES.sets)
    for want, got in zip(f.find_sets_around_points(seeds, fixed_mid=True), g.find_sets_around_points(seeds, fixed_mid=True)):
        assert len(want) == len(got) == 4 and want[0].shape == got[0].shape
        for x, y in zip(want, got):
            assert np.abs(x - y).max() < 1e-6
    p0, p1 = SC.segments(f, 6, 5)
    for want, got in zip(f.find_sets_collision_avoidance(p0, p1), g.find_sets_collision_avoidance(p0, p1)):
        assert len(got) == 5 and want[4] == got[4]
        for x, y in zip(want[:4], got[:4]):
            assert np.abs(x - y).max() < 1e-6


@pytest.fixture(scope="module")
def plan(golden_dir):
    return np.load(os.path.join(golden_dir, "plan.npz"))


def _planner(d, n, backend):
    return BoundPlanner(obstacles=d[f"{n}_boxes"], e_p_max=0.5, workspace_max=d[f"{n}_ws_max"], workspace_min=d[f"{n}_ws_min"], seed=7,
                        set_backend=backend)


def check_plans(plan, backend):
    """tests/test_planner.py's three plans and the replan, with the given set backend."""
    d = plan
    for name in ("example", "wall", "free"):
        pl = _planner(d, name, backend)
        p_via, r_via, bp1, sets = pl.plan_convex_set_path(d[f"{name}_start"], d[f"{name}_end"], d[f"{name}_r0"], d[f"{name}_r1"])
        assert len(p_via) == d[f"{name}_p_via"].shape[0] and pl.nr_sets == int(d[f"{name}_nr_sets"])
        assert np.abs(np.array(p_via) - d[f"{name}_p_via"]).max() < 1e-6
        assert np.abs(np.array(r_via) - d[f"{name}_r_via"]).max() < 1e-6
        assert np.abs(np.array(bp1) - d[f"{name}_bp1"]).max() < 1e-6
        assert np.abs(np.array([s[0] for s in sets]) - d[f"{name}_A"]).max() < 1e-6
        assert np.abs(np.array([s[1] for s in sets]) - d[f"{name}_b"]).max() < 1e-6
    pl = _planner(d, "example", backend)
    pl.plan_convex_set_path(d["example_start"], d["example_end"], d["example_r0"], d["example_r1"])
    p_via, r_via, bp1, sets = pl.plan_convex_set_path(d["replan_start"], d["example_end"], d["replan_r0"], d["example_r1"], replanning=True,
                                                      p_horizon=list(d["replan_horizon"]))
    assert abs(pl.replanning_phi - float(d["replan_phi"])) < 1e-9
    assert np.abs(np.array(p_via) - d["replan_p_via"]).max() < 1e-6
    assert np.abs(np.array(r_via) - d["replan_r_via"]).max() < 1e-6
    assert np.abs(np.array([s[1] for s in sets]) - d["replan_b"]).max() < 1e-6


def test_planner_with_the_emulated_backend(plan):
    calls = []

    def backend(*a, **kw):
        calls.append(np.asarray(a[4]).reshape(-1, 3).shape[0])
        return ES.sets(*a, **kw)
    check_plans(plan, backend)
    assert len(calls) > 0 and max(calls) >= 1
