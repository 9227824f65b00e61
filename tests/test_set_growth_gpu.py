"""The metric projection, the inscribed ellipsoid and the set growth on the GPU against the references of tests/set_growth_lib.py:
bmpc_debug_sets_parts (HipBoundMPC.sets_parts: one lane per item runs sp_polyhedron in a given metric, or sp_mvie with a fixed or a
free centre on given rows -- the same device functions as the product's kernel) and whole runs of HipBoundMPC.convex_sets.  67 items
per call (64 per workgroup: a ragged second group); items 0, 63, 64 and 66 alone must be bitwise themselves inside the batch."""
import numpy as np
import pytest

import set_growth_lib as SG
from boundplanner_amd import planner_opt as PO

pytestmark = pytest.mark.gpu
B = 67
ALONE = (0, 63, 64, 66)


@pytest.fixture(scope="module")
def be():
    from boundplanner_amd.solver import HipBoundMPC
    return HipBoundMPC(10)


def _same_alone(r, one):
    """one(k) -> the result dict of item k run in a call of its own"""
    for k in ALONE:
        r1 = one(k)
        for key in r:
            assert np.array_equal(r1[key][0], r[key][k], equal_nan=True), (k, key)


@pytest.fixture(scope="module")
def proj_cases():
    return SG.projection_cases()


def test_gpu_projection_of_every_polytope(be, proj_cases):
    """One call per polytope (20), 67 of its (metric, seed) items: the single obstacle's row, a ~ E^-2 (pt - p), b = a.pt, against the
    exact projection within 32 x HOST_WORST; seeds nearer than 0.99 in the metric give -1."""
    by_poly = {}
    for fam, p, name, E, S, EX in proj_cases:
        by_poly.setdefault(id(p), (fam, p, []))[2].extend((E, s) for s in S)
    assert len(by_poly) == 20
    worst, n_viol, n_rows = 0.0, 0, 0
    for fam, p, all_items in by_poly.values():
        assert len(all_items) == 72
        # two calls of 67: items 0 .. 66, and the remaining 5 followed by repeats of the first 62
        for call, (items, fresh) in enumerate(((all_items[:B], B), (all_items[B:] + all_items[:2 * B - 72], 72 - B))):
            E = np.array([e for e, s in items]); S = np.array([s for e, s in items])
            scene = ([p.as_set()], [p.pts], SG.WS_MIN, SG.WS_MAX)
            r = be.sets_parts(0, S, E=E, scene=scene)
            for k in range(fresh):
                rep = SG.round_replay([p], E[k], S[k])
                assert rep["decidable"], (fam, k)
                worst = max(worst, SG.check_round(f"{fam} call {call} item {k}", rep, int(r["nrows"][k]), r["A"][k], r["b"][k]))
                n_viol += rep["violates"]; n_rows += not rep["violates"]
            if call == 0 and fam in ("axis_box", "wedge2"):
                _same_alone(r, lambda k: be.sets_parts(0, S[k:k + 1], E=E[k:k + 1], scene=scene))
    print(f"projection rows: worst / bound {worst:.2g}; {n_rows} rows, {n_viol} violations")
    assert n_rows + n_viol == 20 * 72 and n_rows >= 500 and n_viol >= 20


def test_gpu_one_round_scenes(be):
    """The scenes of the CPU test, each as one call of 67 seeds around its seed (the first item is the scene's own)."""
    rng = np.random.default_rng(1)
    scenes = SG.round_scenes()
    pick = [scenes[i] for i in (0, 3, 7, 14, 22, 31)] + scenes[40:42]          # (40, 41: the two rings)
    cls = dict(violates=0, overflow=0, rows=0)
    left = n = 0
    for j, (polys, E, p) in enumerate(pick):
        S = p + np.vstack((np.zeros(3), rng.uniform(-0.01, 0.01, (B - 1, 3))))
        scene = ([P.as_set() for P in polys], [P.pts for P in polys], SG.WS_MIN, SG.WS_MAX)
        Es = np.broadcast_to(E, (B, 3, 3)).copy()
        r = be.sets_parts(0, S, E=Es, scene=scene)
        for k in range(0, B, 1 if len(polys) <= 8 else 8):
            if np.min([np.max((P.A @ S[k] - P.b) / np.linalg.norm(P.A, axis=1)) for P in polys]) < 1e-3:
                continue
            rep = SG.round_replay(polys, E, S[k])
            n += 1
            if not rep["decidable"]:
                left += 1
                continue
            SG.check_round(f"scene {j} item {k}", rep, int(r["nrows"][k]), r["A"][k], r["b"][k])
            cls["violates"] += rep["violates"]; cls["overflow"] += rep["overflow"]; cls["rows"] = max(cls["rows"], len(rep["rows"]))
        if j in (0, len(pick) - 1):
            _same_alone(r, lambda k: be.sets_parts(0, S[k:k + 1], E=Es[k:k + 1], scene=scene))
    for j, (polys, E, p) in enumerate(SG.grazing_scenes()):          # the -1e-4 of the dropping rule: the scene's own seed in every item
        scene = ([P.as_set() for P in polys], [P.pts for P in polys], SG.WS_MIN, SG.WS_MAX)
        r = be.sets_parts(0, np.broadcast_to(p, (B, 3)).copy(), E=np.broadcast_to(E, (B, 3, 3)).copy(), scene=scene)
        rep = SG.round_replay(polys, E, p)
        assert rep["decidable"] and len(rep["rows"]) == 1 + j % 2
        for k in (0, 63, 64, 66):
            SG.check_round(f"grazing scene {j} item {k}", rep, int(r["nrows"][k]), r["A"][k], r["b"][k])
    print(f"rounds: {n} cases, left out {left}, classes {cls}")
    assert left <= SG.MAX_LEFT_OUT * n and cls["violates"] >= 1 and cls["overflow"] >= 1 and cls["rows"] >= 5


def _gpu_mvie_call(be, mode, part, fresh, alone):
    """one call of 67 problems; the first `fresh` of them are checked (the rest repeat problems of the other call)"""
    A = np.zeros((B, 20, 3)); b = np.zeros((B, 20)); m = np.zeros(B, np.int32); p = np.zeros((B, 3))
    for k, (name, Ak, bk, fixed, start) in enumerate(part):
        m[k] = len(bk); A[k, :m[k]] = Ak; b[k, :m[k]] = bk
        p[k] = fixed if fixed is not None else start
    r = be.sets_parts(mode, p, rows=(A, b, m))
    probs = [(n, Ak, bk, f) for n, Ak, bk, f, s in part[:fresh]]
    host = []
    for n, Ak, bk, f in probs:
        qh, ch = PO.mvie(Ak, bk, fixed_mid=f)
        host.append(SG.mvie_certificate(qh, ch, Ak, bk, f is None))
    refs = [SG.mvie_reference(Ak, bk, r["q"][k], r["c"][k], f is None) if r["status"][k] == 0 else None for k, (n, Ak, bk, f) in enumerate(probs)]
    SG.check_mvie_answers(f"gpu mode {mode}", probs[:fresh], [(int(r["status"][k]), r["q"][k], r["c"][k]) for k in range(fresh)],
                          [[x, h] for x, h in zip(refs, host)])
    assert (r["newton"] > 0).all()
    if alone:
        _same_alone(r, lambda k: be.sets_parts(mode, p[k:k + 1], rows=(A[k:k + 1], b[k:k + 1], m[k:k + 1])))


def test_gpu_mvie_direct_families(be):
    """The direct row families with a fixed centre (mode 1) and a free one (mode 2), 67 problems per call."""
    problems = SG.mvie_problems()
    for mode, sel in ((1, [p for p in problems if p[3] is not None]), (2, [p for p in problems if p[3] is None])):
        assert len(sel) == 72
        for call, (part, fresh) in enumerate(((sel[:B], B), (sel[B:] + sel[:2 * B - 72], 72 - B))):
            _gpu_mvie_call(be, mode, part, fresh, alone=call == 0)
    # statuses: a fixed centre outside and on a face, an empty set
    A1, b1 = SG.mvie_families()["box"][0]
    A = np.zeros((3, 20, 3)); b = np.zeros((3, 20)); A[:, :6] = A1; b[:, :6] = b1
    r = be.sets_parts(1, np.array([[5.0, 0, 0], [0.3, 0, 0], [0.0, 0, 0]]), rows=(A, b, np.full(3, 6, np.int32)))
    assert r["status"].tolist() == [3, 3, 0]
    A[0, 6] = [1.0, 0, 0]; b[0, 6] = -1.0
    assert be.sets_parts(2, np.zeros((1, 3)), rows=(A[:1], b[:1], np.array([7], np.int32)))["status"].tolist() == [3]


def test_gpu_whole_runs(be):
    rounds, status, reasons = SG.check_runs("gpu", be.convex_sets)
    assert set(status) == {0} and set(rounds) == {1, 2, 3, 4, 5}, (rounds, status)
    assert all(reasons[k] >= 1 for k in ("eigenvalue", "one_percent", "limit")), reasons


def test_gpu_whole_run_statuses(be):
    SG.check_statuses("gpu", be.convex_sets)
