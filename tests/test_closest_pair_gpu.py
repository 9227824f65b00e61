"""The closest pair and the separating halfspaces of the HIP kernels on the MI355X against the exact QP solve of
tests/closest_pair_lib.py: (a) the closed loop's collision sets (bmpc_loop_k_colpairs_scenes + bmpc_loop_k_prepare_scenes) on one
DeviceLoop with 96 rollouts, one obstacle scene per rollout, (b) the segment mode of the set kernel (HipBoundMPC.convex_sets), (c)
position independence.  The cases, families, bounds and checks are those of tests/test_closest_pair.py (CPU)."""
import numpy as np
import pytest

import closest_pair_lib as L
from test_device_loop_gpu import _params, _scenario

pytestmark = pytest.mark.gpu

N, R = 10, 96
WIDE = ([-3.0] * 3, [3.0] * 3)


class Rig:
    """96 rollouts at random configurations q whose collision points move to those of qf: q itself (single points), 1e-13 rad
    away, ~0.03 rad and ~0.5 rad away per joint (segments up to ~0.6 m)."""

    def __init__(self):
        from boundplanner_amd.batch_node import BatchMPCNode
        from boundplanner_amd.params import COL_JOINT_SIZES
        from boundplanner_amd.solver import HipBoundMPC
        self.be = HipBoundMPC(N, max_batch=R)
        self.q, plans = _scenario(self.be, R, N, 515)
        rng = np.random.default_rng(875)
        step = np.array([0.0, 1e-13, 0.03, 0.5])[np.arange(R) % 4]
        self.qf = self.q + step[:, None] * rng.uniform(-1, 1, size=(R, 7))
        self.c0, self.c1 = self.be.fk(self.q)["col_pts"].reshape(R, 6, 3), self.be.fk(self.qf)["col_pts"].reshape(R, 6, 3)
        self.colsize = np.asarray(COL_JOINT_SIZES, float)
        self.node = BatchMPCNode(self.be, self.q, _params(N))
        for r, P in enumerate(plans):
            self.node.update_reference(r, [self.node.p_lie[r][:3].copy(), P["goal"].copy()], [m.copy() for m in P["r_via"]], [b.copy() for b in P["bp1"]],
                                       [b.copy() for b in P["br1"]], [e.copy() for e in P["erb"]], [a.copy() for a in P["a"]], [b.copy() for b in P["b"]])

    def loop(self, rows):
        from boundplanner_amd.device_loop import DeviceLoop
        n = self.node
        loop = DeviceLoop(self.be, len(rows))
        for i, r in enumerate(rows):
            loop.set_rollout(i, n.mpcs[r], n.q[r], n.dq[r], n.ddq[r], n.jerk[r], self.qf[r], n.v[r], n.p_lie[r])
        loop.upload()
        return loop

    def rows(self, scenes, assign, rows=None):
        """the collision sets of the rollouts `rows` (all) with their scenes: (A [R][6][15][3], b [R][6][15], dead [R])"""
        from boundplanner_amd.device_loop import state_view
        rows = np.arange(R) if rows is None else rows
        loop = self.loop(rows)
        loop.set_scenes([([p.as_set() for p in ps], [p.pts for p in ps]) for ps in scenes], assign)
        loop.prepare()
        p = loop.problem()[3]
        loop.download()
        A = p[:, 515:785].reshape(len(rows), 6, 3, 15).transpose(0, 1, 3, 2)
        b = p[:, 785:875].reshape(len(rows), 15, 6).transpose(0, 2, 1)
        return A, b, state_view(loop.lay, loop.state)["dead"][:, 0].copy()


@pytest.fixture(scope="module")
def rig():
    return Rig()


@pytest.fixture(scope="module")
def single(rig):
    """one obstacle per rollout, every family in turn, placed around one of the rollout's six segments so that it falls into one of
    the classes of closest_pair_lib.segments_around; [(Poly, exact pairs of the six segments)]"""
    rng = np.random.default_rng(96)
    pool = [p for ps in L.families().values() for p in ps]
    out = []
    for r in range(R):
        base, j = pool[r % len(pool)], (r // len(pool) + r) % 6
        while True:
            p = L.place_at(base, rig.c0[r, j], rig.c1[r, j], rng)
            EX = L.exact_pairs(p, rig.c0[r], rig.c1[r])
            if all(L.admissible(E) for E in EX):
                break
        out.append((p, EX))
    return out


def _loop_result(A, b, dead, r, j):
    """(n or -1, rows, offsets, None) of collision point j of rollout r as the checks take them: the padding rows are zero"""
    n = 6 + int((np.abs(A[r, j, 6:]).sum(axis=1) > 0).sum())
    return (-1 if dead[r] == 2 else n), A[r, j], b[r, j], None


def test_loop_rows_of_single_obstacles(rig, single):
    A, b, dead = rig.rows([[p] for p, _ in single], np.arange(R))
    assert np.isfinite(A).all() and np.isfinite(b).all() and not dead.any()
    seen = dict.fromkeys(("through", "face", "edge", "vertex", "phi0", "phi1", "phi_in", "point", "tiny", "flat"), 0)
    fams, wa, wb = set(), 0.0, 0.0
    for r, (p, EX) in enumerate(single):
        fams.add(p.name)
        for j, E in enumerate(EX):
            n, a, bb, _ = _loop_result(A, b, dead, r, j)
            L_ = np.linalg.norm(rig.c1[r, j] - rig.c0[r, j])
            seen["point"] += L_ == 0; seen["tiny"] += 0 < L_ < 1e-12
            if E["through"]:
                assert n == 7, (r, j, n)
                seen["through"] += 1
                continue
            seen[E["feature"]] += 1; seen["phi" + {"0": "0", "1": "1", "in": "_in"}[E["phi_class"]]] += 1; seen["flat"] += E["flat"]
            rep = L.replay([p], [E], rig.c0[r, j], rig.c1[r, j], 15)
            ra, rb = L.check_rows(f"loop: rollout {r} ({p.name}) point {j}", a, bb, n, None, rep, shift=rig.colsize[j])
            wa, wb = max(wa, ra), max(wb, rb)
    print(f"loop on the GPU: single obstacles: worst row / bound: a {wa:.2g}, bh {wb:.2g}; {seen}")
    assert all(v > 0 for v in seen.values()), seen
    assert fams >= {"axis_box", "rot_box", "tet_sliver", "wedge2", "wedge4", "pyramid", "prism13", "pts32"}, fams


def test_loop_rows_of_scenes(rig):
    """8 scenes of 2 .. 16 obstacles around the first 8 rollouts with segments of some length (the last two on a sphere around a
    collision point: more rows than 15, the rollout is dead with code 2)"""
    rng = np.random.default_rng(8)
    rollouts = [r for r in range(R) if r % 4 >= 2][:8]
    scenes, exact = [], []
    for k, (r, n) in enumerate(zip(rollouts, (2, 3, 5, 8, 12, 16, 12, 16))):
        polys, ex = L.scene_for_segments(rig.c0[r], rig.c1[r], n, rng, sphere=rig.c0[r, 5] if k >= 6 else None)
        scenes.append(polys); exact.append(ex)
    assign = np.full(R, -1)
    assign[rollouts] = np.arange(8)
    A, b, dead = rig.rows(scenes, assign)
    assert not dead[np.setdiff1d(np.arange(R), rollouts)].any()
    n_cases = left_out = overflow = most = 0
    for k, r in enumerate(rollouts):
        reps = [L.replay(scenes[k], exact[k][j], rig.c0[r, j], rig.c1[r, j], 15) for j in range(6)]
        n_cases += 6
        left_out += sum(not rep["decidable"] for rep in reps)
        over = any(rep["overflow"] for rep in reps)
        if all(rep["decidable"] for rep in reps):
            assert (dead[r] == 2) == over and dead[r] in (0, 2), (k, r, dead[r], over)
            overflow += over
        if dead[r]:
            continue                      # (the loop keeps the rows that fit, of the points before the overflow)
        for j, rep in enumerate(reps):
            if rep["decidable"]:
                n, a, bb, _ = _loop_result(A, b, dead, r, j)
                L.check_rows(f"loop: scene {k} point {j}", a, bb, n, None, rep, shift=rig.colsize[j])
                most = max(most, n)
    print(f"loop on the GPU: scenes: {n_cases} cases, left out {left_out}, overflow {overflow} scenes, most rows {most}")
    assert left_out <= L.MAX_LEFT_OUT * n_cases and overflow and most >= 9


def _gpu_set_rows(be):
    from test_closest_pair import set_rows
    return lambda polys, P0, P1: set_rows(be.convex_sets([p.as_set() for p in polys], [p.pts for p in polys], *WIDE, P0, P1))


@pytest.fixture(scope="module")
def cases128():
    return L.single_cases(per_poly=128)


def test_set_kernel_rows(rig, cases128):
    """one call per single-obstacle scene with 128 segments each, then the multi-obstacle scenes (up to 32 obstacles, 20 rows)"""
    cases = cases128
    assert L.check_single_rows("set kernel on the GPU", cases, _gpu_set_rows(rig.be), 20)
    ov, most = L.check_scene_rows("set kernel on the GPU", L.scene_cases(nseg=8), _gpu_set_rows(rig.be), 20, 32)
    assert ov and most >= 4
    L.check_scene_rows("set kernel on the GPU, grazing", L.grazing_cases(), _gpu_set_rows(rig.be), 20, 32)


def test_position_independence(rig, single, cases128):
    """a rollout alone gives bitwise the rows it gives inside the batch; a segment alone gives bitwise the rows it gives among 128;
    and the set kernel's rows are bitwise the loop's for the same segment (general polytopes: the loop clamps an axis-aligned box)"""
    A, b, dead = rig.rows([[p] for p, _ in single], np.arange(R))
    for r in (3, 64, 95):
        A1, b1, d1 = rig.rows([[single[r][0]]], np.zeros(1, int), rows=np.array([r]))
        assert np.array_equal(A1[0], A[r]) and np.array_equal(b1[0], b[r]) and d1[0] == dead[r], r
    fam, p, P0, P1, EX = cases128[-1]
    rows = _gpu_set_rows(rig.be)
    batch = rows([p], P0, P1)
    for k in (0, 63, 64, 127):
        n, a, bb, c = rows([p], P0[k:k + 1], P1[k:k + 1])[0]
        assert n == batch[k][0] and np.array_equal(a, batch[k][1]) and np.array_equal(bb, batch[k][2]) and c == batch[k][3], k
    same = 0
    for r, (p, EX) in enumerate(single):
        if p.name == "axis_box" or r % 4 < 2:
            continue
        s = rows([p], rig.c0[r], rig.c1[r])
        for j, E in enumerate(EX):
            n = s[j][0]
            if E["through"]:
                continue
            assert n == 7 and np.array_equal(s[j][1][6], A[r, j, 6]), (r, j, np.abs(s[j][1][6] - A[r, j, 6]).max())
            # the loop subtracts the joint size from the offset: the set kernel's offset, rounded the same way, is the loop's
            assert s[j][2][6] - rig.colsize[j] == b[r, j, 6], (r, j, s[j][2][6] - rig.colsize[j] - b[r, j, 6])
            same += 1
    assert same > 100
