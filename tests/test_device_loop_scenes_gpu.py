"""One obstacle scene per rollout on the MI355X (bmpc_loop_set_scenes / bmpc_loop_set_rollout_scenes, kernels
bmpc_loop_k_colpairs_scenes + bmpc_loop_k_prepare_scenes): a loop whose rollouts look at different scenes gives, rollout by rollout,
bitwise what loops on the existing shared-scene path (bmpc_loop_set_obstacles) give for the rollouts of each scene, and tracks the
host loop whose BoundMPC objects were given their scenes with set_obstacle_sets."""
import ctypes

import numpy as np
import pytest

from test_device_loop_gpu import _params, _scenario

pytestmark = pytest.mark.gpu

N, R, STEPS = 10, 12, 6
_ip = ctypes.POINTER(ctypes.c_int)


def make_scenes(col0, seed=3, counts=(6, 3, 5), rotated=(0.0, 0.5, 0.0)):
    """Scenes of boxes 0.15 to 0.45 m from the nearest collision point at the start (col0: the collision points of ALL rollouts, so
    that every rollout may be given every scene): near the arms, but no point starts inside an obstacle -- a collision point inside
    one has no separating halfspace (0/0 in the reference's finder as well).  (Rotated boxes are judged by their bounding box.)"""
    from test_device_loop import _box_scene
    rng, out = np.random.default_rng(seed), []
    for n, rot in zip(counts, rotated):
        sets, pts = [], []
        while len(sets) < n:
            s1, p1 = _box_scene(rng, 1, rotated=rot)
            lo, hi = p1[0].min(axis=0), p1[0].max(axis=0)
            gap = np.linalg.norm(np.maximum(np.maximum(lo - col0, col0 - hi), 0.0), axis=1).min()
            if 0.15 < gap < 0.45:
                sets += s1; pts += p1
        out.append((sets, pts))
    return out


class Setup:
    """The rollouts (configs[4]-style plans on N = 10) and the scenes of this file; every loop is built from freshly constructed
    host objects, which is deterministic, so two loops holding the same rollout start from the same bits."""

    def __init__(self):
        from boundplanner_amd.solver import HipBoundMPC
        self.params = _params(N)
        self.be = HipBoundMPC(N, max_batch=R)
        self.q_start, self.plans = _scenario(self.be, R, N, 77)
        self.scenes = make_scenes(self.be.fk(self.q_start)["col_pts"].reshape(-1, 3))
        self.rollout_scene = np.array([r % 4 if r % 4 < 3 else -1 for r in range(R)])

    def scene_of(self, r, assign=None):
        s = (self.rollout_scene if assign is None else assign)[r]
        return self.scenes[s] if s >= 0 else ([], [])

    def node(self, rows, assign=None, with_scenes=False):
        """BatchMPCNode of the rollouts `rows` with their plans (and, for the host loop, their scenes)."""
        from boundplanner_amd.batch_node import BatchMPCNode
        node = BatchMPCNode(self.be, self.q_start[rows], self.params)
        for i, r in enumerate(rows):
            P = self.plans[r]
            if with_scenes and len(self.scene_of(r, assign)[0]):
                node.mpcs[i].set_obstacle_sets(*self.scene_of(r, assign))
            node.update_reference(i, [node.p_lie[i][:3].copy(), P["goal"].copy()], [m.copy() for m in P["r_via"]], [b.copy() for b in P["bp1"]],
                                  [b.copy() for b in P["br1"]], [e.copy() for e in P["erb"]], [a.copy() for a in P["a"]], [b.copy() for b in P["b"]])
        return node

    def loop(self, rows):
        from boundplanner_amd.device_loop import DeviceLoop
        ref = self.node(rows)
        loop = DeviceLoop(self.be, len(rows))
        for i in range(len(rows)):
            loop.set_rollout(i, ref.mpcs[i], ref.q[i], ref.dq[i], ref.ddq[i], ref.jerk[i], ref.qf[i], ref.v[i], ref.p_lie[i])
        loop.upload()
        return loop

    def mixed_loop(self, assign=None):
        loop = self.loop(np.arange(R))
        loop.set_scenes(self.scenes, self.rollout_scene if assign is None else assign)
        return loop

    def shared_loop(self, rows, scene):
        """The existing path: the rollouts `rows`, all of them on scene `scene` (set_obstacles; nothing for -1)."""
        loop = self.loop(rows)
        if scene >= 0:
            loop.set_obstacles(*self.scenes[scene])
        return loop


@pytest.fixture(scope="module")
def su():
    return Setup()


def _end_state(loop):
    loop.download()
    return loop.state.copy(), loop.prev.copy()


def _assert_same(mixed, single, rows, what):
    """log [steps][R][w], state [R][.], prev [R][.] of the mixed loop against those of a loop holding the rollouts `rows`."""
    for name, a, b in zip(("log", "state", "prev"), mixed, single):
        a = a[:, rows] if name == "log" else a[rows]
        assert np.isfinite(a).all() and np.array_equal(a, b), (what, name, float(np.abs(a - b).max()))


def _alive(loop, state):
    from boundplanner_amd.device_loop import state_view
    return (state_view(loop.lay, state)["dead"] == 0).all()


def test_mixed_loop_equals_single_scene_loops(su):
    probe = su.mixed_loop()
    probe.prepare()
    p = probe.problem()[3]
    loop = su.mixed_loop()
    rows_per_set = (np.abs(p[:, 515:785].reshape(R, 6, 3, 15)).sum(axis=2) > 0).sum(axis=2)
    assert rows_per_set.max() > 6                                         # obstacle halfspaces are active in the collision sets ...
    assert (rows_per_set[su.rollout_scene < 0] == 6).all()                # ... and not for the rollouts without a scene
    log = loop.run(STEPS)
    mixed = (log,) + _end_state(loop)
    assert _alive(loop, mixed[1]) and (log[:, :, loop.LOG["dead"]] == 0).all()
    for scene in (0, 1, 2, -1):
        rows = np.nonzero(su.rollout_scene == scene)[0]
        assert len(rows) == 3
        single = su.shared_loop(rows, scene)
        slog = single.run(STEPS)
        _assert_same(mixed, (slog,) + _end_state(single), rows, scene)
    # the scenes do matter: a rollout of scene 0 does not move as its neighbour's scene would make it
    other = su.shared_loop(np.array([0]), 1)
    assert not np.array_equal(other.run(STEPS)[:, 0], log[:, 0])


def test_one_scene_for_everybody_equals_set_obstacles(su):
    rows = np.arange(R)
    shared = su.shared_loop(rows, 1)
    ref = (shared.run(STEPS),) + _end_state(shared)
    assert _alive(shared, ref[1])
    table = su.mixed_loop(np.full(R, 1))
    _assert_same((table.run(STEPS),) + _end_state(table), ref, rows, "table, everybody on scene 1")
    # the later call wins: set_obstacles after set_scenes is the shared scene again ...
    back = su.mixed_loop()
    back.set_obstacles(*su.scenes[1])
    _assert_same((back.run(STEPS),) + _end_state(back), ref, rows, "set_obstacles after set_scenes")
    # ... and set_scenes after set_obstacles is the table
    fwd = su.shared_loop(rows, 0)
    fwd.set_scenes(su.scenes, np.full(R, 1))
    _assert_same((fwd.run(STEPS),) + _end_state(fwd), ref, rows, "set_scenes after set_obstacles")


def test_run_async_equals_run_on_the_mixed_loop(su):
    a, b = su.mixed_loop(), su.mixed_loop()
    la, lb = a.run(STEPS), b.run_async(STEPS)
    assert np.isfinite(la).all() and np.array_equal(la, lb)
    assert (la[:, :, a.LOG["dead"]] == 0).all() and _alive(a, _end_state(a)[0]) and _alive(b, _end_state(b)[0])
    assert len(set(la[:, :, a.LOG["iters"]].ravel().tolist())) > 3          # the solves do take different numbers of iterations


def test_mixed_loop_tracks_the_host_loop(su):
    rows = np.arange(R)
    host = su.node(rows, with_scenes=True)
    loop = su.mixed_loop()
    dmax, n_rows = 0.0, 0
    for k in range(STEPS):
        loop.prepare()
        p_dev = loop.problem()[3]
        assert np.isfinite(p_dev).all(), k
        host.step()
        loop.solve()
        log = loop.finish()
        n_rows = max(n_rows, int((np.abs(p_dev[:, 515:785].reshape(R, 6, 3, 15)).sum(axis=2) > 0).sum(axis=2).max()))
        assert np.isfinite(log).all() and np.isfinite(host.q).all(), k
        dmax = max(dmax, np.abs(log[:, loop.LOG["q"]] - host.q).max(), np.abs(log[:, loop.LOG["p_lie"]] - host.p_lie).max())
    print(f"mixed loop against the host loop: max deviation {dmax:.2e}, most rows in a collision set {n_rows}")
    assert n_rows > 6
    assert np.isfinite(dmax) and dmax < 1e-5, dmax           # the halfspaces agree to ~1e-7 (golden section), the closed loops stay together
    assert (log[:, loop.LOG["dead"]] == 0).all()


def test_reassignment_between_runs(su):
    from boundplanner_amd.device_loop import DeviceLoop
    k = STEPS // 2
    loop = su.mixed_loop()
    loop.run(k)
    state, prev = _end_state(loop)
    assign = su.rollout_scene.copy()
    assign[[0, 1, 3, 6]] = [2, -1, 0, 2]                         # scene 0 -> 2, 1 -> none, none -> 0, 2 stays
    loop.set_rollout_scene(0, assign[0])                         # one rollout
    loop.set_rollout_scene(1, assign[1:7])                       # a range
    log2 = loop.run(k)
    mixed = (log2,) + _end_state(loop)
    assert _alive(loop, mixed[1])
    for scene in (0, 1, 2, -1):
        rows = np.nonzero(assign == scene)[0]
        assert len(rows) >= 2
        single = DeviceLoop(su.be, len(rows))                    # handed the downloaded state at the switch
        single.state[:], single.prev[:] = state[rows], prev[rows]
        single.upload()
        if scene >= 0:
            single.set_obstacles(*su.scenes[scene])
        slog = single.run(k)
        _assert_same(mixed, (slog,) + _end_state(single), rows, scene)


def test_misuse_is_refused_and_changes_nothing(su):
    from emu_loop_scenes_lib import pack_scenes
    loop = su.mixed_loop()
    ref = loop.run(3)
    lib, l = loop.lib, loop._l
    n_obs, A, b, nrows, V, nv = pack_scenes(su.scenes)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(_ip)

    def changed(a, i, v):
        a = a.copy(); a[i] = v
        return a

    good = dict(n=len(su.scenes), n_obs=n_obs, A=A, b=b, nrows=nrows, V=V, nv=nv)
    bad_tables = {"n_scenes < 0": dict(n=-1), "null n_obs": dict(n_obs=None), "null A": dict(A=None), "null b": dict(b=None),
                  "null nrows": dict(nrows=None), "null V": dict(V=None), "null nv": dict(nv=None),
                  "17 obstacles": dict(n_obs=changed(n_obs, 1, 17)), "-1 obstacles": dict(n_obs=changed(n_obs, 0, -1)),
                  "16 rows": dict(nrows=changed(nrows, 4, 16)), "0 rows": dict(nrows=changed(nrows, 0, 0)),
                  "33 vertices": dict(nv=changed(nv, 7, 33)), "0 vertices": dict(nv=changed(nv, 2, 0))}
    bad_assign = {"scene == n_scenes": (0, [0, 3]), "scene -2": (2, [-2]), "first < 0": (-1, [0]), "past R": (R - 1, [0, 1]),
                  "count 0": (0, []), "null scene": (0, None)}

    def refused(rc, what, l=l):
        msg = lib.bmpc_loop_last_error(l).decode()
        assert rc == 1 and msg and any(s in msg for s in ("bmpc_loop_set_", "obstacle with", "rollout range")), (what, rc, msg)

    loop.upload()                         # back to the start: the same 3 steps again, after every kind of refused call
    for what, kw in bad_tables.items():
        a = dict(good, **kw)
        I = lambda x: ip(x) if x is not None else None
        D = lambda x: dp(x) if x is not None else None
        refused(lib.bmpc_loop_set_scenes(l, a["n"], I(a["n_obs"]), D(a["A"]), D(a["b"]), I(a["nrows"]), D(a["V"]), I(a["nv"])), what)
    for what, (first, sc) in bad_assign.items():
        refused(lib.bmpc_loop_set_rollout_scenes(l, first, 1 if sc is None else len(sc), ip(sc) if sc is not None else None), what)
    assert np.array_equal(loop.run(3), ref)
    assert lib.bmpc_loop_set_scenes(None, 0, None, None, None, None, None, None) == 1
    assert lib.bmpc_loop_set_rollout_scenes(None, 0, 1, ip([0])) == 1
    with pytest.raises(ValueError):
        loop.set_scenes(su.scenes, np.zeros(R - 1, int))
    with pytest.raises(ValueError):                            # pack_obstacles' 16-obstacle check, per scene
        loop.set_scenes([(su.scenes[0][0] * 3, su.scenes[0][1] * 3)])
    # an assignment without a table: only -1 exists
    plain = su.shared_loop(np.arange(2), 0)
    refused(lib.bmpc_loop_set_rollout_scenes(plain._l, 0, 1, ip([0])), "no table", plain._l)
    assert lib.bmpc_loop_set_rollout_scenes(plain._l, 0, 2, ip([-1, -1])) == 0


def test_empty_scenes_in_the_table(su):
    """A scene without obstacles between non-empty ones (prefix offsets with an empty range), and a table without any obstacle
    at all (no closest-pair results, only the prepare kernel is launched)."""
    mixed = su.mixed_loop()
    ref = (mixed.run(STEPS),) + _end_state(mixed)
    # the same assignment through a table with an empty scene in the middle; the rollouts without a scene name the empty one
    loop = su.loop(np.arange(R))
    loop.set_scenes([su.scenes[0], ([], []), su.scenes[1], su.scenes[2]], np.array([0, 2, 3, 1])[su.rollout_scene % 4])
    _assert_same((loop.run(STEPS),) + _end_state(loop), ref, np.arange(R), "empty scene in the table")
    free = su.shared_loop(np.arange(R), -1)
    ref = (free.run(STEPS),) + _end_state(free)
    loop = su.loop(np.arange(R))
    loop.set_scenes([([], []), ([], [])], np.array([0, 1, -1] * (R // 3)))
    _assert_same((loop.run(STEPS),) + _end_state(loop), ref, np.arange(R), "table without obstacles")
    loop.set_scenes([], None)                                   # n_scenes = 0 clears the table
    assert np.isfinite(loop.run(1)).all()
