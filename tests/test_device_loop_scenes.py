"""One obstacle scene per rollout in the device-resident loop (bmpc_loop_set_scenes / bmpc_loop_set_rollout_scenes), on the CPU
build of the identical header (tests/emu/emu_loop_scenes.cpp): scene resolution by the shared function loop_scene_of, the
closest pairs over the rollout's own scene, loop_prepare, the start vector.  The yardsticks are the existing shared-scene path
(emu_loop_prepare_obs, one rollout with one scene: bitwise) and the host mirror BoundMPC.prepare with set_obstacle_sets."""
import os
import re

import numpy as np
from scipy.spatial.transform import Rotation as Rot

import emu_loop_lib as E
import emu_loop_scenes_lib as ES
import oracle_lib as O
from boundplanner_amd.device_loop import pack_state, state_view
from boundplanner_amd.params import Params, Q_LIM_LOWER, Q_LIM_UPPER, get_default_params
from boundplanner_amd.robot_model import RobotModel
from test_device_loop import _box_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 8


def _params():
    base = get_default_params()
    return Params(n=N, dt=base.dt, build=False, weights=base.weights, nr_segs=base.nr_segs)


def _rollouts(rng, R, robot, params, lay):
    """R rollouts at random configurations with a horizon end qf near q (the degenerate segment qf == q among them): the host
    objects, the node state of each and the packed state vectors."""
    from boundplanner_amd.bound_mpc import BoundMPC
    mpcs, node, S = [], [], np.zeros((R, lay["_size"]))
    for r in range(R):
        q = rng.uniform(0.6 * Q_LIM_LOWER, 0.6 * Q_LIM_UPPER)
        qf = q + rng.normal(size=7) * [0.0, 0.05, 0.4][r % 3]
        dq = rng.normal(size=7) * 0.1
        p_lie = robot.fk(q)
        mpc = BoundMPC([p_lie[:3]] * 2, [Rot.from_rotvec(p_lie[3:]).as_matrix()] * 2, [np.array([1.0, 0, 0])], [np.array([1.0, 0, 0])],
                       [np.array([90, 90, 90, -90, -90, -90]) * np.pi / 180], [np.zeros((15, 3))], [np.ones(15)], [], p0=p_lie,
                       params=params, robot_model=robot)
        v = np.concatenate((robot.velocity_ee(q, dq), robot.omega_ee(q, dq)))
        mpcs.append(mpc); node.append((q, dq, qf, v, p_lie))
        S[r] = pack_state(lay, mpc, q, dq, np.zeros(7), np.zeros(7), qf, v, p_lie)
    return mpcs, node, S


def _host_prepare(mpc, node, scene):
    """The host mirror's parameter vector of one rollout in one scene, or None where it raises (more than 15 rows)."""
    q, dq, qf, v, p_lie = node
    mpc.set_obstacle_sets(*scene)
    try:
        return mpc.prepare(q, dq, np.zeros(7), p_lie, v, np.zeros(7), qf)[3]
    except ValueError:
        return None


def _single(S_r, scene):
    """The existing entry: this rollout with this scene alone (emu_loop_prepare_obs, or emu_loop_prepare without obstacles)."""
    S1 = S_r.copy()
    out = E.prepare_obs(N, S1, np.zeros(44 * N + 6), *scene) if scene is not None and len(scene[0]) else E.prepare(N, S1, np.zeros(44 * N + 6))
    return out, S1


def _assert_bitwise(mixed, S_mixed, r, single, S_single):
    for name, a, b in zip(("x0", "lbx", "ubx", "p"), (m[r] for m in mixed), single):
        assert np.isfinite(a).all() and np.array_equal(a, b), (r, name, np.abs(a - b).max())
    assert np.array_equal(S_mixed[r], S_single), r


def test_each_rollout_sees_its_own_scene():
    params, lay, robot = _params(), E.layout(), RobotModel(O.fk_batch)
    rng = np.random.default_rng(21)
    scenes = [_box_scene(rng, n, rotated=rot) for n, rot in ((3, 0.0), (8, 0.5), (1, 1.0), (5, 0.5), (7, 0.0))]
    rollout_scene = np.array([3, 1, 4, 1, 0, 2, 4, 3, 0, 1, 2, 3])                  # not sorted, with repeats, every scene used
    R = len(rollout_scene)
    mpcs, node, S0 = _rollouts(rng, R, robot, params, lay)
    S = S0.copy()
    mixed = ES.prepare_scenes(N, S, np.zeros((R, 44 * N + 6)), scenes, rollout_scene)
    rows_seen, compared = set(), 0
    for r in range(R):
        scene = scenes[rollout_scene[r]]
        single, S1 = _single(S0[r], scene)
        _assert_bitwise(mixed, S, r, single, S1)
        p_host = _host_prepare(mpcs[r], node[r], scene)
        dead = state_view(lay, S[r])["dead"][0]
        assert dead == (2.0 if p_host is None else 0.0), r
        if p_host is None:
            continue
        p = mixed[3][r]
        assert np.abs(p[:515] - p_host[:515]).max() < 1e-12, r
        # halfspace rows: the golden-section closest pair is resolved to ~1e-8 along the segment on both sides
        assert np.abs(p[515:] - p_host[515:]).max() < 1e-6, (r, np.abs(p[515:] - p_host[515:]).max())
        a_j = p_host[515:785].reshape(6, 3, 15)
        rows_seen.update(int((np.abs(a_j[j]).sum(axis=0) > 0).sum()) for j in range(6))
        compared += 1
    assert compared >= 8 and len(set(rollout_scene.tolist())) >= 4
    assert max(rows_seen) > 7 and min(rows_seen) >= 6        # obstacle halfspaces were active: the scenes are not too far away
    # the scenes do differ for a rollout: the same rollout in another scene gets other collision sets
    other, _ = _single(S0[0], scenes[(rollout_scene[0] + 1) % len(scenes)])
    assert not np.array_equal(other[3][515:], mixed[3][0][515:])


def test_scene_minus_one_and_an_empty_scene_are_obstacle_free():
    params, lay, robot = _params(), E.layout(), RobotModel(O.fk_batch)
    rng = np.random.default_rng(5)
    scenes = [_box_scene(rng, 4, rotated=0.5), ([], []), _box_scene(rng, 2)]
    rollout_scene = np.array([-1, 1, 0, -1, 1, 2])
    R = len(rollout_scene)
    _, _, S0 = _rollouts(rng, R, robot, params, lay)
    S = S0.copy()
    mixed = ES.prepare_scenes(N, S, np.zeros((R, 44 * N + 6)), scenes, rollout_scene)
    for r in range(R):
        free = rollout_scene[r] in (-1, 1)
        single, S1 = _single(S0[r], None if free else scenes[rollout_scene[r]])
        _assert_bitwise(mixed, S, r, single, S1)
        if free:
            assert (np.abs(mixed[3][r][515:785].reshape(6, 3, 15)).sum(axis=1) > 0).sum(axis=1).tolist() == [6] * 6
    # a table without any obstacle at all
    S = S0.copy()
    mixed = ES.prepare_scenes(N, S, np.zeros((R, 44 * N + 6)), [([], []), ([], [])], np.array([0, 1, -1, 0, 1, -1]))
    for r in range(R):
        _assert_bitwise(mixed, S, r, *_single(S0[r], None))


def _shell_scene(centre, radius=0.3, half=0.03):
    """14 small boxes on a sphere around `centre` (the axes and the diagonals): none of them hides another one from the centre, so a
    collision point there needs 6 + 14 rows -- more than max_set_size."""
    dirs = [np.array(d, float) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    dirs += [np.array([sx, sy, sz], float) / np.sqrt(3) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    from boundplanner_amd import scenes
    return scenes.boxes_to_sets([np.concatenate((centre + radius * d - half, centre + radius * d + half)) for d in dirs])


def test_a_scene_with_too_many_rows_freezes_only_its_own_rollouts():
    params, lay, robot = _params(), E.layout(), RobotModel(O.fk_batch)
    rng = np.random.default_rng(33)
    R = 9
    mpcs, node, S0 = _rollouts(rng, R, robot, params, lay)
    col = O.fk_batch(node[4][0][None])["col_pts"][0]                  # the shell goes around the last collision point of rollout 4
    scenes = [_box_scene(rng, 6, rotated=0.5), _shell_scene(col[5]), _box_scene(rng, 2)]
    rollout_scene = np.array([0, 2, 0, -1, 1, 2, 0, 2, 0])
    S = S0.copy()
    mixed = ES.prepare_scenes(N, S, np.zeros((R, 44 * N + 6)), scenes, rollout_scene)
    hit, clear = 0, 0
    for r in range(R):
        scene = scenes[rollout_scene[r]] if rollout_scene[r] >= 0 else ([], [])
        single, S1 = _single(S0[r], scene)
        _assert_bitwise(mixed, S, r, single, S1)
        p_host = _host_prepare(mpcs[r], node[r], scene) if rollout_scene[r] >= 0 else 0
        dead = state_view(lay, S[r])["dead"][0]
        assert dead == (2.0 if p_host is None else 0.0), r       # frozen exactly where the host raises
        hit += p_host is None; clear += p_host is not None
    assert state_view(lay, S[4])["dead"][0] == 2.0 and hit >= 1 and clear >= 1


def test_abi_declares_the_scene_entries():
    """The two entries in include/boundmpc.h and in load_library, with matching argument counts."""
    import __graft_entry__ as ge
    from boundplanner_amd import solver
    ge.build()
    hdr = open(os.path.join(ROOT, "include", "boundmpc.h")).read()
    lib = solver.load_library()
    for name in ("bmpc_loop_set_scenes", "bmpc_loop_set_rollout_scenes"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        assert name in solver.EXPORTS
        assert len(getattr(lib, name).argtypes) == len(m.group(1).split(",")), name
