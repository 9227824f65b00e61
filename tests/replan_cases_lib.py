"""Via paths and carried states for the tests of the device loop's path installation (tests/test_device_loop_replan.py and
tests/test_device_loop_replan_gpu.py) -- TEST INFRASTRUCTURE ONLY.  Every case is a function of a start position and orientation,
so that the GPU tests can hang the same shapes on rollouts that are somewhere else."""
import types

import numpy as np
from scipy.spatial.transform import Rotation as R


def _unit(v):
    return v / np.linalg.norm(v)


def _path(rng, p0, r0, n, short=(), same_rot=(), reverse=(), bp1_parallel=(), br1_parallel=()):
    """n via points from (p0, r0).  Segment i (0-based) in `short`: 1e-4 long; in `same_rot`: identity rotation increment; in
    `reverse`: rotates about minus the axis of the segment before; bp1_parallel / br1_parallel: the desired basis vector lies along
    the segment's direction / rotation axis.  Rotation increments are 0.1 .. 2.0 rad: at least 0.05 rad away from pi, where the
    rotation vector is not unique."""
    p, r = [np.array(p0, float)], [np.array(r0, float)]
    axis = None
    for i in range(n - 1):
        d = _unit(rng.normal(size=3)) * rng.uniform(0.08, 0.3)
        if i in short:
            d = _unit(d) * 1e-4 if short[i] == "tiny" else np.zeros(3)
        p.append(p[-1] + d)
        if i in same_rot:
            r.append(r[-1].copy())
            continue
        ang = rng.uniform(0.1, 2.0)
        axis = -axis if (i in reverse and axis is not None) else _unit(rng.normal(size=3))
        r.append(R.from_rotvec(axis * ang).as_matrix() @ r[-1])
    bp1 = [2.0 * (p[i + 1] - p[i]) if i in bp1_parallel else rng.normal(size=3) for i in range(n - 1)]
    br1 = [0.5 * R.from_matrix(r[i + 1] @ r[i].T).as_rotvec() if i in br1_parallel else rng.normal(size=3) for i in range(n - 1)]
    erb = [np.concatenate((rng.uniform(0.2, 1.5, 3), -rng.uniform(0.2, 1.5, 3))) for _ in range(n - 1)]
    a_sets = [rng.normal(size=(15, 3)) for _ in range(n - 1)]
    b_sets = [rng.uniform(0.5, 2.0, 15) for _ in range(n - 1)]
    return p, r, bp1, br1, erb, a_sets, b_sets


# name -> keyword arguments of _path
CASES = {
    "n2": dict(n=2), "n3": dict(n=3), "n5": dict(n=5), "n8": dict(n=8),
    "n4_short_second": dict(n=4, short={1: "tiny"}),               # list entry 1 of dp is entry 0
    "n3_short_first": dict(n=3, short={0: "tiny"}),                # entry 0 is the default [0, 1, 0]
    "n5_short_run": dict(n=5, short={1: "tiny", 2: "tiny"}),       # entries 0, 1, 2 are one object
    "n5_short_late": dict(n=5, short={3: "tiny"}),                 # the padded entries alias an entry that is not normalised
    "n4_pure_rotation": dict(n=4, short={1: "zero"}),              # coincident points, different orientations
    "n2_pure_rotation": dict(n=2, short={0: "zero"}),
    "n4_reversal": dict(n=4, reverse={1, 2}),                      # the rotation reverses the previous axis
    "n4_identity_rot": dict(n=4, same_rot={0, 2}),                 # identity increments: first segment (default axis) and a later one
    "n3_no_motion": dict(n=3, short={1: "zero"}, same_rot={1}),    # neither length nor rotation: arc length 0, dr stays undivided
    "n4_bp1_parallel": dict(n=4, bp1_parallel={0, 2}, br1_parallel={1}),
}


def make_plan(name, seed, p0, r0):
    return _path(np.random.default_rng(seed), p0, r0, **CASES[name])


def copy_plan(plan):
    return tuple([np.array(a, float) for a in lst] for lst in plan)


def host_replan(lay, N, dt, S, prev, mpc, plan):
    """DeviceLoop.replan (the specification) of one rollout without a device: state S, warm start prev -> the new state vector."""
    from boundplanner_amd.device_loop import DeviceLoop
    me = types.SimpleNamespace(lay=lay, state=S[None].copy(), prev=prev[None].copy(), N=N, be=types.SimpleNamespace(opts=types.SimpleNamespace(dt=dt)))
    DeviceLoop.replan(me, 0, mpc, *copy_plan(plan))
    return me.state[0]
