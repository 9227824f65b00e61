"""Reference paths installed on the GPU (DeviceLoop.replan_batch / init_rollouts: bmpc_loop_replan, bmpc_loop_init_rollouts,
bmpc_loop_k_install) against the host installation (set_rollout / replan between download() and upload()).  The arithmetic is
pinned by the CPU build of the same source in tests/test_device_loop_replan.py; here: the kernel on gfx950, the staging, the
rollout list, and a closed loop that starts from device-installed paths."""
import ctypes

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

import replan_cases_lib as C
from boundplanner_amd.device_loop import pack_plans
from boundplanner_amd.params import Params, get_default_params

pytestmark = pytest.mark.gpu

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)


def _params(N):
    base = get_default_params()
    return Params(n=N, dt=base.dt, build=False, weights=base.weights, nr_segs=base.nr_segs)


def _host_installed_loop(be, R, q_start, params):
    from boundplanner_amd.batch_node import BatchMPCNode
    from boundplanner_amd.device_loop import DeviceLoop
    node = BatchMPCNode(be, q_start, params)
    loop = DeviceLoop(be, R)
    for r in range(R):
        loop.set_rollout(r, node.mpcs[r], node.q[r], node.dq[r], node.ddq[r], node.jerk[r], node.qf[r], node.v[r], node.p_lie[r])
    loop.upload()
    return node, loop


def _q_start(R, seed):
    from boundplanner_amd import scenes
    _, q0, _, _ = scenes.example_scene()
    return q0 + np.random.default_rng(seed).uniform(-0.15, 0.15, size=(R, 7))


def test_replan_batch_of_a_scattered_subset():
    """R = 96 (more than one wavefront, no multiple of 64), 37 rollouts in no order with the path shapes of the CPU test: those
    equal the host replan, everything else on the device -- the other 59 states, all 96 warm starts -- is bitwise untouched."""
    from boundplanner_amd.solver import HipBoundMPC
    N, R = 6, 96
    params = _params(N)
    be = HipBoundMPC(N, max_batch=R)
    node, loop = _host_installed_loop(be, R, _q_start(R, 7), params)
    loop.run(1, log=False)                   # one step on the start-up path: warm starts, velocities and slacks that are not zero
    V = loop.download()
    state0, prev0 = loop.state.copy(), loop.prev.copy()
    assert (state0[:, loop.lay["has_prev"][0]] == 1).all() and np.abs(prev0).max() > 0
    rollouts = np.random.default_rng(1).permutation(R)[:37]
    assert (np.diff(rollouts) < 0).any() and rollouts.max() >= 64
    names = list(C.CASES)
    plans = [C.make_plan(names[i % len(names)], 500 + i, V["p_lie"][r][:3].copy(), Rot.from_rotvec(V["p_lie"][r][3:]).as_matrix())
             for i, r in enumerate(rollouts)]
    assert {len(p[0]) for p in plans} >= {2, 3, 4, 5, 8}
    for r, plan in zip(rollouts, plans):                         # the specification: host replan of the downloaded states
        loop.replan(int(r), node.mpcs[r], *C.copy_plan(plan))
    expect = loop.state.copy()
    loop.replan_batch(rollouts, plans)
    loop.download()
    others = np.setdiff1d(np.arange(R), rollouts)
    dev = np.abs(loop.state[rollouts] - expect[rollouts]).max()
    print(f"replan_batch vs host replan, 37 rollouts: max deviation {dev:.2e}; install kernel {loop.ms_install:.3f} ms")
    assert dev < 1e-9, dev
    assert (np.abs(loop.state[rollouts] - state0[rollouts]).max(axis=1) > 1e-3).all()       # (they did get a new path)
    assert (loop.state[others] == state0[others]).all()
    assert (loop.prev == prev0).all()
    loop.replan_batch([], [])                                    # count = 0: a no-op
    loop.close()


def test_closed_loop_from_device_installed_paths():
    """init_rollouts + start-up step + replan_batch + 14 tracked steps against the same on a host-installed loop: the scenario,
    sizes and criteria of test_device_loop_gpu.py::test_device_loop_tracks_host_loop (same solver, arguments equal to rounding)."""
    from boundplanner_amd.device_loop import DeviceLoop
    from boundplanner_amd.solver import HipBoundMPC
    from test_device_loop_gpu import _scenario
    N, R, steps = 10, 12, 14
    params = _params(N)
    be_h, be_d = HipBoundMPC(N, max_batch=R), HipBoundMPC(N, max_batch=R)
    q_start, plans = _scenario(be_h, R, N, 4096)
    plan_of = lambda r, p_lie: ([p_lie[:3].copy(), plans[r]["goal"].copy()], [m.copy() for m in plans[r]["r_via"]], [b.copy() for b in plans[r]["bp1"]],
                                [b.copy() for b in plans[r]["br1"]], [e.copy() for e in plans[r]["erb"]], [a.copy() for a in plans[r]["a"]],
                                [b.copy() for b in plans[r]["b"]])
    # host-installed loop
    node, host = _host_installed_loop(be_h, R, q_start, params)
    host.run(1)
    Vh = host.download()
    for r in range(R):
        host.replan(r, node.mpcs[r], *plan_of(r, Vh["p_lie"][r]))
    host.upload()
    # device-installed loop: no host BoundMPC objects, only p_lie comes back for the plans
    loop = DeviceLoop(be_d, R)
    loop.init_rollouts(q_start, params.weights)
    loop.run(1)
    Vd = loop.download()
    assert np.abs(Vd["p_lie"] - Vh["p_lie"]).max() < 1e-9
    loop.replan_batch(np.arange(R), [plan_of(r, Vd["p_lie"][r]) for r in range(R)])
    host.prepare(); loop.prepare()
    for name, a, b in zip(("x0", "lbx", "ubx", "p"), host.problem(), loop.problem()):
        d = np.abs(a - b).max()
        print(f"first tracked step, {name}: max deviation {d:.2e}")
        assert d < 1e-9, (name, d)
    dmax = 0.0
    for k in range(steps):
        lh, ld = host.run(1)[0], loop.run(1)[0]
        L = loop.LOG
        dmax = max(dmax, np.abs(ld[:, L["q"]] - lh[:, L["q"]]).max(), np.abs(ld[:, L["p_lie"]] - lh[:, L["p_lie"]]).max(),
                   np.abs(ld[:, L["phi"]] - lh[:, L["phi"]]).max())
        assert (ld[:, L["iters"]] == lh[:, L["iters"]]).mean() > 0.9, k
        assert (ld[:, L["split1"]] == lh[:, L["split1"]]).all(), k
    print(f"device-installed vs host-installed loop over {steps} steps: max deviation {dmax:.2e}")
    assert dmax < 1e-6, dmax
    assert (ld[:, L["phi"]] > 0.05).all()                 # the rollouts actually move along their paths
    host.close(); loop.close()


def test_misuse_is_refused_before_anything_runs():
    """A duplicate rollout, an index equal to R, n_pts = 9, a null pointer: rc 1 with a message, checked on the host before any
    launch -- the device state afterwards is bitwise what it was."""
    from boundplanner_amd.solver import HipBoundMPC
    N, R = 6, 8
    be = HipBoundMPC(N, max_batch=R)
    node, loop = _host_installed_loop(be, R, _q_start(R, 9), _params(N))
    loop.download()
    state0, prev0 = loop.state.copy(), loop.prev.copy()
    plans = [C.make_plan("n3", i, np.zeros(3), np.eye(3)) for i in range(3)]
    n_pts, *arrs = pack_plans(plans)
    I = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(_ip)
    P = [a.ctypes.data_as(_dp) for a in arrs]

    def refused(rollouts, npts, ptrs, what):
        rc = loop.lib.bmpc_loop_replan(loop._l, len(rollouts), I(rollouts), I(npts), *ptrs)
        msg = loop.lib.bmpc_loop_last_error(loop._l).decode()
        assert rc == 1 and what in msg, (rc, msg)

    refused([1, 4, 1], n_pts, P, "twice")
    refused([1, R, 2], n_pts, P, "out of range")
    refused([1, -1, 2], n_pts, P, "out of range")
    refused([1, 2, 3], [3, 9, 3], P, "via points")
    refused([1, 2, 3], [3, 1, 3], P, "via points")
    refused([1, 2, 3], n_pts, P[:3] + [None] + P[4:], "bad arguments")
    with pytest.raises(RuntimeError, match="twice"):
        loop.replan_batch([5, 5], plans[:2])
    q0 = np.zeros((2, 7)); w = np.ones(11)
    assert loop.lib.bmpc_loop_init_rollouts(loop._l, R - 1, 2, q0.ctypes.data_as(_dp), w.ctypes.data_as(_dp)) == 1
    assert loop.lib.bmpc_loop_last_error(loop._l).decode()
    assert loop.lib.bmpc_loop_init_rollouts(loop._l, 0, 2, None, w.ctypes.data_as(_dp)) == 1
    loop.download()
    assert (loop.state == state0).all() and (loop.prev == prev0).all()
    loop.close()
