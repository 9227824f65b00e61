"""The orientation block of the device loop on the MI355X (kernels bmpc_loop_k_prepare, bmpc_loop_k_prepare_scenes, bmpc_loop_k_finish)
against tests/orientation_lib.py, the extended-precision reference written from the definitions -- through the product entries only:
DeviceLoop.state / upload / prepare / problem / download, then set_solution / finish / download.  One loop at N = 6, one rollout per
case of orientation_lib.rollout_cases (error angles 0 .. half turn, the Euler split's pitch next to and at +-90 deg, the +pi rule,
end-effector orientations at a half turn, random and trivial frames per segment; for loop_finish |omega| on both sides of 1e-4 and
a rotation reference crossing the half turn); the count is no multiple of 64.  Bounds: 32 x the host mirror's worst figure per
quantity and family (orientation_lib.HOST_WORST) plus the derived terms stated there."""
import numpy as np
import pytest

import orientation_lib as L
from boundplanner_amd.params import Params, get_default_params

pytestmark = pytest.mark.gpu
N = 6


def _states(lay):
    import oracle_lib as O
    from boundplanner_amd.device_loop import state_view
    from boundplanner_amd.robot_model import RobotModel
    from test_device_loop import _rollout_state
    base = get_default_params()
    params = Params(n=N, dt=base.dt, build=False, weights=base.weights, nr_segs=base.nr_segs)
    robot, q = RobotModel(O.fk_batch), np.array(L.Q_ALL)
    Ree = O.fk_batch(q)["ee_rot"]
    bases = [_rollout_state(lay, params, robot, q[i], q[i])[1] for i in range(len(q))]
    cases = L.rollout_cases()
    S = np.array([bases[c["qi"]] for c in cases])
    for r, c in enumerate(cases):
        L.install(state_view(lay, S[r]), c, Ree[c["qi"]])
    return cases, S, Ree


def _same(a, b):
    """Bitwise, not-a-numbers included (the dual basis of a singular [g h k])."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _step(be, S, cases, scenes=False):
    """upload -> prepare -> problem / download -> planted solution -> finish -> download, on a loop of len(S) rollouts."""
    from boundplanner_amd.device_loop import DeviceLoop, state_view
    R = len(S)
    loop = DeviceLoop(be, R)
    try:
        if scenes:          # a table of one empty scene: the per-scene kernel, obstacle-free collision sets as on the shared path
            loop.set_scenes([([], [])], np.zeros(R, int))
        loop.state[:] = S
        loop.upload()
        loop.prepare()
        x0, lbx, ubx, p = loop.problem()
        loop.download()
        S1 = loop.state.copy()
        x = np.array([L.plant(N, x0[r], state_view(loop.lay, S1[r]), cases[r]) for r in range(R)])
        loop.set_solution(x, np.zeros(R, int), np.zeros(R, int), np.zeros(R))
        log = loop.finish()
        loop.download()
        S2 = loop.state.copy()
    finally:
        loop.close()
    return dict(x0=x0, lbx=lbx, ubx=ubx, p=p, S1=S1, S2=S2, log=log)


@pytest.fixture(scope="module")
def batch():
    from boundplanner_amd.device_loop import DeviceLoop
    from boundplanner_amd.solver import HipBoundMPC
    be = HipBoundMPC(N)
    probe = DeviceLoop(be, 1)
    lay = probe.lay
    probe.close()
    cases, S, Ree = _states(lay)
    assert len(cases) % 64 != 0 and len(cases) > 192          # several wavefronts, the last one ragged
    return dict(be=be, lay=lay, cases=cases, S=S, Ree=Ree, out=_step(be, S, cases))


def test_orientation_block_against_the_reference(batch):
    from boundplanner_amd.device_loop import state_view
    lay, cases, out = batch["lay"], batch["cases"], batch["out"]
    W, left_out, fams = L.Worst(), {"structured": [0, 0], "random": [0, 0]}, set()
    for r, c in enumerate(cases):
        V0, V1, V2 = (state_view(lay, a[r]) for a in (batch["S"], out["S1"], out["S2"]))
        L.check_prepare_one(W, c, V0, V1, out["p"][r], batch["Ree"][c["qi"]], left_out)
        assert (out["x0"][r][31 * N:34 * N].reshape(3, N) == V1["p_lie"][3:, None]).all()          # the cold start carries log R_ee
        assert V2["accept"][0] == 1.0 and V2["dead"][0] == 0.0
        L.check_finish_one(W, c, V1, V2)
        fams.update(L.fam_of(t) for t in c["tags"])
    L.check_left_out(left_out)
    assert fams == {"small", "mid", "half", "near", "lock", "pi_outer"}
    W.report(f"MI355X, prepare + finish kernels over {len(cases)} rollouts (dual basis left out: {left_out}): worst deviation / bound")
    assert not W.failures(), W.failures()


def test_scene_table_path_is_bitwise_the_shared_path(batch):
    out = batch["out"]
    other = _step(batch["be"], batch["S"], batch["cases"], scenes=True)
    for k in ("x0", "lbx", "ubx", "p", "S1", "S2", "log"):
        assert _same(out[k], other[k]), k


def test_a_rollout_alone_is_bitwise_what_it_is_in_the_batch(batch):
    cases, out = batch["cases"], batch["out"]
    lock = next(r for r, c in enumerate(cases) if c["kind"] == "random" and L.fam_of(c["tags"][0]) == "lock")
    half = next(r for r, c in enumerate(cases) if c["qfam"] == "half" and L.fam_of(c["tags"][0]) == "half" and r > 64)
    for r in (lock, half):
        alone = _step(batch["be"], batch["S"][r:r + 1], cases[r:r + 1])
        for k in ("x0", "lbx", "ubx", "p", "S1", "S2", "log"):
            assert _same(out[k][r], alone[k][0]), (r, k)
