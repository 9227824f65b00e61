"""The planted runs of tests/test_loop_switch.py on the MI355X: all scripts of tests/golden/switch_cases.npz as ONE batch of the
device-resident loop (bmpc_loop_k_prepare / bmpc_loop_k_finish), one rollout per script, in lock step.  No solve is launched:
per step prepare -> problem() against the reference's solver arguments -> set_solution from the fixture -> finish -> download,
and every field of every rollout of every step is compared with what the reference carried (integers and flags exactly, floats
to the 1e-9 of tests/test_device_loop.py), the MPCData record of every rollout with the host mirror's.  The per-scene kernels
(set_scenes with one empty scene) and two rollouts run alone must give the batch's bits."""
import numpy as np
import pytest

import switch_cases_lib as SC
from boundplanner_amd.params import Params, get_default_params

pytestmark = pytest.mark.gpu

BIG = lambda a: np.nan_to_num(np.asarray(a, float), posinf=1e20, neginf=-1e20)


class Batch:
    """The scripts `rows` of the fixture through one DeviceLoop; keeps, per step, the problem the prepare kernel wrote, the
    records and the state after the finish kernel.  The first batch builds the rollouts from host mirrors that take the same
    steps (and notes how the records compare with theirs); a batch `like` another starts from that one's serialised states."""

    def __init__(self, be, cases, rows, scenes=False, like=None):
        import oracle_lib as O
        from boundplanner_amd.device_loop import DeviceLoop, state_view
        from boundplanner_amd.mpc_node import MPCNode
        from boundplanner_amd.robot_model import RobotModel
        from test_closed_loop import ReplaySolver
        from test_device_loop import compare_record_with_host_mirror, via_lists
        N = int(cases["N"])
        base = get_default_params()
        params = Params(n=N, dt=base.dt, build=False, weights=base.weights, nr_segs=base.nr_segs)
        rows = list(rows)
        self.scripts = [SC.Script(cases, s) for s in rows]
        R = len(rows)
        self.loop = loop = DeviceLoop(be, R)
        self.lay, self.LOG = loop.lay, loop.LOG
        if scenes:
            loop.set_scenes([([], [])], np.zeros(R, int))
        if like is None:
            shadows = [MPCNode(g["in_q"][0], RobotModel(O.fk_batch), (lambda g: lambda n, dt: ReplaySolver(g, tol=1e-9))(g), params=params)
                       for g in self.scripts]
            for r, sh in enumerate(shadows):
                loop.set_rollout(r, sh.mpc, sh.q, sh.dq, sh.ddq, sh.jerk, sh.qf, sh.v, sh.p_lie)
            self.installed = [(loop.state.copy(), loop.prev.copy())]
        else:
            loop.state[:], loop.prev[:] = like.installed[0][0][rows], like.installed[0][1][rows]
        loop.upload()
        loop.set_record(range(R))
        n_steps, n_update = cases["in_q"].shape[1], int(cases["n_update"])
        self.problems, self.states, self.prevs, self.recs, self.logs, self.mirror_error = [], [], [], [], [], None
        for k in range(n_steps):
            if k == n_update:
                # the paths are installed by set_rollout at the re-plan step; warm start, slacks0 and error count carry over (a15)
                V = loop.download()
                if like is None:
                    keep = {f: V[f].copy() for f in ("slacks0", "error_count", "has_prev", "q", "dq", "ddq", "jerk", "v", "p_lie")}
                    prev = loop.prev.copy()
                    for r, (g, sh) in enumerate(zip(self.scripts, shadows)):
                        sh.update_reference(*via_lists(g), [])
                        loop.set_rollout(r, sh.mpc, keep["q"][r], keep["dq"][r], keep["ddq"][r], keep["jerk"][r], keep["q"][r], keep["v"][r], keep["p_lie"][r])
                        W = state_view(loop.lay, loop.state[r])
                        for f in ("slacks0", "error_count", "has_prev"):
                            W[f][:] = keep[f][r]
                    loop.prev[:] = prev
                    self.installed.append((loop.state.copy(), loop.prev.copy()))
                else:
                    loop.state[:], loop.prev[:] = like.installed[1][0][rows], like.installed[1][1][rows]
                loop.upload()
            loop.prepare()
            self.problems.append(loop.problem())
            loop.set_solution(np.array([g["call_x"][k] for g in self.scripts]), np.array([int(g["iters"][k]) for g in self.scripts]),
                              np.array([int(g["status"][k]) for g in self.scripts]), np.array([float(g["viol"][k]) for g in self.scripts]))
            self.logs.append(loop.finish())
            self.recs.append(loop.records().copy())
            loop.download()
            self.states.append(loop.state.copy())
            self.prevs.append(loop.prev.copy())
            if like is None:
                for r, (g, sh) in enumerate(zip(self.scripts, shadows)):
                    sh.step()
                    try:
                        compare_record_with_host_mirror(self.recs[-1][0, r], N, sh, (g.name, k), set_tol=1e-9, need_sets=True)
                    except AssertionError as e:          # kept for the test that asks: a fixture does not assert
                        self.mirror_error = self.mirror_error or e
        loop.close()


@pytest.fixture(scope="module")
def cases(golden_dir):
    return SC.load(golden_dir)


@pytest.fixture(scope="module")
def backend(cases):
    from boundplanner_amd.solver import HipBoundMPC
    return HipBoundMPC(int(cases["N"]), max_batch=len(cases["script"]))


@pytest.fixture(scope="module")
def batch(backend, cases):
    R = len(cases["script"])
    assert 16 < R and R % 64 != 0              # some tens of rollouts, the last wavefront partly filled
    return Batch(backend, cases, range(R))


def test_kernels_replay_the_planted_runs(batch, cases):
    from boundplanner_amd.device_loop import state_view
    from test_device_loop import compare_state_with_trace
    loop = batch
    worst = {}
    for k in range(len(batch.states)):
        assert batch.recs[k].shape[:2] == (1, len(batch.scripts))
        for r, g in enumerate(batch.scripts):
            for name, mine in zip(("x0", "lbx", "ubx", "p"), batch.problems[k]):
                d = np.abs(mine[r] - BIG(g["call_" + name][k])).max()
                worst[name] = max(worst.get(name, 0.0), d)
                assert d < 1e-9, (g.name, k, name, d)
            compare_state_with_trace(state_view(loop.lay, batch.states[k][r]), g, k, worst, where=g.name)
            assert abs(batch.logs[k][r, loop.LOG["phi"]] - g["phi_current"][k][0]) < 1e-9
            assert int(batch.logs[k][r, loop.LOG["switch"]]) == int(g["switch"][k]) and int(batch.logs[k][r, loop.LOG["split1"]]) == int(g["split_idxs"][k][1])
    assert not np.array([s[:, loop.lay["dead"][0]] for s in batch.states]).any()
    if batch.mirror_error is not None:          # the MPCData record of every rollout and step against the host mirror's, set fields included
        raise batch.mirror_error
    print("max deviation from the planted runs:", {k: float(f"{v:.2e}") for k, v in worst.items()})


def _same(a, b, rows, what):
    for k in range(len(a.states)):
        for name, x, y in zip(("x0", "lbx", "ubx", "p"), a.problems[k], b.problems[k]):
            assert np.array_equal(x, y[rows]), (what, k, name)
        assert np.array_equal(a.states[k], b.states[k][rows]), (what, k, "state")
        assert np.array_equal(a.prevs[k], b.prevs[k][rows]), (what, k, "warm start")
        assert np.array_equal(a.recs[k], b.recs[k][:, rows]), (what, k, "record")
        assert np.array_equal(a.logs[k], b.logs[k][rows]), (what, k, "log")


def test_per_scene_kernels_give_the_same_bits(batch, backend, cases):
    R = len(cases["script"])
    _same(Batch(backend, cases, range(R), scenes=True, like=batch), batch, np.arange(R), "one empty scene for every rollout")


def test_rollouts_alone_give_the_same_bits(batch, backend, cases):
    names = [str(n) for n in cases["script"]]
    for r in (names.index("a_same_step"), len(names) - 1):
        _same(Batch(backend, cases, [r], like=batch), batch, np.array([r]), f"rollout {names[r]} alone")
