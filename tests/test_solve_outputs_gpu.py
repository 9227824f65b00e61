"""What a solve of the HIP kernels returns when it stops short of a solution, pinned to the full-space NLP at the returned point
(MI355X; tests/test_solve_outputs.py is the CPU half, tests/solve_outputs_lib.py documents the reference, the families of points, the
checks and the bounds).

bmpc_solve on handles with max_iter = 0, 1, 2, 5: bmpc_k_out, bmpc_k_fin, bmpc_k_mult, bmpc_k_mult_sweep write x, g, f, viol, lam_g,
lam_x of points that are no solutions.  The handle takes no pool of fewer than 64 slots: the streamed run repeats the batch until
it has more rows than a pool of 64.  The last test is the device loop's view of the same number: the viol of a step's log is the
viol of bmpc_solve on the step's problem, and error_count follows it.  The run prints its worst figures per case.

Reads the oracle library and the scene generator only.
"""
import numpy as np
import pytest

import oracle_lib as O
import solve_outputs_lib as L

pytestmark = pytest.mark.gpu
POOL = 64


@pytest.fixture
def solve():
    """solve(N, x0, lbx, ubx, p, max_iter=, want_g=, want_lam=, robot=None, pool_slots=0): a handle per (N, max_iter, robot, pool)"""
    from boundplanner_amd.solver import HipBoundMPC
    cache = {}

    def run(N, x0, lbx, ubx, p, max_iter, want_g, want_lam, robot=None, pool_slots=0):
        key = (N, max_iter, robot, pool_slots)
        if key not in cache:
            cache[key] = HipBoundMPC(N, max_iter=max_iter, robot=robot, **({"pool_slots": pool_slots} if pool_slots else {}))
        return cache[key].solve_batch(x0, lbx, ubx, p, want_g=want_g, want_lam=want_lam)
    yield run
    for be in cache.values():
        be.close()


def _ids(cases):
    return [f"N{c[0]}-B{c[1]}" + (f"-{c[3]}" if c[3] else "") for c in cases]


@pytest.mark.parametrize("case", L.GPU_CASES, ids=_ids(L.GPU_CASES))
def test_hip_iterates_return_the_nlp_at_their_point(solve, case):
    N, B, _, robot = case
    from boundplanner_amd import robots
    if robot:
        O.set_robot(robots.GEN3)
    try:
        mine = lambda *a, **kw: solve(*a, robot=robot, **kw)
        pool = (lambda *a, **kw: solve(*a, robot=robot, pool_slots=POOL, **kw), POOL)
        L.check_natural(mine, case, f"HIP iterates N={N} B={B}" + (f" ({robot})" if robot else ""), pool=pool)
    finally:
        O.set_robot(None)


@pytest.mark.parametrize("N", L.PLANT_N_GPU)
def test_hip_planted_points(solve, N):
    L.check_planted(solve, N, f"HIP planted points N={N}")


@pytest.mark.parametrize("N", L.WARM_N_GPU)
def test_hip_stopped_warm_starts(solve, N):
    L.check_warm(solve, N, f"HIP stopped warm starts N={N}")


def test_the_device_loop_logs_the_solves_own_viol_and_counts_by_it():
    """R = 8 rollouts at N = 10 whose handle stops after two iterations, from the state a loop on an ordinary handle has reached
    (a warm start and an accepted previous solution each): the step's log holds bitwise the iters, status and viol that bmpc_solve
    returns on the step's own problem -- the loop's solve runs without g --, and error_count rises exactly where the solve has
    failed and viol >= 1e-4, and falls back to zero elsewhere."""
    from boundplanner_amd.batch_node import BatchMPCNode
    from boundplanner_amd.device_loop import DeviceLoop
    from boundplanner_amd.solver import HipBoundMPC
    from test_device_loop_gpu import _params, _scenario
    N, R = 10, 8
    params = _params(N)
    be = HipBoundMPC(N, max_batch=R)
    q_start, plans = _scenario(be, R, N, 4096)
    ref = BatchMPCNode(be, q_start, params)               # only its freshly constructed host objects are used
    first = DeviceLoop(be, R)
    for r in range(R):
        first.set_rollout(r, ref.mpcs[r], ref.q[r], ref.dq[r], ref.ddq[r], ref.jerk[r], ref.qf[r], ref.v[r], ref.p_lie[r])
    first.upload()
    first.run(1)                                           # start-up solve on the trivial path
    V = first.download()
    for r in range(R):
        P = plans[r]
        first.replan(r, ref.mpcs[r], [V["p_lie"][r][:3].copy(), P["goal"]], P["r_via"], P["bp1"], P["br1"], P["erb"], P["a"], P["b"])
    first.upload()
    log = first.run(3)
    assert (log[:, :, first.LOG["error_count"]] == 0).all()
    V = first.download()
    assert (V["has_prev"][:, 0] == 1).all() and (V["error_count"][:, 0] == 0).all()

    short = HipBoundMPC(N, max_iter=2, max_batch=R)
    loop = DeviceLoop(short, R)
    loop.state[:] = first.state
    loop.prev[:] = first.prev
    loop.upload()
    Lg = loop.LOG
    count = np.zeros(R)
    seen = set()
    for step in range(3):
        loop.prepare()
        problem = loop.problem()
        loop.solve()
        log = loop.finish()
        direct = short.solve_batch(*problem)
        assert np.array_equal(log[:, Lg["viol"]], direct["viol"]), step
        assert np.array_equal(log[:, Lg["iters"]], direct["iters"]) and np.array_equal(log[:, Lg["status"]], direct["status"]), step
        failed = (direct["status"] != 0) & (direct["viol"] >= L.ACCEPT)
        count = np.where(failed, count + 1, 0.0)
        assert np.array_equal(log[:, Lg["error_count"]], count), (step, log[:, Lg["error_count"]], count)
        seen |= {(int(s), L.viol_class(float(v))) for s, v in zip(direct["status"], direct["viol"])}
        print(f"device loop step {step}: status {direct['status'].tolist()} viol {direct['viol'].min():.2e} .. {direct['viol'].max():.2e} "
              f"error_count {count.astype(int).tolist()}")
    # the handle did stop solves short, and the steps decide both ways: failed solves that are accepted, and rejected ones
    assert {(1, "accepted"), (1, "rejected")} <= seen, seen
