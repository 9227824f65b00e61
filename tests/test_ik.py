"""Batched inverse kinematics (bmpc_ik.hpp) on the CPU build of the kernel body (tests/emu/emu_ik.cpp), checked against the oracle's
forward kinematics with central differences (tests/ik_check_lib.py): residuals, bounds and first-order optimality -- never q against
another solver, since 7 joints against 6 task dimensions leave a manifold of solutions."""
import logging

import numpy as np
import pytest

import emu_ik_lib as E
import ik_check_lib as C
import oracle_lib as O
from boundplanner_amd import robots

LO, HI = C.limits(robots.IIWA14)


def test_model_is_the_gauss_newton_model_of_the_residual():
    """gh = grad J / 2 and H = Jr^T Jr for the 12-vector residual (p - pd, vec(M - I)), Jr by central differences of the oracle."""
    rng = np.random.default_rng(7)
    q = C.sample_box(rng, 8, robots.IIWA14)
    pd = rng.normal(0.0, 0.5, (8, 3))
    rd = C.random_rotations(rng, 8)
    g = C.grad(q, pd, rd)
    for b in range(8):
        f, gh, H = E.model(q[b], pd[b], rd[b])
        assert abs(f - C.cost(q[b:b + 1], pd[b:b + 1], rd[b:b + 1])[0]) <= 1e-12 * max(1.0, f)
        assert np.abs(2 * gh - g[b]).max() <= 1e-7

        def res(x):
            o = O.fk_batch(x[None])
            return np.concatenate([o["ee_pos"][0] - pd[b], (o["ee_rot"][0] @ rd[b].T - np.eye(3)).ravel()])
        Jr = np.stack([(res(q[b] + C.H_FD * e) - res(q[b] - C.H_FD * e)) / (2 * C.H_FD) for e in np.eye(7)], 1)
        assert np.abs(Jr.T @ Jr - H).max() <= 1e-7


def test_reachable_targets():
    pd, rd, q0, _ = C.reachable(np.random.default_rng(0), 512)
    r = E.ik(pd, rd, q0)
    assert C.reached(r).mean() >= 0.99, np.bincount(r["status"])
    assert ((r["q"] >= LO) & (r["q"] <= HI)).all()
    pe, re = C.errors(r["q"], pd, rd)                      # the kernel's error figures against the oracle's
    assert np.abs(pe - r["pos_err"]).max() <= 1e-9 and np.abs(re - r["rot_err"]).max() <= 1e-9
    assert (r["seed"] == 0).all() and (r["iters"] <= 500).all()


def test_active_bounds():
    pd, rd, q0 = C.beyond_bound(np.random.default_rng(1), 256)
    r = E.ik(pd, rd, q0)
    n_active = C.check_active_bounds(r, pd, rd, LO, HI)
    print(f"instances ending at a bound: {n_active} / 256; status counts {np.bincount(r['status'], minlength=4)}")
    assert n_active >= 1


def test_unreachable_targets():
    """Stationary where the kernel claims it (status 0 or 2), never worse than the start, few at max_iter.  Against scipy's L-BFGS-B
    from the same seed: where both end within 1e-3 in q the costs agree to 1e-8 relative.  The minimisers are not isolated (the
    self-motion of the stretched arm), so two solvers often end apart in q at the same cost: the basin fraction is printed, and the
    cost agreement is asserted for at least half of the instances."""
    from scipy.optimize import minimize
    pd, rd, q0 = C.unreachable(np.random.default_rng(2), 64)
    r = E.ik(pd, rd, q0)
    J, J0 = C.cost(r["q"], pd, rd), C.cost(q0, pd, rd)
    assert (J <= J0).all()
    assert np.abs(J - r["cost"]).max() <= 1e-12 * J.max()
    pg = C.proj_grad(r["q"], C.grad(r["q"], pd, rd), LO, HI)
    claimed = r["status"] != 1
    assert (pg[claimed] <= 1e-6).all(), pg[claimed].max()
    assert claimed.mean() >= 0.9
    same, agree = 0, 0
    for b in range(64):
        fun = lambda x: C.cost(x[None], pd[b:b + 1], rd[b:b + 1])[0]
        jac = lambda x: C.grad(x[None], pd[b:b + 1], rd[b:b + 1])[0]
        s = minimize(fun, q0[b], jac=jac, method="L-BFGS-B", bounds=list(zip(LO, HI)), options=dict(ftol=1e-16, gtol=1e-10, maxiter=3000))
        rel = abs(s.fun - J[b]) / J[b]
        if np.abs(s.x - r["q"][b]).max() <= 1e-3:
            same += 1
            assert rel <= 1e-8
        agree += rel <= 1e-8
    print(f"same basin as L-BFGS-B: {same / 64:.2f}; same cost (1e-8 rel): {agree / 64:.2f}")
    assert agree / 64 >= 0.5


def test_multi_start():
    rng = np.random.default_rng(3)
    pd, rd, q0, _ = C.reachable(rng, 256)
    pb, rb, qb = C.behind(rng, 256)
    pd, rd, q0 = np.concatenate([pd, pb]), np.concatenate([rd, rb]), np.concatenate([q0, qb])
    r1, r16 = E.ik(pd, rd, q0, n_seeds=1), E.ik(pd, rd, q0, n_seeds=16)
    assert (r16["cost"] <= r1["cost"]).all()
    w = r16["seed"] == 0
    for k in r1:
        assert np.array_equal(r16[k][w], r1[k][w]), k
    assert ((r16["q"] >= LO) & (r16["q"] <= HI)).all()
    ok1, ok16 = C.reached(r1)[256:].sum(), C.reached(r16)[256:].sum()
    print(f"targets behind the robot from q0 = 0 reached: 1 seed {ok1} / 256, 16 seeds {ok16} / 256")
    assert ok16 > ok1


def test_more_seeds_never_cost_more():
    """Targets no seed can reach, n_seeds = 1, 2, ..., 64: the seeds of a smaller call are the first ones of a larger call, so on
    these targets the winning cost does not rise (a converged seed outranks a lower-cost stalled one, so this is not a theorem)."""
    pd, rd, q0 = C.unreachable(np.random.default_rng(4), 4)
    r = E.ik(pd, rd, q0, n_seeds=64)
    rs = [E.ik(pd, rd, q0, n_seeds=n) for n in (1, 2, 4, 8, 16, 32)]
    for a, b in zip(rs, rs[1:] + [r]):
        assert (b["cost"] <= a["cost"]).all()


def test_gen3_unlimited_joints():
    O.set_robot(robots.GEN3)
    try:
        lo, hi = C.limits(robots.GEN3)
        pd, rd, q0, _ = C.reachable(np.random.default_rng(5), 512, robots.GEN3)
        r = E.ik(pd, rd, q0, robot=robots.GEN3)
        assert C.reached(r).mean() >= 0.99, np.bincount(r["status"])
        assert ((r["q"] >= lo) & (r["q"] <= hi)).all()
        pe, re = C.errors(r["q"], pd, rd)                  # the oracle's error figures of the reached instances
        ok = C.reached(r)
        assert pe[ok].max() <= 1.5e-8 and re[ok].max() <= 1.5e-8
        assert np.abs(pe - r["pos_err"]).max() <= 1e-9
    finally:
        O.set_robot(None)


def test_nan_input_is_status_3_for_that_instance_only():
    pd, rd, q0, _ = C.reachable(np.random.default_rng(6), 8)
    pd[3, 1] = np.nan
    r = E.ik(pd, rd, q0, n_seeds=4)
    assert r["status"][3] == 3 and (np.delete(r["status"], 3) == 0).all()


def test_robot_model_inverse_kinematics(caplog):
    from boundplanner_amd.robot_model import RobotModel
    pd, rd, q0, _ = C.reachable(np.random.default_rng(8), 4)
    rm = RobotModel(fk_fn=lambda q, dq=None: O.fk_batch(q, dq), ik_fn=E.ik)
    with caplog.at_level(logging.INFO, logger="boundplanner_amd.robot_model"):
        for b in range(4):
            q = rm.inverse_kinematics(pd[b], rd[b], q0[b])
            assert q.shape == (7,)
            pe, re = C.errors(q[None], pd[b:b + 1], rd[b:b + 1])
            assert pe[0] <= 1e-8 and re[0] <= 1e-8
            np.testing.assert_allclose(rm.fk_pos(q), pd[b], atol=1e-8)
    assert any("Position error" in m for m in caplog.messages)
    rb = rm.inverse_kinematics_batch(pd, rd, q0, n_seeds=2)
    assert rb["q"].shape == (4, 7) and (rb["status"] == 0).all()
    # an unreachable target: the reference prints an error and still returns q
    pu, ru, qu = C.unreachable(np.random.default_rng(9), 1)
    with caplog.at_level(logging.WARNING, logger="boundplanner_amd.robot_model"):
        q = RobotModel(fk_fn=lambda q, dq=None: O.fk_batch(q, dq), ik_fn=lambda *a, **k: E.ik(*a, max_iter=3, **k)).inverse_kinematics(
            pu[0], ru[0], qu[0])
    assert q.shape == (7,) and any("No convergence" in m for m in caplog.messages)


def test_default_ik_backend_is_created_lazily_and_has_no_cpu_fallback():
    import torch
    from boundplanner_amd.robot_model import RobotModel
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rm = RobotModel(fk_fn=lambda q, dq=None: O.fk_batch(q, dq))       # constructing does not touch the IK backend
    with pytest.raises(RuntimeError):
        rm.inverse_kinematics(np.zeros(3), np.eye(3), np.zeros(7))
