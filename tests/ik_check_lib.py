"""Independent checks of inverse-kinematics results -- TEST INFRASTRUCTURE ONLY.

J(q) and its gradient come from the oracle's forward kinematics (oracle_lib.fk_batch, pinned to tests/golden/kin.npz) and central
differences; nothing here reuses the kernel's algebra.  Also the target generators the CPU and GPU tests share."""
import numpy as np

import oracle_lib as O
from boundplanner_amd import robots

H_FD = 1e-6


def limits(table):
    return np.array(table["q_lower"], float), np.array(table["q_upper"], float)


def cost(q, pd, rd):
    """J(q) = |p_ee - pd|^2 + |R_ee rd^T - I|_F^2 by the oracle's FK; q [B,7], pd [B,3], rd [B,3,3]."""
    f = O.fk_batch(q)
    e = f["ee_pos"] - pd
    M = f["ee_rot"] @ np.transpose(rd, (0, 2, 1))
    return (e ** 2).sum(1) + ((M - np.eye(3)) ** 2).sum((1, 2))


def grad(q, pd, rd, h=H_FD):
    """Central-difference gradient of cost [B,7]."""
    G = np.zeros_like(q)
    for j in range(7):
        qp, qm = q.copy(), q.copy()
        qp[:, j] += h
        qm[:, j] -= h
        G[:, j] = (cost(qp, pd, rd) - cost(qm, pd, rd)) / (2 * h)
    return G


def proj_grad(q, g, lo, hi):
    """|P(q - g) - q|_inf per instance, P = projection onto [lo, hi]."""
    return np.abs(np.clip(q - g, lo, hi) - q).max(1)


def errors(q, pd, rd):
    """pos_err = |pd - p_ee(q)|, rot_err = |rotvec(R_ee(q) rd^T)| by the oracle's FK and scipy."""
    from scipy.spatial.transform import Rotation as R
    f = O.fk_batch(q)
    pe = np.linalg.norm(pd - f["ee_pos"], axis=1)
    re = np.linalg.norm(R.from_matrix(f["ee_rot"] @ np.transpose(rd, (0, 2, 1))).as_rotvec(), axis=1)
    return pe, re


def sample_box(rng, B, table, margin=0.1):
    """q uniform in the joint box, `margin` inside the limits; unlimited joints uniform in [-pi, pi]."""
    lo, hi = limits(table)
    lo_s = np.where(lo <= -1e19, -np.pi, lo + margin)
    hi_s = np.where(hi >= 1e19, np.pi, hi - margin)
    return rng.uniform(lo_s, hi_s, (B, 7))


def reachable(rng, B, table=robots.IIWA14, sigma=0.3):
    """Targets pd, rd = FK(q*) with q* in the box and seeds clip(q* + N(0, sigma^2)).  The oracle must hold `table`."""
    lo, hi = limits(table)
    qs = sample_box(rng, B, table)
    f = O.fk_batch(qs)
    q0 = np.clip(qs + rng.normal(0.0, sigma, (B, 7)), lo, hi)
    return f["ee_pos"], f["ee_rot"], q0, qs


def beyond_bound(rng, B, table=robots.IIWA14):
    """Targets from q* with one limited joint 0.2 rad beyond one of its limits; seeds: q* projected onto the box plus noise."""
    lo, hi = limits(table)
    qs = sample_box(rng, B, table)
    lim = np.flatnonzero((lo > -1e19) & (hi < 1e19))
    for b in range(B):
        j = rng.choice(lim)
        qs[b, j] = lo[j] - 0.2 if rng.random() < 0.5 else hi[j] + 0.2
    f = O.fk_batch(qs)
    q0 = np.clip(np.clip(qs, lo, hi) + rng.normal(0.0, 0.1, (B, 7)), lo, hi)
    return f["ee_pos"], f["ee_rot"], q0


def random_rotations(rng, B):
    from scipy.spatial.transform import Rotation as R
    return R.random(B, random_state=np.random.RandomState(int(rng.integers(1 << 30)))).as_matrix()


def unreachable(rng, B, table=robots.IIWA14):
    """pd 1.5 m beyond the workspace (the arm reaches ~1.3 m from its shoulder at z = 0.36 m), random rd, seeds in the box."""
    u = rng.normal(size=(B, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    pd = np.array([0.0, 0.0, 0.36]) + (1.3 + 1.5) * u
    return pd, random_rotations(rng, B), sample_box(rng, B, table)


def behind(rng, B):
    """Targets behind the robot (FK of configurations with joint 1 turned by more than 2 rad) and q0 = 0."""
    table = robots.IIWA14
    qs = sample_box(rng, B, table)
    qs[:, 0] = rng.choice([-1.0, 1.0], B) * rng.uniform(2.2, 2.8, B)
    f = O.fk_batch(qs)
    return f["ee_pos"], f["ee_rot"], np.zeros((B, 7))


def reached(r, tol=1e-8):
    return (r["status"] == 0) & (r["pos_err"] <= tol) & (r["rot_err"] <= tol)


def check_active_bounds(r, pd, rd, lo, hi, tol_pg=1e-6):
    """Every instance reached zero cost or is stationary (projected FD gradient <= tol_pg); at an active bound the FD gradient points
    outward.  Returns the number of instances that end with an active bound."""
    q = r["q"]
    lo_b, hi_b = np.broadcast_to(lo, q.shape), np.broadcast_to(hi, q.shape)
    assert ((q >= lo_b) & (q <= hi_b)).all()
    g = grad(q, pd, rd)
    zero = (r["status"] == 0) & (r["cost"] <= 1e-16)
    pg = proj_grad(q, g, lo_b, hi_b)
    bad = ~zero & (pg > tol_pg)
    assert not bad.any(), (np.flatnonzero(bad)[:10], pg[bad][:10], r["status"][bad][:10])
    at_lo, at_hi = q == lo_b, q == hi_b
    assert (g[at_lo] >= -tol_pg).all() and (g[at_hi] <= tol_pg).all()
    return int((at_lo | at_hi).any(1).sum())
