"""Host-side RobotModel with the reference's method names (RobotModel/RobotModel.py:15-267).

The arithmetic is done by a batched kinematics backend `fk_fn(q[B,7], dq[B,7]) -> dict` with
keys ee_pos [B,3], ee_rot [B,3,3], col_pts [B,6,3], jac [B,6,7], dvdq [B,6,7].  The product
backend is the HIP library (`boundplanner_amd.solver.HipBoundMPC.fk`); there is NO CPU fallback
in this package -- tests inject the oracle's FK explicitly.  Inverse kinematics goes through a batched backend
`ik_fn(pd[B,3], rd[B,3,3], q0[B,7], n_seeds) -> dict` (`HipBoundMPC.ik`), created on first use.
"""
import logging

import numpy as np
from scipy.spatial.transform import Rotation as R

from .params import COL_JOINT_SIZES, DQ_LIM, Q_LIM_LOWER, Q_LIM_UPPER, U_MAX


log = logging.getLogger(__name__)


class RobotModel:
    def __init__(self, fk_fn=None, robot=None, ik_fn=None):
        """robot: table of boundplanner_amd.robots (None = iiwa14, RobotModel.py:10 USE_IIWA = True); `fk_fn` must have been
        given the same table (HipBoundMPC(N, robot=...).fk).  ik_fn: batched IK backend for the same table, or None (the HIP
        library's, HipBoundMPC(N, robot=...).ik, created by the first IK call)."""
        if fk_fn is None:
            from .solver import default_fk_fn  # raises loudly when the HIP library is missing
            fk_fn = default_fk_fn()
        self._fk = fk_fn
        self._ik = ik_fn
        self.robot = robot
        if robot is None:
            self.col_joint_sizes = list(COL_JOINT_SIZES)
            self.q_lim_lower, self.q_lim_upper = Q_LIM_LOWER.copy(), Q_LIM_UPPER.copy()
            self.dq_lim_lower, self.dq_lim_upper = -DQ_LIM.copy(), DQ_LIM.copy()
        else:
            self.col_joint_sizes = list(robot["col_joint_sizes"])
            ql, qh = np.asarray(robot["q_lower"], float), np.asarray(robot["q_upper"], float)
            self.q_lim_lower, self.q_lim_upper = np.where(ql <= -1e19, -np.inf, ql), np.where(qh >= 1e19, np.inf, qh)
            self.dq_lim_lower, self.dq_lim_upper = -np.asarray(robot["dq_max"], float), np.asarray(robot["dq_max"], float)
        self.tau_lim_lower = [-320, -320, -176, -176, -110, -40, -40]
        self.tau_lim_upper = [320, 320, 176, 176, 110, 40, 40]
        self.u_max, self.u_min = U_MAX, -U_MAX

    def get_robot_limits(self):
        return (self.q_lim_upper, self.q_lim_lower, self.dq_lim_upper, self.dq_lim_lower,
                self.tau_lim_upper, self.tau_lim_lower, self.u_max, self.u_min)

    def _one(self, q, dq=None):
        q = np.asarray(q, float).reshape(1, 7)
        dq = np.zeros((1, 7)) if dq is None else np.asarray(dq, float).reshape(1, 7)
        return {k: v[0] for k, v in self._fk(q, dq).items()}

    def batch(self, q, dq=None):
        q = np.ascontiguousarray(q, float)
        dq = np.zeros_like(q) if dq is None else np.ascontiguousarray(dq, float)
        return self._fk(q, dq)

    def fk_pos(self, q):
        return self._one(q)["ee_pos"]

    def fk_pos_col(self, q, i):
        return self._one(q)["col_pts"][i]

    def hom_transform_endeffector(self, q):
        o = self._one(q)
        h = np.eye(4)
        h[:3, :3], h[:3, 3] = o["ee_rot"], o["ee_pos"]
        return h

    def fk(self, q):
        o = self._one(q)
        return np.concatenate((o["ee_pos"], R.from_matrix(o["ee_rot"]).as_rotvec()))

    def jacobian_fk(self, q):
        return self._one(q)["jac"]

    def velocity_ee(self, q, dq):
        return (self.jacobian_fk(q) @ dq)[:3]

    def omega_ee(self, q, dq):
        return (self.jacobian_fk(q) @ dq)[3:]

    def forward_kinematics(self, q, dq):
        """(p_lie, jac, djac) as RobotModel.py:70-77; djac is not used on the MPC path and is
        returned as zeros."""
        o = self._one(q, dq)
        p = np.concatenate((o["ee_pos"], R.from_matrix(o["ee_rot"]).as_rotvec()))
        return p, o["jac"], np.zeros((6, 7))

    def _ik_fn(self):
        if self._ik is None:
            from .solver import default_ik_fn  # raises loudly when the HIP library or the GPU is missing
            self._ik = default_ik_fn(self.robot)
        return self._ik

    def inverse_kinematics_batch(self, pd, rd, q0, n_seeds=1):
        """B inverse-kinematics problems at once: pd [B,3], rd [B,3,3], q0 [B,7] -> dict q [B,7], cost, pos_err, rot_err, iters,
        status, seed [B] (status 0 converged, 1 max_iter, 2 stalled, 3 numerical; include/boundmpc.h bmpc_ik)."""
        pd = np.asarray(pd, float).reshape(-1, 3)
        B = pd.shape[0]
        return self._ik_fn()(pd, np.asarray(rd, float).reshape(B, 3, 3), np.asarray(q0, float).reshape(B, 7), n_seeds=n_seeds)

    def inverse_kinematics(self, pd, rd, q0):
        """RobotModel.py:131-144: joint configuration for the end-effector position pd (3) and rotation rd (3x3) from the start q0,
        within the joint limits.  Returns q (7,) also when the solve did not converge (with a warning, as the reference)."""
        r = self.inverse_kinematics_batch(np.asarray(pd, float)[None], np.asarray(rd, float)[None], np.asarray(q0, float)[None])
        if int(r["status"][0]) != 0:
            log.warning("(IK) No convergence in IK optimization (status %d)", int(r["status"][0]))
        log.info("(IK) Position error %sm", float(r["pos_err"][0]))
        log.info("(IK) Rotation error %s deg", float(r["rot_err"][0]) * 180 / np.pi)
        return np.array(r["q"][0])
