"""ctypes access to the CPU build of the batched inverse-kinematics kernel body (tests/emu/emu_ik.cpp) -- TEST INFRASTRUCTURE ONLY.
Same arguments and results as HipBoundMPC.ik; never imported by the product package."""
import ctypes

import numpy as np

import emu_build

_dp = ctypes.POINTER(ctypes.c_double)
_lib = None

DEFAULT_OPTS = dict(tol_cost=1e-20, tol_grad=1e-10, lambda0=1e-3, max_iter=500)    # bmpc_default_ik_opts


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(emu_build.build("emu_ik.cpp", "libbmpc_emuik.so", ("-O2",)))
    return _lib


def ik(pd, rd, q0, n_seeds=1, lo=None, hi=None, robot=None, nthreads=8, **opts):
    """pd [B,3], rd [B,3,3], q0 [B,7]; lo / hi [B,7] or None (the robot's limits); robot: table of boundplanner_amd.robots or None
    (iiwa14).  Returns the dict of HipBoundMPC.ik."""
    from boundplanner_amd import robots
    from boundplanner_amd.solver import IK_OUT, out_args, out_arrays
    o = dict(DEFAULT_OPTS)
    o.update(opts)
    pd = np.ascontiguousarray(pd, float).reshape(-1, 3)
    B = pd.shape[0]
    rd = np.ascontiguousarray(rd, float).reshape(B, 9)
    q0 = np.ascontiguousarray(q0, float).reshape(B, 7)
    lo = None if lo is None else np.ascontiguousarray(np.broadcast_to(lo, (B, 7)), float)
    hi = None if hi is None else np.ascontiguousarray(np.broadcast_to(hi, (B, 7)), float)
    o4 = np.array([o["tol_cost"], o["tol_grad"], o["lambda0"], o["max_iter"]], float)
    out = out_arrays(IK_OUT, B, np.zeros)
    P = lambda a: a.ctypes.data_as(_dp) if a is not None else None
    r = ctypes.byref(robots.to_struct(robot)) if robot is not None else None
    rc = lib().emu_ik_solve(r, B, int(n_seeds), P(o4), P(pd), P(rd), P(q0), P(lo), P(hi), *out_args(IK_OUT, out), int(nthreads))
    if rc != 0:
        raise ValueError(f"emu_ik_solve: invalid arguments ({rc})")
    return out


def model(q, pd, rd, robot=None):
    """J(q), the half gradient gh [7] and the Gauss-Newton matrix H [7,7] the kernel builds from the geometric Jacobian (ik_eval)."""
    from boundplanner_amd import robots
    q, pd, rd = (np.ascontiguousarray(a, float).ravel() for a in (q, pd, rd))
    gh, Hp = np.zeros(7), np.zeros(28)
    L = lib()
    L.emu_ik_model.restype = ctypes.c_double
    r = ctypes.byref(robots.to_struct(robot)) if robot is not None else None
    f = L.emu_ik_model(r, q.ctypes.data_as(_dp), pd.ctypes.data_as(_dp), rd.ctypes.data_as(_dp), gh.ctypes.data_as(_dp),
                       Hp.ctypes.data_as(_dp))
    H = np.zeros((7, 7))
    H[np.tril_indices(7)] = Hp
    return f, gh, H + np.tril(H, -1).T
