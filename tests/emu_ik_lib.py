"""ctypes access to the CPU build of the batched inverse-kinematics kernel body (tests/emu/emu_ik.cpp) -- TEST INFRASTRUCTURE ONLY.
Same arguments and results as HipBoundMPC.ik; never imported by the product package."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "emu_ik.cpp")
LIB = os.path.join(ROOT, "tests", "emu", "libbmpc_emuik.so")
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_lib = None

DEFAULT_OPTS = dict(tol_cost=1e-20, tol_grad=1e-10, lambda0=1e-3, max_iter=500)    # bmpc_default_ik_opts


def lib():
    global _lib
    if _lib is None:
        cs = os.path.join(ROOT, "boundplanner_amd", "csrc")
        deps = [SRC] + [os.path.join(cs, f) for f in ("bmpc_ik.hpp", "bmpc_device.hpp", "bmpc_robot.hpp")]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas", "-o", LIB, SRC])
        _lib = ctypes.CDLL(LIB)
    return _lib


def ik(pd, rd, q0, n_seeds=1, lo=None, hi=None, robot=None, nthreads=8, **opts):
    """pd [B,3], rd [B,3,3], q0 [B,7]; lo / hi [B,7] or None (the robot's limits); robot: table of boundplanner_amd.robots or None
    (iiwa14).  Returns the dict of HipBoundMPC.ik."""
    from boundplanner_amd import robots
    o = dict(DEFAULT_OPTS)
    o.update(opts)
    pd = np.ascontiguousarray(pd, float).reshape(-1, 3)
    B = pd.shape[0]
    rd = np.ascontiguousarray(rd, float).reshape(B, 9)
    q0 = np.ascontiguousarray(q0, float).reshape(B, 7)
    lo = None if lo is None else np.ascontiguousarray(np.broadcast_to(lo, (B, 7)), float)
    hi = None if hi is None else np.ascontiguousarray(np.broadcast_to(hi, (B, 7)), float)
    o4 = np.array([o["tol_cost"], o["tol_grad"], o["lambda0"], o["max_iter"]], float)
    out = dict(q=np.zeros((B, 7)), cost=np.zeros(B), pos_err=np.zeros(B), rot_err=np.zeros(B), iters=np.zeros(B, np.int32),
               status=np.zeros(B, np.int32), seed=np.zeros(B, np.int32))
    P = lambda a: a.ctypes.data_as(_dp) if a is not None else None
    I = lambda a: a.ctypes.data_as(_ip)
    r = ctypes.byref(robots.to_struct(robot)) if robot is not None else None
    rc = lib().emu_ik_solve(r, B, int(n_seeds), P(o4), P(pd), P(rd), P(q0), P(lo), P(hi), P(out["q"]), P(out["cost"]),
                            P(out["pos_err"]), P(out["rot_err"]), I(out["iters"]), I(out["status"]), I(out["seed"]), int(nthreads))
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
