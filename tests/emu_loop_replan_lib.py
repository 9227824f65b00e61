"""ctypes access to the CPU build of the device loop's path installation (tests/emu/emu_loop_replan.cpp) -- TEST INFRASTRUCTURE
ONLY.  Same compiler flags as emu_loop_lib."""
import ctypes

import numpy as np

import emu_build

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(emu_build.build("emu_loop_replan.cpp", "libbmpc_emuloopreplan.so", ("-O1", "-g")))
    return _lib


def install_replan(N, S, plans):
    """S [R][state] (rewritten in place, as the kernel does), plans: one (p_via, r_via, bp1, br1, e_r_bound, a_sets, b_sets) per rollout."""
    from boundplanner_amd.device_loop import pack_plans
    assert S.ndim == 2 and S.flags.c_contiguous and len(plans) == S.shape[0]
    n_pts, *arrs = pack_plans(plans)
    lib().emu_loop_install_replan(N, S.shape[0], S.ctypes.data_as(_dp), n_pts.ctypes.data_as(_ip), *[a.ctypes.data_as(_dp) for a in arrs])
    return S


def install_fresh(N, S, q0s, weights):
    """S [R][state] (rewritten in place): rollouts at rest at q0s [R][7]."""
    q0s = np.ascontiguousarray(q0s, float)
    w = np.ascontiguousarray(weights, float)
    assert S.ndim == 2 and S.flags.c_contiguous and q0s.shape == (S.shape[0], 7) and w.shape == (11,)
    lib().emu_loop_install_fresh(N, S.shape[0], S.ctypes.data_as(_dp), q0s.ctypes.data_as(_dp), w.ctypes.data_as(_dp))
    return S
