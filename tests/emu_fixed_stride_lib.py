"""ctypes access to the CPU emulation of the pair kernels' generic and fixed-horizon instantiations (tests/emu/emu_fixed_stride.cpp)
-- TEST INFRASTRUCTURE ONLY."""
import ctypes

import numpy as np

import emu_build

_dp = ctypes.POINTER(ctypes.c_double)


def build(force=False):
    return emu_build.build("emu_fixed_stride.cpp", "libbmpc_emufixed.so", ("-O1", "-g"), force=force)


def super_steps(N, x0, lbx, ubx, p, fixed, steps, trial_spec=False, dt=0.1):
    """`steps` super-steps from the cold start on the generic (fixed=False) or the fixed-horizon bodies: the whole workspace and the
    instance states as raw 64-bit / 8-bit patterns, the largest number of rejected trials of one line search, and their total."""
    lib = ctypes.CDLL(build())
    lib.emu_fixed_work_doubles.restype = ctypes.c_size_t
    lib.emu_fixed_state_bytes.restype = ctypes.c_size_t
    lbx = np.where(np.isinf(lbx), -1e20, lbx); ubx = np.where(np.isinf(ubx), 1e20, ubx)
    x0, lbx, ubx, p = (np.ascontiguousarray(np.atleast_2d(a), float) for a in (x0, lbx, ubx, p))
    B = x0.shape[0]
    work = np.zeros(lib.emu_fixed_work_doubles(N, B))
    state = np.zeros(lib.emu_fixed_state_bytes(B), np.uint8)
    bt = np.zeros(2, np.int32)
    P = lambda a: a.ctypes.data_as(_dp)
    rc = lib.emu_fixed_super_steps(N, ctypes.c_double(dt), B, P(x0), P(lbx), P(ubx), P(p), int(fixed), steps, int(trial_spec), P(work),
                                   state.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), bt.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    assert rc == 0, rc
    return dict(work=work.view(np.uint64), state=state, bt_max=int(bt[0]), bt_sum=int(bt[1]))
