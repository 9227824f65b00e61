"""ctypes access to the CPU build of the closed-loop step logic (tests/emu/emu_loop.cpp) -- TEST INFRASTRUCTURE ONLY."""
import ctypes

import numpy as np

import emu_build

_dp = ctypes.POINTER(ctypes.c_double)
P = lambda a: a.ctypes.data_as(_dp) if a is not None else None
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(emu_build.build("emu_loop.cpp", "libbmpc_emuloop.so", ("-O1", "-g")))
    return _lib


def layout():
    from boundplanner_amd.device_loop import read_layout
    L = lib()
    return read_layout(L.emu_loop_field, L.emu_loop_state_doubles)


def prepare(N, S, prev):
    n_w = 44 * N + 6
    x0, lbx, ubx, p = np.zeros(n_w), np.zeros(n_w), np.zeros(n_w), np.zeros(875)
    lib().emu_loop_prepare(N, P(S), P(prev), P(x0), P(lbx), P(ubx), P(p))
    return x0, lbx, ubx, p


def prepare_obs(N, S, prev, obs_sets, obs_points_sets):
    from boundplanner_amd.device_loop import MAX_OBS
    from boundplanner_amd.scenes import pack_scene
    sc = pack_scene(obs_sets, obs_points_sets, MAX_OBS)
    ip = ctypes.POINTER(ctypes.c_int)
    n_w = 44 * N + 6
    x0, lbx, ubx, p = np.zeros(n_w), np.zeros(n_w), np.zeros(n_w), np.zeros(875)
    lib().emu_loop_prepare_obs(N, P(S), P(prev), P(x0), P(lbx), P(ubx), P(p), sc["n_obs"], P(sc["A"]), P(sc["b"]),
                               sc["nrows"].ctypes.data_as(ip), P(sc["V"]), sc["nv"].ctypes.data_as(ip))
    return x0, lbx, ubx, p


def finish(N, dt, S, x, prev, status, viol, iters=0, par=None):
    """-> log row; with `par` (the step's parameter vector) -> (log row, MPCData record of the step)."""
    log = np.zeros(lib().emu_loop_logw())
    rec = np.zeros(lib().emu_loop_record_doubles(N)) if par is not None else None
    lib().emu_loop_finish(N, ctypes.c_double(dt), P(S), P(np.ascontiguousarray(x, float)), P(prev), int(status),
                          ctypes.c_double(viol), int(iters), P(log), P(rec) if rec is not None else None,
                          P(np.ascontiguousarray(par, float)) if par is not None else None)
    return log if par is None else (log, rec)


def so3(v, M):
    R, v2, e = np.zeros((3, 3)), np.zeros(3), np.zeros(3)
    lib().emu_so3(P(np.ascontiguousarray(v, float)), P(np.ascontiguousarray(M, float)), P(R), P(v2), P(e))
    return R, v2, e


_A = lambda a: np.ascontiguousarray(a, float)


def jac_inv(ax, sign):
    J = np.zeros((3, 3))
    lib().emu_jac_inv(P(_A(ax)), ctypes.c_double(sign), P(J))
    return J


def initial_rot_errors(pr, pr_ref, dpn, br1, br2):
    out = [np.zeros(3) for _ in range(4)]
    lib().emu_initial_rot_errors(P(_A(pr)), P(_A(pr_ref)), P(_A(dpn)), P(_A(br1)), P(_A(br2)), *[P(o) for o in out])
    return out


def integrate_rot_ref(pr_ref, omega, phi0, phi1):
    out = np.zeros(3)
    lib().emu_integrate_rot_ref(P(_A(pr_ref)), P(_A(omega)), ctypes.c_double(phi0), ctypes.c_double(phi1), P(out))
    return out
