"""ctypes access to the CPU build of the prepare phase with one scene per rollout (tests/emu/emu_loop_scenes.cpp) -- TEST
INFRASTRUCTURE ONLY.  Same compiler flags as emu_loop_lib, so that the two builds can be compared bitwise."""
import ctypes

import numpy as np

import emu_build

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(emu_build.build("emu_loop_scenes.cpp", "libbmpc_emuloopscenes.so", ("-O1", "-g")))
    return _lib


def pack_scenes(scenes):
    """[(obs_sets, obs_points_sets), ...] -> n_obs, A, b, nrows, V, nv in the layout of bmpc_loop_set_scenes."""
    from boundplanner_amd.device_loop import MAX_OBS
    from boundplanner_amd.scenes import pack_scene
    packed = [pack_scene(sets, pts, MAX_OBS) for sets, pts in scenes]
    n_obs = np.array([p["n_obs"] for p in packed], np.int32)
    cat = lambda k, t: np.ascontiguousarray(np.concatenate([p[k] for p in packed]), t) if packed else np.zeros(0, t)
    return n_obs, cat("A", float), cat("b", float), cat("nrows", np.int32), cat("V", float), cat("nv", np.int32)


def prepare_scenes(N, S, prev, scenes, rollout_scene):
    """S [R][state], prev [R][n_w] (S is advanced in place, as the kernels do) -> x0, lbx, ubx [R][n_w], p [R][875]."""
    R, n_w = S.shape[0], 44 * N + 6
    assert S.flags.c_contiguous and prev.shape == (R, n_w) and prev.flags.c_contiguous
    n_obs, A, b, nrows, V, nv = pack_scenes(scenes)
    sc = np.ascontiguousarray(rollout_scene, np.int32)
    assert sc.shape == (R,) and sc.min() >= -1 and sc.max() < len(scenes)
    x0, lbx, ubx, p = np.zeros((R, n_w)), np.zeros((R, n_w)), np.zeros((R, n_w)), np.zeros((R, 875))
    P = lambda a: a.ctypes.data_as(_dp)
    I = lambda a: a.ctypes.data_as(_ip)
    lib().emu_loop_prepare_scenes(N, R, P(S), P(prev), P(x0), P(lbx), P(ubx), P(p), len(scenes), I(n_obs), P(A), P(b), I(nrows), P(V), I(nv),
                                  I(sc))
    return x0, lbx, ubx, p
