"""ctypes access to the CPU build of the batched convex-set kernel body (tests/emu/emu_sets.cpp) -- TEST INFRASTRUCTURE ONLY.
Same arguments and results as HipBoundMPC.convex_sets; `sets` is a sets_fn for ConvexSetFinder / BoundPlanner.  Never imported by the
product package."""
import ctypes

import numpy as np

import emu_build

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(emu_build.build("emu_sets.cpp", "libbmpc_emusets.so", ("-O2",)))
    return _lib


def sets(obs_sets, obs_points_sets, e_min, e_max, p0, p1=None, fixed_mid=False, optimize=True, nthreads=8):
    """The dict of HipBoundMPC.convex_sets, computed on the CPU."""
    from boundplanner_amd.scenes import pack_scene
    from boundplanner_amd.solver import SETS_MAXOBS, SETS_OUT, out_args, out_arrays
    sc = pack_scene(obs_sets, obs_points_sets, SETS_MAXOBS, min_nv=1, pad_empty=True)
    p0 = np.ascontiguousarray(p0, float).reshape(-1, 3)
    B = p0.shape[0]
    p1 = None if p1 is None else np.ascontiguousarray(p1, float).reshape(B, 3)
    e_min, e_max = (np.ascontiguousarray(e, float).reshape(3) for e in (e_min, e_max))
    out = out_arrays(SETS_OUT, B, np.zeros)
    P = lambda a: a.ctypes.data_as(_dp) if a is not None else None
    I = lambda a: a.ctypes.data_as(_ip)
    rc = lib().emu_convex_sets(sc["n_obs"], P(sc["A"]), P(sc["b"]), I(sc["nrows"]), P(sc["V"]), I(sc["nv"]), P(e_min), P(e_max), B,
                               P(p0), P(p1), int(bool(fixed_mid)), int(bool(optimize)), *out_args(SETS_OUT, out), int(nthreads))
    if rc != 0:
        raise ValueError(f"emu_convex_sets: invalid arguments ({rc})")
    return out


def project(A, b, E, p0):
    """compute_set_projs for one obstacle: the point of {A x <= b} nearest to p0 in the metric of E (exact active-set method)."""
    A = np.ascontiguousarray(A, float); b = np.ascontiguousarray(b, float)
    E = np.ascontiguousarray(E, float); p0 = np.ascontiguousarray(p0, float)
    pt = np.zeros(3)
    rc = lib().emu_sets_project(A.shape[0], A.ctypes.data_as(_dp), b.ctypes.data_as(_dp), E.ctypes.data_as(_dp), p0.ctypes.data_as(_dp),
                                pt.ctypes.data_as(_dp))
    if rc != 0:
        raise RuntimeError(f"emu_sets_project: {rc}")
    return pt


def mvie(A, b, fixed_mid=None, start=None):
    """(q, centre, status, newton steps) of the kernel's MVIE; free centre: the interior search starts at `start`."""
    A = np.ascontiguousarray(A, float); b = np.ascontiguousarray(b, float)
    c = np.array(fixed_mid if fixed_mid is not None else start, float)
    q = np.zeros(9)
    nw = ctypes.c_int()
    st = lib().emu_sets_mvie(A.shape[0], A.ctypes.data_as(_dp), b.ctypes.data_as(_dp), int(fixed_mid is not None),
                             c.ctypes.data_as(_dp), q.ctypes.data_as(_dp), ctypes.byref(nw))
    return q.reshape(3, 3), c, st, nw.value


def polyhedron(obs_sets, obs_points_sets, e_min, e_max, E, p):
    """One round of the polyhedron growth around p in the metric E: (n, A [20][3], b [20]); n < 0: minus the set status."""
    from boundplanner_amd.scenes import pack_scene
    from boundplanner_amd.solver import SETS_MAXOBS, SETS_ROWS
    sc = pack_scene(obs_sets, obs_points_sets, SETS_MAXOBS, min_nv=1, pad_empty=True)
    E, p, e_min, e_max = (np.ascontiguousarray(v, float) for v in (E, p, e_min, e_max))
    A, b = np.zeros((SETS_ROWS, 3)), np.zeros(SETS_ROWS)
    P = lambda a: a.ctypes.data_as(_dp)
    n = lib().emu_sets_polyhedron(sc["n_obs"], P(sc["A"]), P(sc["b"]), sc["nrows"].ctypes.data_as(_ip), P(sc["V"]),
                                  sc["nv"].ctypes.data_as(_ip), P(e_min), P(e_max), P(E), P(p), A.ctypes.data_as(_dp), b.ctypes.data_as(_dp))
    if n == -100:
        raise ValueError("emu_sets_polyhedron: invalid arguments")
    return n, A, b
