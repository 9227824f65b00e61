"""The two device users of the greedy separating-halfspace routine (boundplanner_amd/csrc/bmpc_freespace.hpp:
separating_halfspaces) produce the same rows, bit for bit: the closed loop's way for one collision point (closest pairs stored by a
first pass, then the rows: tests/emu/emu_segment_rows.cpp) against the set kernel's segment mode (closest pairs computed again
inside the loop: emu_convex_sets).  CPU builds of the identical source; rows 0..5 are each caller's own box and are not compared."""
import ctypes

import numpy as np
from scipy.spatial.transform import Rotation as R

import emu_build
import emu_sets_lib as ES
from boundplanner_amd.device_loop import MAX_OBS
from boundplanner_amd.scenes import pack_scene

_dp, _ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
SETS_TOO_MANY_ROWS = 2


def _rotated_boxes(rng, n, centres, h_lo, h_hi):
    """n boxes turned by random rotations (general polytopes: never the loop's box clamp) as [A, b] + their 8 corners."""
    sets, pts = [], []
    for c in centres[:n]:
        h = rng.uniform(h_lo, h_hi, size=3)
        Q = R.from_rotvec(rng.normal(size=3)).as_matrix()
        sets.append([np.vstack((Q.T, -Q.T)), np.concatenate((Q.T @ c + h, -(Q.T @ c) + h))])
        pts.append(np.array([c + Q @ (np.array([sx, sy, sz]) * h) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]))
    return sets, pts


def _cases():
    """48 scenes of 1..16 rotated boxes, 6 segments each (lengths 0, ~0.05, ~0.6, twice): 288 segments.  Two kinds of scene:
    boxes scattered through the arm's workspace, the segments starting anywhere in it (few rows, now and then a segment that runs
    through a box), and small boxes on a sphere of radius 0.3 around the segments' start (every box needs a halfspace of its own:
    many rows, and more than 15 once there are 10 boxes or more)."""
    rng = np.random.default_rng(2024)
    out = []
    for k in range(48):
        n = 1 + k % 16
        if (k // 16) % 2 == 0:
            centre = None
            sets, pts = _rotated_boxes(rng, n, rng.uniform([-0.7, -0.7, 0.0], [0.7, 0.7, 1.1], size=(n, 3)), 0.03, 0.15)
        else:
            centre = rng.uniform([-0.3, -0.3, 0.4], [0.3, 0.3, 0.8])
            d = rng.normal(size=(n, 3))
            sets, pts = _rotated_boxes(rng, n, centre + 0.3 * d / np.linalg.norm(d, axis=1)[:, None], 0.02, 0.04)
        for length in (0.0, 0.05, 0.6) * 2:
            while True:
                p0 = rng.uniform([-0.7, -0.7, 0.0], [0.7, 0.7, 1.1]) if centre is None else centre + rng.normal(size=3) * 0.01
                # a single point inside an obstacle has no separating direction (cp = p0 = p1: the row is 0 / 0 on both sides, and
                # the set kernel then reports a numerical failure instead of rows): the degenerate segments start in free space
                if length or not any(np.all(A @ p0 <= b) for A, b in sets):
                    break
            d = rng.normal(size=3)
            out.append((sets, pts, p0, p0 + length * rng.uniform(0.8, 1.2) * d / np.linalg.norm(d) if length else p0.copy()))
    return out


def _loop_rows(lib, sets, pts, p0, p1):
    sc = pack_scene(sets, pts, MAX_OBS)
    a, b, touched = np.zeros((15, 3)), np.zeros(15), ctypes.c_int()
    P = lambda x: np.ascontiguousarray(x, float).ctypes.data_as(_dp)
    n = lib.emu_loop_segment_rows(sc["n_obs"], P(sc["A"]), P(sc["b"]), sc["nrows"].ctypes.data_as(_ip), P(sc["V"]),
                                  sc["nv"].ctypes.data_as(_ip), P(p0), P(p1), a.ctypes.data_as(_dp), b.ctypes.data_as(_dp),
                                  ctypes.byref(touched))
    return n, a, b, touched.value


def test_loop_and_set_kernel_choose_the_same_rows():
    lib = ctypes.CDLL(emu_build.build("emu_segment_rows.cpp", "libbmpc_emusegrows.so", ("-O1", "-g")))
    seen = dict(touching=0, degenerate=0, rows10=0, overflow=0)
    for k, (sets, pts, p0, p1) in enumerate(_cases()):
        assert all(v.shape == (8, 3) for v in pts)
        n, a, b, touched = _loop_rows(lib, sets, pts, p0, p1)
        s = ES.sets(sets, pts, [-3.0] * 3, [3.0] * 3, p0[None], p1[None], nthreads=1)
        status, ns = int(s["status"][0]), int(s["nrows"][0])
        # the set kernel hands out rows only with status 0, and says so when 20 do not suffice; anything else (no interior point
        # for its ellipsoid) would leave this segment unchecked
        assert status in (0, SETS_TOO_MANY_ROWS), (k, status)
        assert bool(touched) == bool(s["collision"][0]), k
        assert (n == -1) == (status == SETS_TOO_MANY_ROWS or ns > 15), (k, n, status, ns)
        if status == 0:
            m = min(ns, 15)                  # on overflow the loop has written the rows that fit
            assert n == -1 or n == ns, (k, n, ns)
            assert a[6:m].tobytes() == s["A"][0, 6:m].tobytes() and b[6:m].tobytes() == s["b"][0, 6:m].tobytes(), (k, n)
        seen["touching"] += bool(touched)
        seen["degenerate"] += bool(np.array_equal(p0, p1))
        seen["rows10"] += n >= 10
        seen["overflow"] += n == -1
    print(seen)
    assert all(v > 0 for v in seen.values()), seen
