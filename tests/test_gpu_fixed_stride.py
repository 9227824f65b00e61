"""The pair kernels compiled for one horizon (bmpc_pair_n20.hip, bmpc_pair_n30.hip: the SoA strides are compile-time constants)
against the generic kernels of bmpc_pipeline.hip, on the GPU.  The two are the same source with different integer address
arithmetic, so a solve must not depend on which ran: x, f, viol, iters, status bitwise equal.  BMPC_FIXED_STRIDE (1: the
fixed-horizon kernels where there are some; 0: the generic kernels everywhere) is read once per process, so the two settings run in
child processes, each solving all cases:
  N = 20, B = 7   three instances per wavefront: two full wavefronts plus one instance
  N = 30, B = 5   two per wavefront: two full plus one
  N = 20, B = 70 through a pool of 64 slots (the smallest pool a handle takes): six rows wait for slots that are refilled while
                 the other instances are mid-solve
All cold start, the benchmark's generator (scenes.make_batch, randomised sets) at a small seed.  Each child also reports how many
launches went to a fixed-horizon kernel (bmpc_pipe_fixed_launches): none with the switch at 0, some with it at 1."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("x", "f", "viol", "iters", "status")
CASES = (("n20", 20, 7, 0), ("n30", 30, 5, 0), ("n20_pool64", 20, 70, 64))      # name, N, B, pool_slots (0: a slot per instance)
CODE = """
import sys, ctypes, numpy as np
sys.path.insert(0, %r)
import torch
from boundplanner_amd import scenes, solver
from boundplanner_amd.solver import HipBoundMPC
out = {}
for name, N, B, slots in %r:
    be = HipBoundMPC(N, pool_slots=slots) if slots else HipBoundMPC(N)
    b = scenes.make_batch(B, N, 5, be.fk, randomize_sets=True)
    r = be.solve_batch(b["x0"], b["lbx"], b["ubx"], b["p"])
    for k in %r:
        out[name + "_" + k] = r[k]
    be.close()
lib = solver.load_library()
lib.bmpc_pipe_fixed_launches.restype = ctypes.c_long
out["fixed_launches"] = np.int64(lib.bmpc_pipe_fixed_launches())
np.savez(sys.argv[1], **out)
""" % (ROOT, CASES, KEYS)


@pytest.mark.gpu
def test_fixed_horizon_pair_kernels_agree_bitwise_with_the_generic_ones(tmp_path):
    res = {}
    for switch in ("1", "0"):
        path = str(tmp_path / f"fixed_{switch}.npz")
        subprocess.run([sys.executable, "-c", CODE, path], check=True, env=dict(os.environ, BMPC_FIXED_STRIDE=switch), timeout=300)
        res[switch] = np.load(path)
    assert int(res["1"]["fixed_launches"]) > 0 and int(res["0"]["fixed_launches"]) == 0
    for name, N, B, _ in CASES:
        for k in KEYS:
            a, b = res["1"][f"{name}_{k}"], res["0"][f"{name}_{k}"]
            assert a.shape[0] == B and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, k)
        assert (res["1"][f"{name}_status"] == 0).any(), name          # the solves did something
