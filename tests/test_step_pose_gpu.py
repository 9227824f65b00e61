"""k_step and k_pose on the MI355X against the same bodies in the CPU emulator (tests/test_step_pose_phases.py is the CPU half).

64 instances of the benchmark's generator (randomized convex sets) at their cold start, at N = 6 and N = 20, with seeded row
slacks / multipliers (the inputs of tests/test_step_pose_phases.py, Gauss-Newton mode), through bmpc_debug_line_search: the
product's own evaluation launches (k_points || k_pose, k_eval), Riccati sweep, k_fwd and k_step, whose row steps dt and
line-search start (ap, ad, D of the ls record) are compared with emu_pipe_lib.line_search on the same inputs.

HIP and emulator run the same source with another contraction of products into sums, so the comparison is not bitwise.  Bounds:
  dt      1e-9 x the largest |dt| of the stage, the project's bound for a same-source comparison (tests/test_curvature_gpu.py);
  ap, ad  1e-9 x the value itself;
  D       1e-9 x (|df| + sum |mu dt_i / t_i|), the scale tests/line_search_lib.py (merit_derivative) holds D to -- without the
          share of that bound that is its finite-difference reference's own error, which has no counterpart here.

64 is not a multiple of the instances per wavefront (12 at N = 6, 3 at N = 20): the last wavefront of k_step has padding lanes.
The first and the last instance alone must give bitwise what they give inside the batch.
"""
import numpy as np
import pytest

import line_search_lib as L
from test_step_pose_phases import make_inputs

pytestmark = pytest.mark.gpu
B = 64


@pytest.mark.parametrize("N", [6, 20])
def test_hip_row_steps_equal_the_emulators(N):
    import emu_pipe_lib as E
    from boundplanner_amd.solver import HipBoundMPC
    assert B % (64 // (N - 1)) != 0, "the last wavefront must have padding lanes"
    x0, lbx, ubx, p, TS, ZS, _ = make_inputs(N, B, 5400 + N)
    args = (x0, lbx, ubx, p, TS, ZS, np.zeros(B, np.int32))
    h = HipBoundMPC(N)
    out = h.line_search(*args)
    ref = E.line_search(N, *args)
    live = ZS > 0
    assert np.array_equal(~np.isnan(ref["dt"]), live) and np.array_equal(~np.isnan(out["dt"]), live)
    dt, dte = np.where(live, out["dt"], 0.0), np.where(live, ref["dt"], 0.0)
    scale = np.abs(dte).max(axis=2, keepdims=True)
    assert (scale > 0).all()
    d_dt = (np.abs(dt - dte) / scale).max()
    ls, lse = out["ls"], ref["ls"]
    d_ap, d_ad = (np.abs(ls[:, L.LS[k]] - lse[:, L.LS[k]]) / np.abs(lse[:, L.LS[k]]) for k in ("ap", "ad"))
    terms = lse[:, L.LS["mu"], None, None] * np.where(live, ref["dt"] / np.where(live, ref["t0"], 1.0), 0.0)
    df = lse[:, L.LS["D"]] + terms.sum(axis=(1, 2))               # D = df - sum mu dt_i / t_i
    d_D = np.abs(ls[:, L.LS["D"]] - lse[:, L.LS["D"]]) / (np.abs(df) + np.abs(terms).sum(axis=(1, 2)))
    print(f"HIP against emulator, N={N}, B={B}: max |d dt| / max|dt_stage| = {d_dt:.2g}, |d ap| / ap = {d_ap.max():.2g}, |d ad| / ad = "
          f"{d_ad.max():.2g}, |d D| / (|df| + sum |mu dt / t|) = {d_D.max():.2g}; ap < 1 in {(lse[:, L.LS['ap']] < 1).sum()}, ad < 1 in "
          f"{(lse[:, L.LS['ad']] < 1).sum()} instances", flush=True)
    assert np.isfinite(ls[:, :3]).all() and np.isfinite(lse[:, :3]).all()
    assert d_dt <= 1e-9
    assert d_ap.max() <= 1e-9 and d_ad.max() <= 1e-9
    assert d_D.max() <= 1e-9
    for j in (0, B - 1):                   # a first lane, and the ragged last wavefront
        one = h.line_search(*(a[j:j + 1] for a in args))
        for k in ("dt", "ls"):
            assert np.array_equal(one[k][0], out[k][j], equal_nan=True), f"{k}: instance {j} alone differs from instance {j} of the batch"
