"""k_curv on the MI355X against the same kernel body in the CPU emulator (tests/test_curvature_contraction.py is the CPU half).

64 instances of the benchmark's generator (randomized convex sets) at their cold start, at N = 6 and N = 20, with seeded row
slacks / multipliers and seeded lam_pi, through bmpc_debug_stage_matrices: the product's own evaluation launches (k_points ||
k_pose, bmpc_k_eval_curv_split) and the Riccati sweep's load phase.  That entry puts EVERY instance into exact-Hessian mode (its
k_set_rows_body is called without a mode array: hess_mode = 1), so k_curv runs for all 64.

The record fields k_curv writes (F_CQP .. F_END) are not handed out; they reach the stage matrix through the scatter table as its
q x (q, dq, pi) blocks.  Those blocks are compared on a scale of their own -- the largest entry of rows q, columns q, dq, pi of the
stage with the q x q diagonal (where the barrier terms of the joint bounds sit) left out, one to two orders of magnitude below max|H_stage|
for these batches -- so that an error in a curvature entry cannot hide under a large entry elsewhere in the stage; the whole matrix is
compared against max|H_stage| as well.  HIP and emulator run the same source with another contraction of products into sums: the
bound is the one tests/test_hessian_pin_gpu.py holds the HIP kernels to, 1e-9 x the scale.

64 is not a multiple of the instances per wavefront (12 at N = 6, 3 at N = 20): the last wavefront of k_curv has padding lanes.
One instance alone must give bitwise what it gives inside the batch.
"""
import numpy as np
import pytest

import hessian_pin_lib as HP
import oracle_lib as O

pytestmark = pytest.mark.gpu
B = 64


def _batch(N, seed):
    from boundplanner_amd import scenes
    b = scenes.make_batch(B, N, seed, O.fk_batch, randomize_sets=True)
    rng = np.random.default_rng(seed + 1)
    x0 = b["x0"].copy()
    st0 = np.arange(40) * N
    x0[:, st0] = b["lbx"][:, st0]
    TS, ZS = np.zeros((B, N - 1, HP.NSLOT)), np.zeros((B, N - 1, HP.NSLOT))
    for i in range(B):
        rows = O.stage_rows(N, x0[i], b["lbx"][i], b["ubx"][i], b["p"][i])
        t = 0.3 * np.exp(rng.normal(size=(N - 1, HP.MAXROWS)))
        z = 0.5 * np.exp(rng.normal(size=(N - 1, HP.MAXROWS)))
        TS[i], ZS[i] = HP.slot_arrays(N, rows, t, z, HP.ORACLE_Y_NAMES)
    return x0, b["lbx"], b["ubx"], b["p"], TS, ZS, rng.normal(size=(B, N, 3))


@pytest.mark.parametrize("N", [6, 20])
def test_hip_curvature_block_equals_the_emulators(N):
    import emu_pipe_lib as E
    from boundplanner_amd.solver import HipBoundMPC
    assert B % (64 // (N - 1)) != 0, "the last wavefront must have padding lanes"
    args = _batch(N, 5200 + N)
    h = HipBoundMPC(N)
    H = h.stage_matrices(*args)
    He = E.stage_matrices(N, *args, split=1)
    assert H.shape == He.shape == (B, N - 1, 41, 41) and np.isfinite(H).all()
    scale = np.abs(He).max(axis=(2, 3), keepdims=True)
    d = np.abs(H - He) / scale
    blk, blk_e = H[:, :, :7, :24], He[:, :, :7, :24].copy()          # rows q, columns q, dq, ddq, pi (ddq: zero but for the coordinate change)
    own = blk_e.copy()
    own[:, :, np.arange(7), np.arange(7)] = 0
    bscale = np.abs(own).max(axis=(2, 3), keepdims=True)
    assert (bscale > 0).all()
    db = np.abs(blk - blk_e) / bscale
    print(f"HIP against emulator, N={N}, B={B}: max |dH| / max|H_stage| = {d.max():.2g}; q x (q, dq, pi) blocks on their own scale "
          f"{db.max():.2g} (that scale is {float((bscale / scale).min()):.2g} .. {float((bscale / scale).max()):.2g} x max|H_stage|)", flush=True)
    assert db.max() <= 1e-9
    assert d.max() <= 1e-9
    for j in (0, B - 1):                   # a first lane, and the ragged last wavefront
        Hj = h.stage_matrices(*(a[j:j + 1] for a in args))
        assert np.array_equal(Hj[0], H[j]), f"instance {j} alone differs from instance {j} of the batch"
