"""The stage matrices of the HIP kernels, pinned to the reference (MI355X; tests/test_hessian_pin.py is the CPU half).

bmpc_debug_stage_matrices: slots initialised by the product's init launch, row slacks / multipliers and the exact-Hessian switch
overwritten, the product's own evaluation launches of a super-step (k_points || k_pose, bmpc_k_eval_curv_split) once, then a debug
kernel that runs the Riccati sweep's load phase (ric_phase_load_impl<128>) per stage and copies the matrix it leaves in LDS.

  * every probe of tests/golden/hess_N*.npz (N = 6, 10, 20, 30; none skipped) within 10 x its error estimate + 1e-9 x its scale;
  * entry by entry against the oracle at 1e-9 x max|H_stage| on B = 257 instances at N = 20 and N = 30 (floor(64 / (N-1)) instances per
    wavefront of the thread-per-pair kernels: whole wavefronts and a ragged last one), multipliers from a seeded generator;
  * position independence: instances of that batch run alone give bitwise the matrices they give inside it.

Reads tests/golden/ and the oracle library only.
"""
import numpy as np
import pytest

import hessian_pin_lib as HP
import oracle_lib as O

pytestmark = pytest.mark.gpu


def _handle(N):
    from boundplanner_amd.solver import HipBoundMPC
    return HipBoundMPC(N)


@pytest.mark.parametrize("N", HP.HORIZONS)
def test_hip_kernels_meet_every_probe(golden_dir, N):
    fx = HP.load(golden_dir, N)
    P = len(fx["w"])
    inp = [HP.point_inputs(fx, ip, O) for ip in range(P)]
    slots = [HP.slot_arrays(N, i[7], i[4], i[5], fx["y_names"]) for i in inp]
    stack = lambda j: np.array([i[j] for i in inp])
    H = _handle(N).stage_matrices(stack(0), stack(1), stack(2), stack(3), np.array([s[0] for s in slots]), np.array([s[1] for s in slots]), stack(6))
    ratios, worst_o = [], 0.0
    for ip in range(P):
        w, lbx, ubx, p, t, z, lam_pi, rows = inp[ip]
        ratios += HP.probe_ratios(fx, ip, H[ip], t, z, rows)
        Ho = O.stage_matrices(N, w, lbx, ubx, p, t, z, lam_pi, float(fx["dt"]))
        worst_o = max(worst_o, max(np.abs(H[ip, k] - Ho[k]).max() / np.abs(Ho[k]).max() for k in range(N - 1)))
    assert len(ratios) == len(fx["pr_b"]) + len(fx["dd_b"])
    worst = HP.worst_by_block(ratios)
    print(f"HIP kernels N={N}: " + ", ".join(f"{b} {v[0]:.2g}" for b, v in worst.items()) + f"; against the oracle {worst_o:.2g} x max|H_stage|", flush=True)
    bad = [(b, k, f"{r:.3g}", got, want) for b, k, r, got, want in ratios if not r <= 1.0]
    assert not bad, f"N={N}: {len(bad)} of {len(ratios)} probes miss their tolerance (block, stage, ratio, got, expected): {bad[:8]}"
    assert worst_o <= 1e-9


def _batch(N, B, seed):
    """B problems of the benchmark's generator at their cold start, with seeded (t, z) on every row and seeded lam_pi"""
    from boundplanner_amd import scenes
    b = scenes.make_batch(B, N, seed, O.fk_batch, randomize_sets=True)
    rng = np.random.default_rng(seed + 1)
    x0 = b["x0"].copy()
    st0 = np.arange(40) * N
    x0[:, st0] = b["lbx"][:, st0]
    T, Z, TS, ZS = (np.zeros((B, N - 1, n)) for n in (HP.MAXROWS, HP.MAXROWS, HP.NSLOT, HP.NSLOT))
    for i in range(B):
        rows = O.stage_rows(N, x0[i], b["lbx"][i], b["ubx"][i], b["p"][i])
        T[i] = 0.3 * np.exp(rng.normal(size=(N - 1, HP.MAXROWS)))
        Z[i] = 0.5 * np.exp(rng.normal(size=(N - 1, HP.MAXROWS)))
        TS[i], ZS[i] = HP.slot_arrays(N, rows, T[i], Z[i], HP.ORACLE_Y_NAMES)
    lam_pi = rng.normal(size=(B, N, 3))
    return x0, b["lbx"], b["ubx"], b["p"], T, Z, TS, ZS, lam_pi



@pytest.mark.parametrize("N", [20, 30])
def test_hip_kernels_against_oracle_on_ragged_batch_and_alone(N):
    B = 257
    x0, lbx, ubx, p, T, Z, TS, ZS, lam_pi = _batch(N, B, 4100 + N)
    h = _handle(N)
    H = h.stage_matrices(x0, lbx, ubx, p, TS, ZS, lam_pi)
    worst = 0.0
    for i in range(B):
        Ho = O.stage_matrices(N, x0[i], lbx[i], ubx[i], p[i], T[i], Z[i], lam_pi[i])
        for k in range(N - 1):
            worst = max(worst, np.abs(H[i, k] - Ho[k]).max() / np.abs(Ho[k]).max())
    print(f"HIP kernels against the oracle, N={N}, B={B}: max |dH| / max|H_stage| = {worst:.2g}", flush=True)
    assert worst <= 1e-9
    ipw = 64 // (N - 1)
    for j in (0, 1, ipw - 1, ipw, 100, B - 2, B - 1):          # first / last lanes of a wavefront, the ragged last wavefront
        Hj = h.stage_matrices(x0[j:j + 1], lbx[j:j + 1], ubx[j:j + 1], p[j:j + 1], TS[j:j + 1], ZS[j:j + 1], lam_pi[j:j + 1])
        assert np.array_equal(Hj[0], H[j]), f"instance {j} alone differs from instance {j} of the batch"
    sub = slice(37, 37 + 5)                                     # a sub-batch at another position
    Hs = h.stage_matrices(x0[sub], lbx[sub], ubx[sub], p[sub], TS[sub], ZS[sub], lam_pi[sub])
    assert np.array_equal(Hs, H[sub])
