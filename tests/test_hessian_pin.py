"""The exact Lagrangian Hessian of oracle and kernel bodies, pinned to the reference (no GPU).

tests/golden/hess_N*.npz (tests/golden/gen/gen_hess.py) hold bilinear probes b = D^2 L~ [s, r] of the Hessian of the substituted stage
Lagrangian, computed from the reference's own formulation at complex arguments, per stage and per block (q x q, q x dq, q x pi,
dq x dq, q x slacks, pi x pi, random pairs over all of y_k, d x d), at random points with all five split patterns and at points
the solver visits.  Asserted here, for N = 6, 10, 20, 30 and for EVERY probe (none is skipped):

  * the oracle's stage matrices (eval_stage + assemble_stage with the exact Hessian, bmpc_oracle_stage_matrices) and
  * the kernel bodies' (k_init*, k_points, k_pose, k_eval -- as one wavefront and as the product's two-wavefront pair --, k_curv,
    then the Riccati sweep's own load phase, which adds the pi term in LDS: tests/emu/emu_pipe.cpp emu_stage_matrices)

satisfy  (T^-1 s)^T H (T^-1 r) = b + barrier term  within 10 x the probe's stored error estimate + 1e-9 x the probe's scale
(tests/hessian_pin_lib.py; T is built there from dt alone).  The two k_eval forms agree bitwise; kernel bodies and oracle agree
entry by entry to 1e-9 x max|H_stage|.  The worst ratio |difference| / tolerance per block is printed (DESIGN.md section 5 quotes it).

What a wrong Hessian looks like here (tried on scratch copies, not committed): without the `i < j` angular term of the q x dq
block in k_curv, and with lam_pi(k) in place of lam_pi(k+1), the q x dq / q x q probes miss their tolerance by four to six orders
of magnitude while the other blocks stay green.

Also: bmpc_oracle_debug_hess -- the analytic stage matrix against central differences of the oracle's own stage gradient (which is
pinned to the reference by tests/test_oracle_nlp.py), entry by entry: it localises to an entry where the probes localise to a block.
"""
import numpy as np
import pytest

import hessian_pin_lib as HP
import oracle_lib as O

BLOCKS = ("all", "own", "qxq", "qxdq", "qxpi", "dqxdq", "qxslacks", "pixpi", "dxd")


def _report(tag, N, ratios):
    worst = HP.worst_by_block(ratios)
    print(f"{tag} N={N}: " + ", ".join(f"{b} {worst[b][0]:.2g}" for b in BLOCKS if b in worst), flush=True)
    bad = [(b, k, f"{r:.3g}", got, want) for b, k, r, got, want in ratios if not r <= 1.0]
    assert not bad, f"{tag} N={N}: {len(bad)} of {len(ratios)} probes miss their tolerance (block, stage, ratio, got, expected): {bad[:8]}"


@pytest.mark.parametrize("N", HP.HORIZONS)
def test_fixture_covers_every_stage_and_block(golden_dir, N):
    fx = HP.load(golden_dir, N)
    assert int(fx["N"]) == N and len(fx["y_names"]) == 41
    kinds = [str(k) for k in fx["point_kind"]]
    assert any(k.startswith("split") for k in kinds) and any(k in ("cold", "iter8", "conv") for k in kinds)
    for ip in range(len(kinds)):
        mine = fx["pr_point"] == ip
        assert sorted(set(fx["pr_stage"][mine])) == list(range(1, N)), "every stage of every point has probes"
        assert (fx["dd_point"] == ip).any()
    assert sorted(set(fx["pr_block"])) == list(range(len(fx["block_names"]))), "every block occurs"
    assert np.all(fx["pr_err"] <= 1e-7 * fx["pr_scale"]) and np.all(fx["dd_err"] <= 1e-7 * fx["dd_scale"])
    assert np.all(np.isfinite(fx["pr_b"])) and np.all(fx["z_up"] >= 0) and np.all(fx["t_up"] > 0) and np.all(fx["t_lo"] > 0)


@pytest.mark.parametrize("N", HP.HORIZONS)
def test_oracle_meets_every_probe(golden_dir, N):
    fx = HP.load(golden_dir, N)
    ratios = []
    for ip in range(len(fx["w"])):
        w, lbx, ubx, p, t, z, lam_pi, rows = HP.point_inputs(fx, ip, O)
        H = O.stage_matrices(N, w, lbx, ubx, p, t, z, lam_pi, float(fx["dt"]))
        ratios += HP.probe_ratios(fx, ip, H, t, z, rows)
    assert len(ratios) == len(fx["pr_b"]) + len(fx["dd_b"])
    _report("oracle", N, ratios)


@pytest.mark.parametrize("N", HP.HORIZONS)
def test_kernel_bodies_meet_every_probe(golden_dir, N):
    import emu_pipe_lib as E
    fx = HP.load(golden_dir, N)
    P = len(fx["w"])
    inp = [HP.point_inputs(fx, ip, O) for ip in range(P)]
    slots = [HP.slot_arrays(N, i[7], i[4], i[5], fx["y_names"]) for i in inp]
    stack = lambda j: np.array([i[j] for i in inp])
    args = (stack(0), stack(1), stack(2), stack(3), np.array([s[0] for s in slots]), np.array([s[1] for s in slots]), stack(6))
    H1 = E.stage_matrices(N, *args, dt=float(fx["dt"]), split=0)
    H2 = E.stage_matrices(N, *args, dt=float(fx["dt"]), split=1)
    assert np.array_equal(H1, H2), "k_eval as one wavefront and as the two-wavefront pair differ"
    ratios, worst_o = [], 0.0
    for ip in range(P):
        w, lbx, ubx, p, t, z, lam_pi, rows = inp[ip]
        ratios += HP.probe_ratios(fx, ip, H2[ip], t, z, rows)
        Ho = O.stage_matrices(N, w, lbx, ubx, p, t, z, lam_pi, float(fx["dt"]))
        for k in range(N - 1):
            worst_o = max(worst_o, np.abs(H2[ip, k] - Ho[k]).max() / np.abs(Ho[k]).max())
    assert len(ratios) == len(fx["pr_b"]) + len(fx["dd_b"])
    print(f"kernel bodies against the oracle, N={N}: max |dH| / max|H_stage| = {worst_o:.2g}")
    assert worst_o <= 1e-9
    _report("kernel bodies", N, ratios)


@pytest.mark.parametrize("N,kinds", [(6, ("cold", "iter8", "conv", "split0", "split2")), (10, ("conv", "split1"))])
def test_oracle_stage_matrix_against_differences_of_its_gradient(golden_dir, N, kinds):
    """bmpc_oracle_debug_hess: H (without barrier terms) against central differences (step 1e-6 in zeta) of the stage's Lagrangian
    gradient gdual + A^T lam, every entry of every stage.  Bound 1e-6 x max|H_stage|: the truncation error of the difference is
    (1e-6)^2 / 6 x the third derivative of the gradient -- the sigmoid's argument is scaled by 60, so at most (60e-6)^2 / 6 = 6e-10
    relative -- and its rounding error is 2^-52 x |gradient| / 1e-6, with |gradient| up to 1e3 x max|H| at these points: 2e-7."""
    fx = HP.load(golden_dir, N)
    worst = 0.0
    for ip, kind in enumerate(str(k) for k in fx["point_kind"]):
        if kind not in kinds:
            continue
        w, lbx, ubx, p = HP.point_inputs(fx, ip, O)[:4]
        for k in range(1, N):
            Ha, Hf = O.debug_hess(N, w, lbx, ubx, p, k, 0.7, 0.3, float(fx["dt"]))
            assert np.abs(Ha - Ha.T).max() <= 1e-12 * np.abs(Ha).max()
            d = np.abs(Ha - Hf).max() / np.abs(Ha).max()
            worst = max(worst, d)
            i, j = np.unravel_index(np.argmax(np.abs(Ha - Hf)), Ha.shape)
            assert d <= 1e-6, f"N={N} {kind} stage {k}: entry ({HP.ZETA_NAMES[i]}, {HP.ZETA_NAMES[j]}) analytic {Ha[i, j]} differences {Hf[i, j]}"
    print(f"analytic stage matrix against differences of the stage gradient, N={N}: worst {worst:.2g} x max|H_stage|")
