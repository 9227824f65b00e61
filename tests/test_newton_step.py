"""The Newton step of one interior-point iteration, pinned to a dense KKT solve (CPU half; tests/test_newton_step_gpu.py is the
MI355X half).

What is compared: the step dzeta, the row steps dt, dz and the fraction-to-boundary lengths that one super-step of the kernel
bodies returns (tests/emu/emu_pipe.cpp emu_newton_step: k_init*, rows overwritten, k_points, k_pose, k_eval, k_curv, the Riccati
body, k_fwd, k_step), and the oracle's own riccati_backward / riccati_forward step, against the solution of the linear system the
oracle states stage by stage (bmpc_oracle_newton_system), solved densely with extended-precision refinement and WITHOUT a Riccati
recursion (tests/newton_step_lib.py, which also says where delta_w and the fixed 1e-9 sit in that system and how that was checked).

Asserted per case (newton_step_lib.CASES and THROUGHPUT_CASES; cold starts of scenes.make_batch(randomize_sets=True) with seeded rows: (a) log-normal
t, z; (b) a late iteration, a quarter of the rows nearly active with t down to 1e-8 and z / t up to ~1e10, the rest slack;
(c) exact Hessian, with instances that factorise as they are, that fall back to Gauss-Newton and that get delta_w > 0 -- each
outcome must occur):
  * at most 2 % of the instances without a step;
  * the oracle's A_k, B_k equal the jerk integrator stated in numpy from dt, outside the pi rows;
  * dynamics rows of the returned step, relative to max(|dx|, |r|) of the stage;
  * || dzeta - dzeta* ||_M / || dzeta* ||_M with M = Z^T H Z;
  * dt_i, dz_i of every live row against the reference step's, relative to the sum of the absolute terms of each; padding slots
    are left UNTOUCHED by k_step (the entry plants a NaN in every slot beforehand: NaN exactly off the live rows);
  * the step lengths against the minima recomputed from the kernel's own returned rows (<= 16 ulp: the reduction over rows, pairs
    and wavefronts alone) and against the reference step's;
  * instances run alone give bitwise what they give inside the batch (first / last lane group of a wavefront, last instance).

Bounds: 32 x the worst figure of the oracle's own step per profile (two FP64 implementations of one recursion differ in summation
order and FMA contraction; the iterate-parity record shows such noise within a factor <= 35 between runs).  Measured on these
cases (oracle, worst per profile; dynamics / energy / dt / dz / step lengths):
    (a) 2.9e-16  1.4e-15  9.2e-15  3.5e-15  1.8e-14
    (b) 2.2e-16  2.3e-10  6.9e-6   3.0e-7   6.0e-10
    (c) 2.1e-16  6.8e-14  1.0e-12  9.2e-13  5.0e-13
(the problems of the GPU half's throughput-variant batch, newton_step_lib.THROUGHPUT_CASES, are among the cases: they hold the
worst of (a)'s step lengths and of (c)'s energy, dt, dz and step lengths), so the energy-norm bounds are 4.8e-14, 7.7e-9 and 2.2e-12.  The emulated kernels use at most 0.25 of any bound (the printed ratios).
Profile (b) stays below the 1e-6 limit on the energy bound as specified: it was not softened.

Shown to bite on scratch copies of the kernel source under this emulation (factor by which the worst figure misses its bound;
cases N=4 (a) / N=6 (c) / N=20 (b)): the P r_k term of the coupling phase dropped -- energy 3.2e10 / 4.1e9 / 1.5e5; the stage's own
g1 in place of the value-function gradient p_{k+1} in the coupling phase's mu part -- energy 7.6e9 / 7.3e9 / 1.5e6 or more (it varies between runs); the
step-length maxima of k_step skipping one row group (the box rows of q) -- own step lengths 5.5e13 x their 16 ulp, and 9.9e6 x the bound against the reference's, at N=20 (b).  With the
unperturbed cold start, whose defects r_k are zero, the first mutation passed: hence the perturbation in make_batch.

Reads the oracle library and the scene generator only.
"""
import numpy as np
import pytest

import emu_pipe_lib as E
import newton_step_lib as NS
import oracle_lib as O


def _run(bt, variant=0, sub=None):
    s = slice(None) if sub is None else sub
    return E.newton_step(bt["N"], bt["x0"][s], bt["lbx"][s], bt["ubx"][s], bt["p"][s], bt["TS"][s], bt["ZS"][s], bt["mode"][s], variant=variant)


@pytest.mark.parametrize("N,B,profile,seed", NS.CASES + NS.THROUGHPUT_CASES)
def test_emulated_kernels_and_oracle_meet_the_dense_solve(N, B, profile, seed):
    bt = NS.make_batch(N, B, seed, profile)
    out = _run(bt)
    NS.check_case(bt, profile, *out, O, f"emulated kernels N={N} B={B} ({profile})")
    if B == 67:          # position independence: first / last instance of a wavefront's lanes, the ragged last wavefront
        ipw = 64 // (N - 1)
        for j in (0, ipw - 1, ipw, B - 1):
            alone = _run(bt, sub=slice(j, j + 1))
            for a, b in zip(alone, out):
                assert np.array_equal(a[0], b[j], equal_nan=True), f"instance {j} alone differs from instance {j} of the batch"


def test_speculative_riccati_pair_gives_the_same_step():
    """the deep tail's kernels (k_ric_att + k_ric_sel bodies) on the case with all three factorisation outcomes: bitwise the
    step of k_ric_body, and so within the same bounds"""
    N, B, profile, seed = 6, 12, "c", 7206
    bt = NS.make_batch(N, B, seed, profile)
    ref, spec = _run(bt, 0), _run(bt, 1)
    NS.check_case(bt, profile, *spec, O, f"emulated speculative pair N={N} B={B} (c)")
    for a, b in zip(ref[:3], spec[:3]):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(ref[3][:, :9], spec[3][:, :9])
