"""The Newton step of the HIP kernels, pinned to a dense KKT solve (MI355X; tests/test_newton_step.py is the CPU half and documents
the checks, the profiles, the bounds and the figures they come from).

bmpc_debug_newton_step: slots initialised by the product's init launch, rows and the first attempt's Hessian mode overwritten, the
product's evaluation launches, the product's own Riccati launch in the variant the number of live instances selects, bmpc_k_fwd,
bmpc_k_step, and a copy-out kernel.  The cases of newton_step_lib.CASES run below BMPC_RIC_SPEC_BELOW / BMPC_RIC_LAT_BELOW
(bmpc_k_ric_att + bmpc_k_ric_sel); one more batch at N = 6 has as many instances as the larger of the two thresholds, so that the
throughput variant bmpc_k_ric runs -- 32 distinct problems repeated to fill it, every one compared, every copy bitwise equal to
the first.  The bounds are those of the CPU half (32 x the oracle's own error); the run prints its worst ratios per case.

Reads the oracle library and the scene generator only.
"""
import os
import re

import numpy as np
import pytest

import newton_step_lib as NS
import oracle_lib as O

pytestmark = pytest.mark.gpu


def _handle(N):
    from boundplanner_amd.solver import HipBoundMPC
    return HipBoundMPC(N)


def _run(h, bt, sub=None):
    s = slice(None) if sub is None else sub
    return h.newton_step(bt["x0"][s], bt["lbx"][s], bt["ubx"][s], bt["p"][s], bt["TS"][s], bt["ZS"][s], bt["mode"][s])


@pytest.mark.parametrize("N,B,profile,seed", NS.CASES)
def test_hip_kernels_meet_the_dense_solve(N, B, profile, seed):
    bt = NS.make_batch(N, B, seed, profile)
    h = _handle(N)
    out = _run(h, bt)
    NS.check_case(bt, profile, *out, O, f"HIP kernels N={N} B={B} ({profile})")
    if B == 67:          # position independence: first / last instance of a wavefront's lanes, the ragged last wavefront
        ipw = 64 // (N - 1)
        for j in (0, ipw - 1, ipw, B - 1):
            alone = _run(h, bt, slice(j, j + 1))
            for a, b in zip(alone, out):
                assert np.array_equal(a[0], b[j], equal_nan=True), f"instance {j} alone differs from instance {j} of the batch"


def _threshold():
    """the larger of the two launch thresholds, from the source's constants"""
    src = open(os.path.join(O.ROOT, "boundplanner_amd", "csrc", "bmpc_pipeline.hip")).read()
    vals = [int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1)) for name in ("BMPC_RIC_SPEC_BELOW", "BMPC_RIC_LAT_BELOW")]
    return max(vals)


@pytest.mark.parametrize("N,D,profile,seed", NS.THROUGHPUT_CASES)
def test_throughput_variant_meets_the_dense_solve(N, D, profile, seed):
    B = _threshold()                 # not below either threshold: bmpc_k_ric
    assert B % D == 0
    bt = NS.make_batch(N, D, seed, profile)
    rep = lambda a: np.concatenate([a] * (B // D))
    big = {k: (rep(v) if isinstance(v, np.ndarray) else v) for k, v in bt.items()}
    out = _run(_handle(N), big)
    for a in out:
        assert np.array_equal(a, rep(a[:D]), equal_nan=True), "copies of one problem at other positions of the batch differ"
    NS.check_case(bt, profile, *(a[:D] for a in out), O, f"HIP kernels, throughput variant, N={N} B={B} ({profile})")
