"""The filter line search of the HIP kernels, pinned to an independent check (MI355X; tests/test_line_search.py is the CPU half,
tests/line_search_lib.py documents the reference, the acceptance rule, the cases, the classes of search and the bounds).

bmpc_debug_line_search: the sequence of bmpc_debug_newton_step, line-search state planted before the evaluation launches and after
bmpc_k_step, then the product's trial launch once.  The cases of line_search_lib.CASES have fewer groups of pairs than
BMPC_TRIAL_SPEC_WGS and run bmpc_k_trial_spec; one more batch at N = 6 has just enough instances for more groups than that and runs
bmpc_k_trial -- 32 distinct problems repeated, every copy bitwise the first, and the 32 bitwise what the same problems give as a
small batch under bmpc_k_trial_spec.  Each case runs twice (the first run gives what the reference and the planted state are
computed from).  The run prints its worst ratios per case.

Reads the oracle library and the scene generator only.
"""
import os
import re

import numpy as np
import pytest

import line_search_lib as L
import newton_step_lib as NS
import oracle_lib as O

pytestmark = pytest.mark.gpu
NEWTON = ("dzeta", "dt", "dz", "state", "zeta0", "t0", "z0")


def _handle(N):
    from boundplanner_amd.solver import HipBoundMPC
    return HipBoundMPC(N)


def _run(h, bt, P0=None, P1=None, sub=None, cold=False):
    s = slice(None) if sub is None else sub
    rows = (None, None, None) if cold else (bt["TS"][s], bt["ZS"][s], bt["mode"][s])
    return h.line_search(bt["x0"][s], bt["lbx"][s], bt["ubx"][s], bt["p"][s], *rows,
                         plant0=None if P0 is None else P0[s], plant1=None if P1 is None else P1[s])


def same_search(a, b, live):
    """two runs of a search agree bitwise in everything but the slots of t1 that no row uses"""
    diff = [k for k in a if not (np.array_equal(a[k], b[k], equal_nan=True) if k != "t1" else np.array_equal(a["t1"][live], b["t1"][live]))]
    assert not diff, f"two runs of one search differ in {diff}"
    return True


@pytest.mark.parametrize("ci", range(len(L.CASES)))
def test_hip_line_search_meets_the_reference(ci):
    N, B, profile, seed = L.CASES[ci]
    bt = NS.make_batch(N, B, seed, profile)
    h = _handle(N)
    first = _run(h, bt)
    P0, P1, info = L.plans_for(bt, profile, first, O, ci)
    out = _run(h, bt, P0, P1)
    for k in NEWTON:          # (state[0] is the planted iteration counter itself)
        a, b = (first[k], out[k]) if k != "state" else (first[k][:, 1:], out[k][:, 1:])
        assert np.array_equal(a, b, equal_nan=True), f"{k} depends on the planted line-search state"
    L.check_case(bt, profile, out, info, True, O, f"HIP bmpc_k_trial_spec N={N} B={B} ({profile})", L.wanted_classes(ci, B))
    if B == 67:          # position independence: first / last instance of a wavefront's lanes, the ragged last wavefront
        ipw = 64 // (N - 1)
        for j in (0, ipw - 1, ipw, B - 1):
            alone = _run(h, bt, P0, P1, slice(j, j + 1))
            assert same_search(alone, {k: v[j:j + 1] for k, v in out.items()}, bt["ZS"][j:j + 1] > 0), f"instance {j} alone differs from instance {j} of the batch"


def _spec_wgs():
    """groups of pairs up to which bmpc_k_trial_spec runs, from the source's constant"""
    src = open(os.path.join(O.ROOT, "boundplanner_amd", "csrc", "bmpc_pipeline.hip")).read()
    return int(re.search(r"#define\s+BMPC_TRIAL_SPEC_WGS\s+(\d+)", src).group(1))


def test_sequential_variant_meets_the_reference_and_the_speculative_one():
    N, D, profile, seed = L.SPEC_CASE
    ci = L.CASES.index(L.SPEC_CASE)
    ipw = min(64 // (N - 1), 8)
    B = (_spec_wgs() * ipw // D + 1) * D          # more groups of pairs than BMPC_TRIAL_SPEC_WGS: bmpc_k_trial
    assert -(-B // ipw) > _spec_wgs()
    bt = NS.make_batch(N, D, seed, profile)
    h = _handle(N)
    first = _run(h, bt)
    P0, P1, info = L.plans_for(bt, profile, first, O, ci)
    small = _run(h, bt, P0, P1)
    rep = lambda a: np.concatenate([a] * (B // D))
    big = {k: (rep(v) if isinstance(v, np.ndarray) else v) for k, v in bt.items()}
    out = _run(h, big, rep(P0), rep(P1))
    for k, a in out.items():
        assert np.array_equal(a, rep(a[:D]), equal_nan=True), f"{k}: copies of one problem at other positions of the batch differ"
    head = {k: a[:D] for k, a in out.items()}
    L.check_case(bt, profile, head, info, False, O, f"HIP bmpc_k_trial N={N} B={B} ({profile})", L.wanted_classes(ci, D))
    assert same_search(head, small, bt["ZS"] > 0), "bmpc_k_trial and bmpc_k_trial_spec differ"


def test_cold_start_pins_the_merit_pieces_of_the_init_launch():
    N, B, seed = L.COLD_CASE
    from boundplanner_amd import scenes
    b = scenes.make_batch(B, N, seed, O.fk_batch, randomize_sets=True)
    x0 = b["x0"] + 1e-2 * np.random.default_rng(seed + 2).normal(size=b["x0"].shape)
    st0 = np.arange(40) * N
    x0[:, st0] = b["lbx"][:, st0]
    bt = dict(N=N, B=B, x0=x0, lbx=b["lbx"], ubx=b["ubx"], p=b["p"])
    L.check_cold(bt, _run(_handle(N), bt, cold=True), O, f"HIP cold start N={N} B={B}")
