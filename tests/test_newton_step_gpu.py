"""The Newton step of the HIP kernels, pinned to a dense KKT solve (MI355X; tests/test_newton_step.py is the CPU half and documents
the checks, the profiles, the bounds and the figures they come from).

bmpc_debug_superstep stopped after the direction launches: slots initialised by the product's init launch, rows and the first attempt's Hessian mode overwritten, the
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


def test_entries_of_different_kinds_leave_nothing_behind_on_a_handle():
    """Solves and the two test entries share the builder of the argument block and the seed of the pool (bmpc_capi.hip: pipe_args,
    pipe_seed).  One handle, N = 4, B = 5 (one ragged wavefront holding several instances): solve, newton_step, line_search, stage_matrices,
    solve, newton_step, line_search.  Repeats of a kind are bitwise equal, and equal to what a fresh handle returns when that kind of call is
    its first (np.array_equal; bit patterns for newton_step) -- the same kernels run on the same inputs in slots 0 .. B-1.  Directly after a test entry the multipliers of "the
    last solve" are refused (its iterates are gone from the workspace) and the output buffers stay untouched."""
    import torch
    N, B = 4, 5
    bt = NS.make_batch(N, B, 11, "a")
    lam_pi = np.random.default_rng(12).normal(size=(B, N, 3))
    solve = lambda h: h.solve_batch(bt["x0"], bt["lbx"], bt["ubx"], bt["p"])
    stage = lambda h: h.stage_matrices(bt["x0"], bt["lbx"], bt["ubx"], bt["p"], bt["TS"], bt["ZS"], lam_pi)
    same_solve = lambda a, b: all(np.array_equal(a[k], b[k]) for k in ("x", "f", "viol", "iters", "status"))
    # dt and dz carry the NaN that bmpc_k_dbg_set_rows plants in the slots no row uses, and a NaN is not equal to itself: the
    # newton_step results are compared bit pattern by bit pattern (stricter than np.array_equal where that can hold at all)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    same = lambda a, b: all(u.shape == v.shape and np.array_equal(bits(u), bits(v)) for u, v in zip(a, b))
    h = _handle(N)
    lg = torch.full((B, h.n_g), -7.0, dtype=torch.float64, device="cuda:0"); lx = torch.full((B, h.n_w), -7.0, dtype=torch.float64, device="cuda:0")

    def refused():
        with pytest.raises(RuntimeError, match=r"\(1\).*no finished solve of this batch size"):
            h.multipliers_dev(B, lg.data_ptr(), lx.data_ptr())
        assert bool((lg == -7.0).all()) and bool((lx == -7.0).all()), "a refused request wrote multipliers"

    # (t1 only in the slots a row uses: when the accepted trial is not the first, bmpc_k_trial_spec copies whole candidate records over,
    # and the slots no row uses then hold what the dead gain copies held -- include/boundmpc.h)
    def search(h):
        r = h.line_search(bt["x0"], bt["lbx"], bt["ubx"], bt["p"], bt["TS"], bt["ZS"], bt["mode"])
        return tuple(np.where(bt["ZS"] > 0, v, 0.0) if k == "t1" else v for k, v in r.items())
    s1 = solve(h)
    n1 = _run(h, bt); refused()
    l1 = search(h); refused()
    m1 = stage(h); refused()
    s2 = solve(h)
    h.multipliers_dev(B, lg.data_ptr(), lx.data_ptr())      # (after a solve they are there)
    assert bool((lg != -7.0).any())
    lg.fill_(-7.0); lx.fill_(-7.0)
    n2 = _run(h, bt); refused()
    l2 = search(h); refused()
    assert same_solve(s1, s2), "the second solve differs from the first: a test entry left something on the handle"
    assert same(n1, n2), "the second newton_step differs from the first: a solve left something on the handle"
    assert same(l1, l2), "the second line_search differs from the first: a solve or another entry left something on the handle"
    assert same(l1, search(_handle(N))), "line_search after a solve differs from a fresh handle's first call"
    assert same(l1[:4], n1), "line_search returns another Newton step than newton_step"
    assert same_solve(s1, solve(_handle(N))), "solve differs from a fresh handle's"
    assert same(n1, _run(_handle(N), bt)), "newton_step after a solve differs from a fresh handle's first call"
    assert np.array_equal(m1, stage(_handle(N))), "stage_matrices after a solve and a newton_step differs from a fresh handle's first call"


def test_a_misused_entry_is_refused_and_leaves_nothing_behind():
    """bmpc_debug_superstep checks its record on the host before anything is launched (include/boundmpc.h).  N = 4, B = 2: every
    misuse raises with rc 1, and the newton_step that follows on the same handle has the bit patterns of a fresh handle's.  A
    handle whose line search does not end inside one launch (trial_repeats = 1) is refused the line search and served the Newton
    step."""
    from boundplanner_amd.solver import STOPS, HipBoundMPC
    N, B = 4, 2
    bt = NS.make_batch(N, B, 11, "a")
    lam_pi = np.random.default_rng(12).normal(size=(B, N, 3))
    prob = dict(x0=bt["x0"], lbx=bt["lbx"], ubx=bt["ubx"], p=bt["p"])
    rows = dict(prob, t=bt["TS"], z=bt["ZS"], mode=bt["mode"])
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    same = lambda a, b: all(u.shape == v.shape and np.array_equal(bits(u), bits(v)) for u, v in zip(a, b))
    fresh = _run(_handle(N), bt)
    h = _handle(N)
    misuses = {
        "t without z": (STOPS["newton"], dict(prob, t=bt["TS"], mode=bt["mode"])),
        "a plant without rows": (STOPS["ls"], dict(prob, plant0=np.full((B, 22), np.nan))),
        "mode = 3": (STOPS["newton"], dict(rows, mode=3)),
        "H together with the ls group": (STOPS["H"] + STOPS["ls"], dict(rows, lam_pi=lam_pi)),
        "H without lam_pi": (STOPS["H"], rows),
        "ctl without the ls group": (STOPS["newton"] + ("ctl",), rows),
    }
    for what, (want, arrays) in misuses.items():
        with pytest.raises(RuntimeError, match=r"\(1\)"):
            h._superstep(want, **arrays)
        assert same(fresh, _run(h, bt)), f"newton_step after the refusal of {what} differs from a fresh handle's"
    short = HipBoundMPC(N, trial_repeats=1)
    with pytest.raises(RuntimeError, match=r"\(1\).*trial_repeats"):
        short.line_search(*(rows[k] for k in ("x0", "lbx", "ubx", "p", "t", "z", "mode")))
    assert same(fresh, _run(short, bt)), "newton_step of a handle with trial_repeats = 1 differs from the default handle's"
