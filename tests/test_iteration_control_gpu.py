"""The KKT error and the iteration control of the HIP kernels, pinned to an independent check (MI355X;
tests/test_iteration_control.py is the CPU half, tests/iteration_control_lib.py documents the reference, the rule, the cases, the classes
and the bounds).

bmpc_debug_iteration_control: the sequence of bmpc_debug_line_search with the iteration-control state planted per instance before the
evaluation launches and copied out after the direction launches and after the trial launch.  The cases of iteration_control_lib.CASES
are small batches and run bmpc_k_ric_att + bmpc_k_ric_sel; one more batch at N = 6, filled to the larger launch threshold with copies
of 32 problems, runs bmpc_k_ric -- every copy bitwise the first.  Every setting of a case (tol, max_iter, mu_floor_k, dw0) uses a handle of
its own.  The run prints its worst ratios per case.

For the profiles of iteration_control_lib.NO_ATTEMPTS ("x", "d": exact solutions) delta_w, tries, gn_back, gn_skip, dw_last and hess_mode
after the search are not compared (the library's docstring says why); for every other profile they are.

Reads the oracle library and the scene generator only.
"""
import os
import re

import numpy as np
import pytest

import iteration_control_lib as IC
import oracle_lib as O

pytestmark = pytest.mark.gpu


def _handle(N, o):
    from boundplanner_amd.solver import HipBoundMPC
    return HipBoundMPC(N, tol=o["tol"], max_iter=o["max_iter"], mu_floor_k=o["mu_floor_k"], dw0=o["dw0"])


def _run(h, bt, plant, sub=None):
    s = slice(None) if sub is None else sub
    return h.iteration_control(bt["x0"][s], bt["lbx"][s], bt["ubx"][s], bt["p"][s], bt["TS"][s], bt["ZS"][s], bt["mode"][s], plant[s])


def same(a, b, live):
    return [k for k in a if not (np.array_equal(a[k], b[k], equal_nan=True) if k != "t1" else np.array_equal(a["t1"][live], b["t1"][live]))]


@pytest.mark.parametrize("ci", range(len(IC.CASES)))
def test_hip_iteration_control_meets_the_reference(ci):
    N, B, profile, seed = IC.CASES[ci]
    bt = IC.make_batch(N, B, seed, profile, O)
    reached = set()
    for setting in IC.SETTINGS_OF(N, profile):
        o, plant = IC.opts_of(setting), IC.plant_for(setting, ci, B, bt)
        h = _handle(N, o)
        out = _run(h, bt, plant)
        ms, cls = IC.check_case(bt, profile, out, plant, o, O, f"HIP bmpc_k_ric_att + bmpc_k_ric_sel N={N} B={B} ({profile}) {setting}", with_oracle=False)
        reached |= cls
        if B == 67:          # position independence: first / last instance of a wavefront's lanes, the ragged last wavefront
            ipw = 64 // (N - 1)
            for j in (0, ipw - 1, ipw, B - 1):
                alone = _run(h, bt, plant, slice(j, j + 1))
                diff = same(alone, {k: v[j:j + 1] for k, v in out.items()}, bt["ZS"][j:j + 1] > 0)
                assert not diff, f"instance {j} alone differs from instance {j} of the batch in {diff}"
        h.close()
    missing = set(IC.CASE_CLASSES[ci]) - reached
    assert IC.CASE_CLASSES[ci] and not missing, f"case {ci} N={N} B={B} ({profile}): classes {sorted(missing)} did not occur"


def _threshold(name):
    src = open(os.path.join(O.ROOT, "boundplanner_amd", "csrc", "bmpc_pipeline.hip")).read()
    return int(re.search(rf"#define\s+{name}\s+(\d+)", src).group(1))


def test_throughput_variant_meets_the_reference_and_every_copy_is_the_first():
    N, D, profile, seed = IC.THROUGHPUT_CASE
    ci = len(IC.CASES)
    B = (max(_threshold("BMPC_RIC_SPEC_BELOW"), _threshold("BMPC_RIC_LAT_BELOW")) // D + 1) * D      # neither the speculative pair nor bmpc_k_ric_lat
    bt = IC.make_batch(N, D, seed, profile, O)
    o, plant = IC.opts_of("default"), IC.plant_for("default", ci, D)
    rep = lambda a: np.concatenate([a] * (B // D))
    big = {k: (rep(v) if isinstance(v, np.ndarray) else v) for k, v in bt.items()}
    h = _handle(N, o)
    out = _run(h, big, rep(plant))
    stepped = out["ctl"][:, IC.CTL["status"]] == -1      # (a finished instance never reaches the line-search start: its record there is no state)
    for k, a in out.items():
        rows = slice(None) if k in ("ctl", "state") else stepped
        assert np.array_equal(a[rows], rep(a[:D])[rows], equal_nan=True), f"{k}: copies of one problem at other positions of the batch differ"
    head = {k: a[:D] for k, a in out.items()}
    ms, cls = IC.check_case(bt, profile, head, plant, o, O, f"HIP bmpc_k_ric N={N} B={B} ({profile})", with_oracle=False)
    missing = {"first_attempt", "gn_allowed", "gn_refused_err", "dw_x8", "dead"} - cls      # (of the default setting alone)
    assert not missing, f"classes {sorted(missing)} did not occur"
    small = _run(h, bt, plant)
    assert np.array_equal(small["ctl"][:, IC.CONTROL], head["ctl"][:, IC.CONTROL]), "bmpc_k_ric and the speculative pair differ in the control state"
